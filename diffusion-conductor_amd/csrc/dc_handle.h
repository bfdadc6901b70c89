// dc_handle.h - host scaffold of the evaluation networks' handles (dc_stgcn.hip, dc_m2snet.hip, dc_m2sgan.hip, dc_rhythm.hip; dc_loss.hip takes
// the error macro): what each of them needs around its kernels and at least two of them share.  Internal, host only.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/dc_ddim.h"
#include "dc_music.h"   // DcParams, DcParamList (dc_pack.h); the music encoder a handle may own

int dc_set_error(int code, const char* msg);      // dc_api.hip: sets dc_last_error's message

#define DC_HIP_TRY(expr)                                                                                              \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return dc_set_error(DC_ERR_HIP, (std::string(#expr) + " failed: " + hipGetErrorString(e_)).c_str()); \
    } while (0)

inline bool starts_with(const std::string& s, const std::string& p) { return s.rfind(p, 0) == 0; }
inline bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

// the device ordinal a `fn` (PREFIX_create) was given
inline int dc_check_device(const char* fn, int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return dc_set_error(DC_ERR_NO_DEVICE, (std::string(fn) + ": no HIP device visible").c_str());
    if (device < 0 || device >= n) return dc_set_error(DC_ERR_INVALID, (std::string(fn) + ": no device " + std::to_string(device)).c_str());
    return DC_OK;
}

// Makes `device` current for a scope and puts the caller's device back: a destroy must not leave the process on the handle's
// device.  (A failure in a destructor has nobody to report to.)
struct DcDeviceGuard {
    int prev = -1;
    explicit DcDeviceGuard(int device) {
        (void)hipGetDevice(&prev);
        (void)hipSetDevice(device);
    }
    ~DcDeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DcDeviceGuard(const DcDeviceGuard&) = delete;
};

// A handle's activation planes on the current device: grown on demand, never shrunk.
struct DcWorkspace {
    float* p = nullptr;
    size_t floats = 0;
    int reserve(size_t n, hipStream_t st) {
        if (floats >= n) return DC_OK;
        if (p) {
            DC_HIP_TRY(hipStreamSynchronize(st));    // (the previous call's work on this stream may still read the old planes)
            DC_HIP_TRY(hipFree(p));
            p = nullptr;
            floats = 0;
        }
        DC_HIP_TRY(hipMalloc((void**)&p, n * sizeof(float)));
        floats = n;
        return DC_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        floats = 0;
    }
};

// f(b0, nb) -> int for the clips [b0, b0 + nb) of B in passes of at most `chunk`; stops at the first non-zero and returns it
template <class F>
inline int dc_chunks(int B, int chunk, F&& f) {
    for (int b0 = 0; b0 < B; b0 += chunk)
        if (const int rc = f(b0, B - b0 < chunk ? B - b0 : chunk)) return rc;
    return DC_OK;
}

// ---- parameter intake ---------------------------------------------------------------------------------------------
// One state_dict entry of the network `what` ("M2SNet": the subject of the error texts) against its (name, numel) lists.  `key` in
// `used` with the right size: stored in *dst and *changed set (dst == NULL: checked and dropped).  In `unused`, or the
// num_batches_tracked counter (one element) of a BatchNorm whose running_mean is used - state_dict entries eval mode never
// applies -: checked and dropped.  Anything else is DC_ERR_PARAM.  `given`: the caller's spelling of `key`, for the texts.
inline int dc_param_take(const char* what, const DcParamList& used, const DcParamList& unused, const std::string& key, const std::string& given,
                         const float* h_data, int64_t numel, DcParams* dst, bool* changed = nullptr) {
    const auto sized = [&](size_t want) {
        if ((size_t)numel == want) return (int)DC_OK;
        return dc_set_error(DC_ERR_PARAM, (std::string(what) + " parameter " + given + " has " + std::to_string(numel) + " elements, expected " +
                                           std::to_string(want)).c_str());
    };
    for (const auto& r : used)
        if (r.first == key) {
            const int rc = sized(r.second);
            if (rc == DC_OK && dst) {
                (*dst)[key].assign(h_data, h_data + numel);
                if (changed) *changed = true;
            }
            return rc;
        }
    for (const auto& r : unused)
        if (r.first == key) return sized(r.second);
    const std::string nbt = ".num_batches_tracked";
    if (ends_with(key, nbt)) {
        const std::string rm = key.substr(0, key.size() - nbt.size()) + ".running_mean";
        for (const auto& r : used)
            if (r.first == rm) return sized(1);
    }
    return dc_set_error(DC_ERR_PARAM, (std::string("unknown ") + what + " parameter " + given).c_str());
}
// finalize's half: every entry of `used` was set
inline int dc_param_complete(const char* what, const DcParamList& used, const DcParams& have) {
    for (const auto& r : used)
        if (!have.count(r.first)) return dc_set_error(DC_ERR_PARAM, (std::string(what) + " parameter " + r.first + " was not set").c_str());
    return DC_OK;
}

// ---- the music encoder a handle owns ------------------------------------------------------------------------------
// Built from the handle's own `music_encoder.*` entries (no proj), pinned to the split format: a metric's or a baseline's numbers
// must not move with DC_ME_PREC, and have no use for the fp16 planes' 3.7e-4.
struct DcOwnedMusic {
    DcParams params;
    dc_music* enc = nullptr;
    int take(const char* what, int channels, const std::string& key, const float* h_data, int64_t numel, bool* changed) {
        return dc_param_take(what, dc_music_required(channels, false), {}, key, key, h_data, numel, &params, changed);
    }
    int check(const char* what, int channels) const {
        std::string err;
        if (dc_music_check(params, channels, &err, false)) return DC_OK;
        return dc_set_error(DC_ERR_PARAM, (std::string(what) + " music encoder: " + err).c_str());
    }
    // on the current device (dc_music_build runs dc_music_check itself; `check` lets a finalize refuse before it touches the device)
    int rebuild(const char* what, int channels) {
        if (enc) {
            DC_HIP_TRY(hipDeviceSynchronize());     // (work of earlier calls may still read the old weights)
            release();
        }
        std::string err;
        enc = dc_music_build(params, channels, &err, false);
        if (!enc) return dc_set_error(DC_ERR_PARAM, (std::string(what) + " music encoder: " + err).c_str());
        dc_music_pin_format(enc, DC_ME_SPLIT);
        return DC_OK;
    }
    int encode(const char* what, const float* d_mel, int B, int Tm, float* d_out, hipStream_t st) {
        std::string err;
        const hipError_t e = dc_music_encode(enc, d_mel, B, Tm, nullptr, d_out, st, &err);
        if (e != hipSuccess) return dc_set_error(DC_ERR_HIP, (std::string(what) + " music encoder: " + hipGetErrorString(e) + " " + err).c_str());
        return DC_OK;
    }
    void release() {
        dc_music_destroy(enc);
        enc = nullptr;
    }
};
