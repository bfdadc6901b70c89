// dc_m2snet.hip - M2SNet, the reference's learned music-motion synchronisation discriminator, on gfx950 (MI355X).
//
// Reference (restated, not translated): Contrastive_Stage/models/M2SNet.py:7-36 in eval mode,
//   hx = music_encoder(mel)        [B, T, 64]   MusicEncoder.py:30-53 - the layers of dc_music.hip, without the denoiser's proj
//   hy = motion_encoder(motion)    [B, T, 64]   MotionEncoder.py:6-27 - dc_stgcn.hip, which keeps it as [B, 64, T]
//   out = fuse_layer(cat(hx, hy))  [B, T, 1]    Conv1d(128 -> 64, 1), ReLU, Conv1d(64 -> 64, 1), ReLU, Conv1d(64 -> 1, 1), Sigmoid
// The handle owns one dc_music (built from M2SNet's own `music_encoder.*` entries, split planes, pinned) and one
// dc_motion_encoder; both run through their existing entry points.  Only the fuse head is a kernel of this file.
//
// k_m2s_head: one wave = 32 frames of ONE clip on the lanes (lane l: frame l & 31, k half l >> 5), v_mfma_f32_32x32x2_f32 with
// the weights as lane-major A fragments read from L2 (dc_pack.h, m2s_head_pack), as k_stgcn_fc does.  The music latent is
// [B][T][64], channel-contiguous: a lane loads its frame's row as 16 float4 and picks channel 2 ks + (l >> 5) per k-step; the
// motion latent is [B][64][T], time-contiguous: one coalesced load per k-step.  No transposing pass, no LDS.
// Layers 1 and 2 take the previous accumulator as their B operand: an accumulator register of lane (j, h) holds channel
// (r & 3) + 8 (r >> 2) + 4 h of frame j, the B operand of k-step ks wants channel 2 ks + h - both channels of a k-step live in the
// same half of the wave, so one exchange with lane l ^ 32 per k-step hands the other half its value.  The last conv (one output
// row) runs as an MFMA as well, w2 in row 0 of its fragments, so that every output of the head is one k-ordered fmaf chain
// (k = 0 .. K-1, the bias added last) - no partial sums, no reduction across lanes, frames or clips: a frame's result depends on
// its own 128 inputs only and is bit-identical in any batch.  ReLU is a select (NaN stays NaN, as torch.relu).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/dc_ddim.h"
#include "dc_common.h"
#include "dc_mfma_f32.h"
#include "dc_music.h"

int dc_set_error(int code, const char* msg);      // dc_api.hip: sets dc_last_error's message

namespace {

using namespace dc_f32;

constexpr int MH_C = 64;                   // channels of either latent and of both hidden layers
constexpr int MH_WAVES = 4;                // waves (32-frame tiles of one clip) per workgroup
constexpr int MH_CHUNK = 64;               // clips per pass of dc_m2snet_score (bounds the two latent planes: 2 x 64 x 64 x T floats)
constexpr int MH_GRID_Y = 1024;            // clips per launch of the head

// mus [B][T][64], mot [B][64][T] -> prob [B][T] (and logit [B][T] unless NULL).  Frames >= T of a partial tile read frame T - 1
// (in bounds; an MFMA column depends on its own frame only) and are not written.
__global__ __launch_bounds__(64 * MH_WAVES) void k_m2s_head(const float* __restrict__ mus, const float* __restrict__ mot,
                                                            const float* __restrict__ P, float* __restrict__ prob,
                                                            float* __restrict__ logit, int T) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int t0 = (blockIdx.x * MH_WAVES + (threadIdx.x >> 6)) * 32;
    if (t0 >= T) return;                 // wave-uniform; no barriers below
    const int b = blockIdx.y, t = t0 + j;
    const bool tv = t < T;
    const int tc = tv ? t : T - 1;

    // layer 0: 128 -> 64.  k = 0 .. 63 the music latent, k = 64 .. 127 the motion latent (torch.cat([hx, hy], dim=2))
    const f32x4* mrow = reinterpret_cast<const f32x4*>(mus + ((size_t)b * T + tc) * MH_C);
    f32x4 m[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = mrow[i];
    const float* w0 = P + kHeadW0;
    f32x16 a0 = {}, a1 = {};
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const float x = h ? m[ks >> 1][2 * (ks & 1) + 1] : m[ks >> 1][2 * (ks & 1)];      // channel 2 ks + h
        a0 = mfma2(w0[ks * 64 + lane], x, a0);
        a1 = mfma2(w0[(64 + ks) * 64 + lane], x, a1);
    }
    const float* src = mot + (size_t)b * MH_C * T + tc;
#pragma unroll 8
    for (int ks = 0; ks < 32; ++ks) {
        const float x = src[(size_t)(2 * ks + h) * T];
        a0 = mfma2(w0[(32 + ks) * 64 + lane], x, a0);
        a1 = mfma2(w0[(96 + ks) * 64 + lane], x, a1);
    }
    const float* b0 = P + kHeadB0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
        a0[r] = relu(a0[r] + b0[o]);
        a1[r] = relu(a1[r] + b0[o + 32]);
    }

    // layer 1: 64 -> 64
    f32x16 c0 = {}, c1 = {};
    Layer<0, 32>::run<2, 32>(P + kHeadW1, lane, h, a0, a1, c0, c1);
    const float* b1 = P + kHeadB1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
        c0[r] = relu(c0[r] + b1[o]);
        c1[r] = relu(c1[r] + b1[o + 32]);
    }

    // layer 2: 64 -> 1 (row 0 of the tile: register 0 of the lanes h = 0), then the sigmoid
    f32x16 d0 = {}, d1 = {};
    Layer<0, 32>::run<1, 32>(P + kHeadW2, lane, h, c0, c1, d0, d1);
    if (tv && h == 0) {
        const float y = d0[0] + P[kHeadB2];
        const size_t o = (size_t)b * T + t;
        prob[o] = 1.f / (1.f + expf(-y));
        if (logit) logit[o] = y;
    }
}

struct HeadSpec {
    const char* name;
    size_t numel;
};
const HeadSpec kHeadParams[6] = {{"fuse_layer.0.weight", (size_t)kHeadHid * kHeadIn}, {"fuse_layer.0.bias", kHeadHid},
                                 {"fuse_layer.2.weight", (size_t)kHeadHid * kHeadHid}, {"fuse_layer.2.bias", kHeadHid},
                                 {"fuse_layer.4.weight", kHeadHid},                     {"fuse_layer.4.bias", 1}};

#define M2S_TRY(expr)                                                                                                 \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return dc_set_error(DC_ERR_HIP, (std::string(#expr) + " failed: " + hipGetErrorString(e_)).c_str()); \
    } while (0)

bool starts_with(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }
bool ends_with(const std::string& s, const std::string& e) { return s.size() >= e.size() && s.compare(s.size() - e.size(), e.size(), e) == 0; }

}  // namespace

struct dc_m2snet {
    int device = 0;
    DcParams music_params, head_params;
    dc_motion_encoder* motion = nullptr;
    dc_music* music = nullptr;
    float* d_head = nullptr;
    float* d_ws = nullptr;               // [chunk][T][64] music latents, then [chunk][64][T] motion latents
    size_t ws_floats = 0;
    bool finalized = false;
};

namespace {

int head_launch(const dc_m2snet* n, const float* mus, const float* mot, int B, int T, float* prob, float* logit, hipStream_t st) {
    const unsigned gx = (unsigned)(((T + 31) / 32 + MH_WAVES - 1) / MH_WAVES);
    for (int b0 = 0; b0 < B; b0 += MH_GRID_Y) {
        const int nb = B - b0 < MH_GRID_Y ? B - b0 : MH_GRID_Y;
        const size_t o = (size_t)b0 * T;
        k_m2s_head<<<dim3(gx, nb), 64 * MH_WAVES, 0, st>>>(mus + o * MH_C, mot + o * MH_C, n->d_head, prob + o, logit ? logit + o : nullptr, T);
    }
    M2S_TRY(hipGetLastError());
    return DC_OK;
}

int music_run(dc_m2snet* n, const float* d_mel, int B, int Tm, float* d_out, hipStream_t st) {
    std::string err;
    const hipError_t e = dc_music_encode(n->music, d_mel, B, Tm, nullptr, d_out, st, &err);
    if (e != hipSuccess) return dc_set_error(DC_ERR_HIP, (std::string("M2SNet music encoder: ") + hipGetErrorString(e) + " " + err).c_str());
    return DC_OK;
}

}  // namespace

extern "C" {

int dc_m2snet_create(int32_t device, dc_m2snet** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_create: out is NULL");
    *out = nullptr;
    dc_motion_encoder* me = nullptr;
    if (const int rc = dc_motion_encoder_create(device, &me)) return rc;      // (checks the device ordinal)
    auto* n = new dc_m2snet;
    n->device = device;
    n->motion = me;
    *out = n;
    return DC_OK;
}

void dc_m2snet_destroy(dc_m2snet* n) {
    if (!n) return;
    hipSetDevice(n->device);
    dc_motion_encoder_destroy(n->motion);
    dc_music_destroy(n->music);
    if (n->d_head) hipFree(n->d_head);
    if (n->d_ws) hipFree(n->d_ws);
    delete n;
}

int dc_m2snet_set_param(dc_m2snet* n, const char* name, const float* h_data, int64_t numel) {
    if (!n || !name || !h_data) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_set_param: NULL argument");
    const std::string k(name);
    const auto wrong = [&](size_t want) {
        return dc_set_error(DC_ERR_PARAM, ("M2SNet parameter " + k + " has " + std::to_string(numel) + " elements, expected " +
                                           std::to_string(want)).c_str());
    };
    if (starts_with(k, "motion_encoder.")) {
        const int rc = dc_motion_encoder_set_param(n->motion, name + 15, h_data, numel);
        if (rc == DC_OK) n->finalized = false;
        return rc;
    }
    if (starts_with(k, "music_encoder.")) {
        for (const auto& r : dc_music_required(MH_C, false))
            if (r.first == k) {
                if ((size_t)numel != r.second) return wrong(r.second);
                n->music_params[k].assign(h_data, h_data + numel);
                n->finalized = false;
                return DC_OK;
            }
        // the BatchNorm counters: state_dict entries eval mode never applies
        const std::string nbt = ".num_batches_tracked";
        if (ends_with(k, nbt)) {
            const std::string rm = k.substr(0, k.size() - nbt.size()) + ".running_mean";
            for (const auto& r : dc_music_required(MH_C, false))
                if (r.first == rm) return numel == 1 ? DC_OK : wrong(1);
        }
    }
    for (const HeadSpec& hs : kHeadParams)
        if (k == hs.name) {
            if ((size_t)numel != hs.numel) return wrong(hs.numel);
            n->head_params[k].assign(h_data, h_data + numel);
            n->finalized = false;
            return DC_OK;
        }
    return dc_set_error(DC_ERR_PARAM, ("unknown M2SNet parameter " + k).c_str());
}

int dc_m2snet_finalize(dc_m2snet* n) {
    if (!n) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_finalize: NULL handle");
    n->finalized = false;
    std::string err;
    if (!dc_music_check(n->music_params, MH_C, &err, false)) return dc_set_error(DC_ERR_PARAM, ("M2SNet music encoder: " + err).c_str());
    for (const HeadSpec& hs : kHeadParams)
        if (!n->head_params.count(hs.name))
            return dc_set_error(DC_ERR_PARAM, (std::string("M2SNet parameter ") + hs.name + " was not set").c_str());
    if (const int rc = dc_motion_encoder_finalize(n->motion)) return rc;
    M2S_TRY(hipSetDevice(n->device));
    if (n->music) {
        M2S_TRY(hipDeviceSynchronize());     // (work of earlier calls may still read the old weights)
        dc_music_destroy(n->music);
        n->music = nullptr;
    }
    n->music = dc_music_build(n->music_params, MH_C, &err, false);
    if (!n->music) return dc_set_error(DC_ERR_PARAM, ("M2SNet music encoder: " + err).c_str());
    dc_music_pin_format(n->music, DC_ME_SPLIT);      // a score has no use for the fp16 planes' 3.7e-4, whatever DC_ME_PREC says
    const std::vector<float> img = m2s_head_pack(n->head_params);
    if (!n->d_head) M2S_TRY(hipMalloc((void**)&n->d_head, img.size() * sizeof(float)));
    M2S_TRY(hipMemcpy(n->d_head, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    n->finalized = true;
    return DC_OK;
}

int dc_m2snet_encode_music(dc_m2snet* n, const float* d_mel, int32_t B, int32_t Tm, float* d_music_latent, void* stream) {
    if (!n || !d_mel || !d_music_latent) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music: NULL argument");
    if (!n->finalized) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music before dc_m2snet_finalize");
    if (B < 1) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music: B must be >= 1");
    if (Tm < 4) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music: need at least 4 mel frames (the encoder's reflection padding)");
    M2S_TRY(hipSetDevice(n->device));
    return music_run(n, d_mel, B, Tm, d_music_latent, (hipStream_t)stream);
}

int dc_m2snet_fuse(dc_m2snet* n, const float* d_music_latent, const float* d_motion_latent, int32_t B, int32_t T, float* d_prob,
                   float* d_logit, void* stream) {
    if (!n || !d_music_latent || !d_motion_latent || !d_prob) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse: NULL argument");
    if (!n->finalized) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse before dc_m2snet_finalize");
    if (B < 1 || T < 1) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse: B and T must be >= 1");
    if ((uintptr_t)d_music_latent & 15) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse: the music latent must be 16-byte aligned");
    M2S_TRY(hipSetDevice(n->device));
    return head_launch(n, d_music_latent, d_motion_latent, B, T, d_prob, d_logit, (hipStream_t)stream);
}

int dc_m2snet_score(dc_m2snet* n, const float* d_mel, const float* d_motion, int32_t B, int32_t Tm, int32_t T, float* d_prob,
                    float* d_logit, void* stream) {
    if (!n || !d_mel || !d_motion || !d_prob) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_score: NULL argument");
    if (!n->finalized) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_score before dc_m2snet_finalize");
    if (B < 1) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_score: B must be >= 1");
    if (Tm < 4) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_score: need at least 4 mel frames (the encoder's reflection padding)");
    if (T != dc_music_frames(Tm))
        return dc_set_error(DC_ERR_INVALID, ("dc_m2snet_score: " + std::to_string(Tm) + " mel frames make " + std::to_string(dc_music_frames(Tm)) +
                                             " latent frames, the motion has " + std::to_string(T)).c_str());
    M2S_TRY(hipSetDevice(n->device));
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < MH_CHUNK ? B : MH_CHUNK;
    const size_t plane = (size_t)chunk * MH_C * T;
    if (n->ws_floats < 2 * plane) {
        if (n->d_ws) {
            M2S_TRY(hipStreamSynchronize(st));    // (the previous call's work on this stream may still read the old planes)
            M2S_TRY(hipFree(n->d_ws));
            n->d_ws = nullptr;
            n->ws_floats = 0;
        }
        M2S_TRY(hipMalloc((void**)&n->d_ws, 2 * plane * sizeof(float)));
        n->ws_floats = 2 * plane;
    }
    float *mus = n->d_ws, *mot = n->d_ws + plane;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        if (const int rc = music_run(n, d_mel + (size_t)b0 * Tm * 128, nb, Tm, mus, st)) return rc;
        if (const int rc = dc_motion_encoder_encode(n->motion, d_motion + (size_t)b0 * T * 26, nb, T, mot, stream)) return rc;
        if (const int rc = head_launch(n, mus, mot, nb, T, d_prob + (size_t)b0 * T, d_logit ? d_logit + (size_t)b0 * T : nullptr, st)) return rc;
    }
    return DC_OK;
}

}  // extern "C"
