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

#include "dc_common.h"
#include "dc_handle.h"
#include "dc_mfma_f32.h"

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
    f32x4 m[16];
    load_row64(mus + ((size_t)b * T + tc) * MH_C, m);
    const float* w0 = P + kHeadW0;
    f32x16 a0 = {}, a1 = {};
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const float x = row_operand(m, ks, h);
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
    add_bias<true>(a0, a1, P + kHeadB0, h);

    // layer 1: 64 -> 64
    f32x16 c0 = {}, c1 = {};
    Layer<0, 32>::run<2, 32>(P + kHeadW1, lane, h, a0, a1, c0, c1);
    add_bias<true>(c0, c1, P + kHeadB1, h);

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

const char* const kWhat = "M2SNet";
const DcParamList kHeadParams = {{"fuse_layer.0.weight", (size_t)kHeadHid * kHeadIn}, {"fuse_layer.0.bias", kHeadHid},
                                 {"fuse_layer.2.weight", (size_t)kHeadHid * kHeadHid}, {"fuse_layer.2.bias", kHeadHid},
                                 {"fuse_layer.4.weight", kHeadHid},                     {"fuse_layer.4.bias", 1}};

}  // namespace

struct dc_m2snet {
    int device = 0;
    DcOwnedMusic music;                  // from M2SNet's own `music_encoder.*` entries
    DcParams head_params;
    dc_motion_encoder* motion = nullptr;
    float* d_head = nullptr;
    DcWorkspace ws;                      // [chunk][T][64] music latents, then [chunk][64][T] motion latents
    bool finalized = false;
};

namespace {

int head_launch(const dc_m2snet* n, const float* mus, const float* mot, int B, int T, float* prob, float* logit, hipStream_t st) {
    const unsigned gx = (unsigned)(((T + 31) / 32 + MH_WAVES - 1) / MH_WAVES);
    dc_chunks(B, MH_GRID_Y, [&](int b0, int nb) -> int {
        const size_t o = (size_t)b0 * T;
        k_m2s_head<<<dim3(gx, nb), 64 * MH_WAVES, 0, st>>>(mus + o * MH_C, mot + o * MH_C, n->d_head, prob + o, logit ? logit + o : nullptr, T);
        return DC_OK;
    });
    DC_HIP_TRY(hipGetLastError());
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
    const DcDeviceGuard on(n->device);
    dc_motion_encoder_destroy(n->motion);
    n->music.release();
    if (n->d_head) (void)hipFree(n->d_head);
    n->ws.release();
    delete n;
}

int dc_m2snet_set_param(dc_m2snet* n, const char* name, const float* h_data, int64_t numel) {
    if (!n || !name || !h_data) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_set_param: NULL argument");
    const std::string k(name);
    bool changed = false;
    int rc;
    if (starts_with(k, "motion_encoder.")) {
        rc = dc_motion_encoder_set_param(n->motion, name + 15, h_data, numel);
        changed = rc == DC_OK;
    } else if (starts_with(k, "music_encoder.")) {
        rc = n->music.take(kWhat, MH_C, k, h_data, numel, &changed);
    } else {
        rc = dc_param_take(kWhat, kHeadParams, {}, k, k, h_data, numel, &n->head_params, &changed);
    }
    if (changed) n->finalized = false;
    return rc;
}

int dc_m2snet_finalize(dc_m2snet* n) {
    if (!n) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_finalize: NULL handle");
    n->finalized = false;
    if (const int rc = n->music.check(kWhat, MH_C)) return rc;
    if (const int rc = dc_param_complete(kWhat, kHeadParams, n->head_params)) return rc;
    if (const int rc = dc_motion_encoder_finalize(n->motion)) return rc;
    DC_HIP_TRY(hipSetDevice(n->device));
    if (const int rc = n->music.rebuild(kWhat, MH_C)) return rc;
    const std::vector<float> img = m2s_head_pack(n->head_params);
    if (!n->d_head) DC_HIP_TRY(hipMalloc((void**)&n->d_head, img.size() * sizeof(float)));
    DC_HIP_TRY(hipMemcpy(n->d_head, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    n->finalized = true;
    return DC_OK;
}

int dc_m2snet_encode_music(dc_m2snet* n, const float* d_mel, int32_t B, int32_t Tm, float* d_music_latent, void* stream) {
    if (!n || !d_mel || !d_music_latent) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music: NULL argument");
    if (!n->finalized) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music before dc_m2snet_finalize");
    if (B < 1) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music: B must be >= 1");
    if (Tm < 4) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_encode_music: need at least 4 mel frames (the encoder's reflection padding)");
    DC_HIP_TRY(hipSetDevice(n->device));
    return n->music.encode(kWhat, d_mel, B, Tm, d_music_latent, (hipStream_t)stream);
}

int dc_m2snet_fuse(dc_m2snet* n, const float* d_music_latent, const float* d_motion_latent, int32_t B, int32_t T, float* d_prob,
                   float* d_logit, void* stream) {
    if (!n || !d_music_latent || !d_motion_latent || !d_prob) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse: NULL argument");
    if (!n->finalized) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse before dc_m2snet_finalize");
    if (B < 1 || T < 1) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse: B and T must be >= 1");
    if ((uintptr_t)d_music_latent & 15) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse: the music latent must be 16-byte aligned");
    DC_HIP_TRY(hipSetDevice(n->device));
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
    DC_HIP_TRY(hipSetDevice(n->device));
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < MH_CHUNK ? B : MH_CHUNK;
    const size_t plane = (size_t)chunk * MH_C * T;
    if (const int rc = n->ws.reserve(2 * plane, st)) return rc;
    float *mus = n->ws.p, *mot = n->ws.p + plane;
    return dc_chunks(B, chunk, [&](int b0, int nb) -> int {
        if (const int rc = n->music.encode(kWhat, d_mel + (size_t)b0 * Tm * 128, nb, Tm, mus, st)) return rc;
        if (const int rc = dc_motion_encoder_encode(n->motion, d_motion + (size_t)b0 * T * 26, nb, T, mot, stream)) return rc;
        return head_launch(n, mus, mot, nb, T, d_prob + (size_t)b0 * T, d_logit ? d_logit + (size_t)b0 * T : nullptr, st);
    });
}

}  // extern "C"
