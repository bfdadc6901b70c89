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

// ---- every music against every motion ------------------------------------------------------------------------------------------
// Layer 0 of the head is one k-ordered chain per output, k = 0 .. 63 over the music latent and k = 64 .. 127 over the motion latent:
// its state after k = 63 is a function of the music alone.  k_m2s_pairs runs that half once per 32-frame tile of music i and
// continues a COPY of it with one motion after another - the same MFMAs on the same operands in the same order as k_m2s_head from
// there on, so every probability has the bits dc_m2snet_fuse gives that pair.  160 MFMAs per pair tile instead of 224.
constexpr int MP_SHARE = 8;                // motions one wave walks per launch (dc_m2snet_pairs_share): the music half is 64 of 64 + 8 x 160 MFMAs
constexpr int MP_COLS = 512;               // motions per pass
constexpr int MP_ROWS = 1024;              // musics per pass, at most; fewer where MP_PAIR_TILES binds
constexpr size_t MP_PAIR_TILES = 1u << 22; // (pair, tile) partials per pass: 3 x 16 MB of workspace

// kstep_operand of dc_mfma_f32.h - the same value on every lane - with one v_permlane32_swap in place of the exchange through the
// LDS crossbar: registers r0 and r1 of the half HC that owns channels 2 S and 2 S + 1 are swapped across the halves (the upper
// half of the first with the lower half of the second), which leaves channel 2 S on the lanes h = 0 and 2 S + 1 on the lanes h = 1
// of one of the two.  A VALU instruction: the MFMA behind it waits for no LDS counter.  (Two k-steps share a swap: registers
// r0, r1 hold channels 2 S, 2 S + 1 in one half and 2 S + 4, 2 S + 5 in the other.)
template <int S>
DEV float kstep_operand_swap(const f32x16& lo, const f32x16& hi) {
    constexpr int c = (2 * S) & 31, HC = (c >> 2) & 1, r0 = (c & 3) + 4 * (c >> 3), r1 = r0 + 1;
    const f32x16& t = S < 16 ? lo : hi;
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(t[r0]), __float_as_uint(t[r1]), false, false);
    return __uint_as_float(HC ? r[1] : r[0]);
}
// Layer<>::run of dc_mfma_f32.h with the A fragments in registers (w0[s], w1[s]: k-step s of output tile 0 and 1): the same
// operands in the same order
template <int S0, int N>
struct RegLayer {
    template <int NMT>
    static DEV void run(const float (&w0)[32], const float (&w1)[32], const f32x16& lo, const f32x16& hi, f32x16& acc0, f32x16& acc1) {
        const float x = kstep_operand_swap<S0>(lo, hi);
        acc0 = mfma2(w0[S0], x, acc0);
        if (NMT == 2) acc1 = mfma2(w1[S0], x, acc1);
        RegLayer<S0 + 1, N - 1>::template run<NMT>(w0, w1, lo, hi, acc0, acc1);
    }
};
template <int S0>
struct RegLayer<S0, 0> {
    template <int NMT>
    static DEV void run(const float (&)[32], const float (&)[32], const f32x16&, const f32x16&, f32x16&, f32x16&) {}
};

// mus [nbm][T][64], mot [nbn][64][T], len_mus [nbm], len_mot [nbn] (NULL: every length is T) -> per (tile, pair) partials
// [ntiles][nbm * nbn] of the valid frames t < min(len_mus[i], len_mot[c]): the sum of the probabilities (a fixed xor tree over the tile's 32 lanes, an invalid frame
// a literal 0), the counts of p > 0.5 and of p < 0.5.  prob, unless NULL: [.][.][T] with `prob_row` floats between two musics,
// every frame t < T written.  grid (tile groups, nbm, ceil(nbn / MP_SHARE)).
__global__ __launch_bounds__(64 * MH_WAVES) void k_m2s_pairs(const float* __restrict__ mus, const float* __restrict__ mot,
                                                             const float* __restrict__ P, const int* __restrict__ len_mus,
                                                             const int* __restrict__ len_mot, float* __restrict__ part_sum,
                                                             int* __restrict__ part_above, int* __restrict__ part_below,
                                                             float* __restrict__ prob, size_t prob_row, int T, int nbn) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x * MH_WAVES + (threadIdx.x >> 6);
    const int t0 = tile * 32;
    if (t0 >= T) return;                 // wave-uniform; no barriers below
    const int i = blockIdx.y, t = t0 + j;
    const bool tv = t < T;
    const int tc = tv ? t : T - 1;

    // layer 0, k = 0 .. 63: the music latent, once
    f32x4 m[16];
    load_row64(mus + ((size_t)i * T + tc) * MH_C, m);
    const float* w0 = P + kHeadW0;
    f32x16 m0 = {}, m1 = {};
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const float x = row_operand(m, ks, h);
        m0 = mfma2(w0[ks * 64 + lane], x, m0);
        m1 = mfma2(w0[(64 + ks) * 64 + lane], x, m1);
    }
    const int lm = len_mus ? len_mus[i] : T;
    const int c0 = blockIdx.z * MP_SHARE, c1 = c0 + MP_SHARE < nbn ? c0 + MP_SHARE : nbn;
    const size_t np = (size_t)gridDim.y * nbn;
    // The weights the loop reads (W0's motion half, W1, W2: 160 fragments per lane) stay in registers across the motions, and a
    // motion's 32 operands are loaded one motion ahead: the loop body waits for no load of its own.
    float wa[32], wb[32], ua[32], ub[32], u2[32];
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        wa[ks] = w0[(32 + ks) * 64 + lane];
        wb[ks] = w0[(96 + ks) * 64 + lane];
        ua[ks] = P[kHeadW1 + ks * 64 + lane];
        ub[ks] = P[kHeadW1 + (32 + ks) * 64 + lane];
        u2[ks] = P[kHeadW2 + ks * 64 + lane];
    }
    float bz0[32], bz1[32];              // add_bias's operands: register r of tile 0 | 1
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        bz0[r] = P[kHeadB0 + tile_channel(r, h)], bz0[16 + r] = P[kHeadB0 + 32 + tile_channel(r, h)];
        bz1[r] = P[kHeadB1 + tile_channel(r, h)], bz1[16 + r] = P[kHeadB1 + 32 + tile_channel(r, h)];
    }
    const float bz2 = P[kHeadB2];
    const float* src = mot + (size_t)c0 * MH_C * T + tc;
    float x[32];
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) x[ks] = src[(size_t)(2 * ks + h) * T];
#pragma unroll 1
    for (int c = c0; c < c1; ++c) {
        if (c + 1 < c1) src += (size_t)MH_C * T;      // (the last motion is loaded twice: in bounds, unused)
        float nx[32];
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) nx[ks] = src[(size_t)(2 * ks + h) * T];
        const int ln = len_mot ? len_mot[c] : T, n = lm < ln ? lm : ln;
        float v = 0.f;
        int above = 0, below = 0;
        if (prob || t0 < n) {            // wave-uniform: a tile without a valid frame is computed only for its probabilities
            // layer 0, k = 64 .. 127: this motion's latent continues a copy of the music's chain
            f32x16 a0 = m0, a1 = m1;
            f32x16 b0 = {}, b1 = {}, d0 = {}, d1 = {};
#pragma unroll
            for (int ks = 0; ks < 32; ++ks) {
                a0 = mfma2(wa[ks], x[ks], a0);
                a1 = mfma2(wb[ks], x[ks], a1);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) a0[r] = relu(a0[r] + bz0[r]), a1[r] = relu(a1[r] + bz0[16 + r]);
            RegLayer<0, 32>::run<2>(ua, ub, a0, a1, b0, b1);
#pragma unroll
            for (int r = 0; r < 16; ++r) b0[r] = relu(b0[r] + bz1[r]), b1[r] = relu(b1[r] + bz1[16 + r]);
            RegLayer<0, 32>::run<1>(u2, u2, b0, b1, d0, d1);
            const float y = d0[0] + bz2;
            const float p = 1.f / (1.f + expf(-y));
            if (prob && tv && h == 0) prob[(size_t)i * prob_row + (size_t)c * T + t] = p;
            const bool ok = h == 0 && t < n;     // (n <= T)
            v = ok ? p : 0.f;
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) v += __shfl_xor(v, off);
            above = __popcll(__ballot(ok && p > 0.5f));
            below = __popcll(__ballot(ok && p < 0.5f));
        }
        if (lane == 0) {
            const size_t o = (size_t)tile * np + (size_t)i * nbn + c;
            part_sum[o] = v;
            part_above[o] = above;
            part_below[o] = below;
        }
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) x[ks] = nx[ks];
    }
}

// the tiles of a pair in ascending order: one thread per pair of the pass
__global__ __launch_bounds__(256) void k_m2s_pairs_reduce(const float* __restrict__ part_sum, const int* __restrict__ part_above,
                                                          const int* __restrict__ part_below, int ntiles, int np, int nbn, int Bn,
                                                          float* __restrict__ sum, int* __restrict__ above, int* __restrict__ below) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= np) return;
    float s = part_sum[idx];
    int a = part_above[idx], b = part_below[idx];
    for (int k = 1; k < ntiles; ++k) {
        const size_t o = (size_t)k * np + idx;
        s += part_sum[o];
        a += part_above[o];
        b += part_below[o];
    }
    const size_t o = (size_t)(idx / nbn) * Bn + idx % nbn;
    sum[o] = s;
    above[o] = a;
    below[o] = b;
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

int32_t dc_m2snet_pairs_share(void) { return MP_SHARE; }

int dc_m2snet_fuse_pairs(dc_m2snet* n, const float* d_music_latent, const float* d_motion_latent, int32_t Bm, int32_t Bn, int32_t T,
                         const int32_t* h_len_music, const int32_t* h_len_motion, float* d_sum, int32_t* d_above, int32_t* d_below,
                         float* d_prob, void* stream) {
    if (!n || !d_music_latent || !d_motion_latent || !d_sum || !d_above || !d_below)
        return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse_pairs: NULL argument");
    if (!n->finalized) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse_pairs before dc_m2snet_finalize");
    if (Bm < 1 || Bn < 1 || T < 1) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse_pairs: Bm, Bn and T must be >= 1");
    if ((uintptr_t)d_music_latent & 15) return dc_set_error(DC_ERR_INVALID, "dc_m2snet_fuse_pairs: the music latent must be 16-byte aligned");
    std::vector<int32_t> len((size_t)Bm + Bn, T);
    for (int k = 0; k < Bm + Bn; ++k) {
        const int32_t* src = k < Bm ? h_len_music : h_len_motion;
        if (!src) continue;
        len[k] = src[k < Bm ? k : k - Bm];
        if (len[k] < 1 || len[k] > T)
            return dc_set_error(DC_ERR_INVALID, (std::string("dc_m2snet_fuse_pairs: length ") + std::to_string(len[k]) + " of " + (k < Bm ? "music " : "motion ") +
                                                 std::to_string(k < Bm ? k : k - Bm) + " is outside [1, " + std::to_string(T) + "]").c_str());
    }
    DC_HIP_TRY(hipSetDevice(n->device));
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = (T + 31) / 32;
    const int cols = Bn < MP_COLS ? Bn : MP_COLS;
    const size_t fit = MP_PAIR_TILES / ((size_t)ntiles * cols);
    const int rows = (int)(fit < 1 ? 1 : fit > (size_t)(Bm < MP_ROWS ? Bm : MP_ROWS) ? (size_t)(Bm < MP_ROWS ? Bm : MP_ROWS) : fit);
    const size_t plane = (size_t)ntiles * rows * cols, nlen = ((size_t)Bm + Bn + 3) & ~(size_t)3;
    if (const int rc = n->ws.reserve(3 * plane + nlen, st)) return rc;
    float* ps = n->ws.p;
    int *pa = reinterpret_cast<int*>(n->ws.p + plane), *pb = reinterpret_cast<int*>(n->ws.p + 2 * plane);
    int* d_len = reinterpret_cast<int*>(n->ws.p + 3 * plane);
    const bool ragged = h_len_music || h_len_motion;
    if (ragged) {                        // behind the stream's earlier work (which may read the last call's lengths), and out of `len` before it dies
        DC_HIP_TRY(hipMemcpyAsync(d_len, len.data(), len.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
        DC_HIP_TRY(hipStreamSynchronize(st));
    }
    const unsigned gx = (unsigned)((ntiles + MH_WAVES - 1) / MH_WAVES);
    const size_t prob_row = (size_t)Bn * T;
    const int rc = dc_chunks(Bm, rows, [&](int i0, int nbm) -> int {
        return dc_chunks(Bn, cols, [&](int j0, int nbn) -> int {
            const size_t out = (size_t)i0 * Bn + j0;
            k_m2s_pairs<<<dim3(gx, nbm, (nbn + MP_SHARE - 1) / MP_SHARE), 64 * MH_WAVES, 0, st>>>(
                d_music_latent + (size_t)i0 * T * MH_C, d_motion_latent + (size_t)j0 * MH_C * T, n->d_head, ragged ? d_len + i0 : nullptr, ragged ? d_len + Bm + j0 : nullptr, ps, pa, pb,
                d_prob ? d_prob + out * T : nullptr, prob_row, T, nbn);
            const int np = nbm * nbn;
            k_m2s_pairs_reduce<<<(np + 255) / 256, 256, 0, st>>>(ps, pa, pb, ntiles, np, nbn, Bn, d_sum + out, d_above + out, d_below + out);
            return DC_OK;
        });
    });
    DC_HIP_TRY(hipGetLastError());
    return rc;
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
