// dc_rhythm.hip - the scores of the M2S-GAN evaluation that look at HOW the motion moves, on gfx950 (MI355X): the Welch power
// spectrum behind the rhythm density error, the speed contour behind the strength contour error, the per-channel standard
// deviation, and the M2S-GAN critic behind the W-distance.
//
// Reference (restated, not translated):
//   rhythm_density_error   Contrastive_Stage/utils/loss.py:154-190: scipy.signal.welch(x, 30) of each of the 26 pose channels, summed,
//                          / 26, compared in bins 6 .. 25.  (The signal.spectrogram calls at :168-171 fill arrays nobody reads.)
//   strengh_contour_error  loss.py:128-151: |mean over the channels of x[t-1] - x[t]| (0 at frame 0), AvgPool1d(60, 30).
//   SD                     Contrastive_Stage/M2SGAN_eval.py:101-102: mean over the channels of torch.std(motion, dim=1).
//   Discriminator_1DCNN    Contrastive_Stage/models/Discriminator.py:5-41, scored as D(real) - D(fake) at M2SGAN_eval.py:107-109.
//
// Kernels (all arithmetic fp32; every output a fixed-order sum, no atomics: bit-identical on a rerun and in any batch):
//   k_psd_cols     one wave = 32 (segment, channel) columns of ONE clip on the lanes (lane l: column l & 31, k half l >> 5).  Each
//                  column's mean is removed first (constant detrend, BEFORE the window), then the 64 x 256 window-and-twiddle table
//                  (dc_pack.h, welch_table: window, density scale and one-sided doubling folded in) is applied as 128 k-steps of
//                  v_mfma_f32_32x32x2_f32 into two accumulator tiles - cos rows and sin rows, so re^2 + im^2 of a bin is
//                  register-local -, and a xor butterfly over the 32 columns leaves one partial per wave and bin.
//   k_psd_finish   sums a clip's wave partials in wave order, / (segments x 26).
//   k_contour      one workgroup = 7 windows of one clip: the 240 frames' speeds into LDS, then each window's 60 in frame order.
//   k_sd           one workgroup per clip, 26 channels x 32 time lanes; two passes (mean first) on x - x[0], so a constant is exact.
//   k_disc_conv    one stage of the critic: Conv1d(k = 5, zero padding 2) as a k-ordered chain, K = 5 CIN tap-major, one wave = 32
//                  conv frames of one clip x 64 channels, + bias, ReLU, and MaxPool1d(5, stride S) in the epilogue: lane S q takes the
//                  maximum of lanes S q .. S q + 4 (nanmax: a NaN frame in the window wins, as in torch's max_pool1d) and writes pooled
//                  frame p0 + q; a wave advances by (27 / S + 1) pooled frames.
//   k_disc_head    fc 64 -> 32 -> 32 -> 1 per pooled frame, chained in registers (as k_gan_head); k_disc_mean: mean over the frames.
//
// Beat consistency (BC) and Beat Align from supplied music beats:
//   motion_peak_onehot     Diffusion_Stage/tools/eval_new_metrics.py:285-309 = Contrastive_Stage/M2SGAN_eval.py:310-332: the summed joint
//                          speed and scipy.signal.argrelextrema(envelope, np.less, order=10) - strict minima over +-10 frames.
//   alignment_score        eval_new_metrics.py:253-275 = M2SGAN_eval.py:345-367: per music beat a Gaussian of the distance to the nearest
//                          motion beat.  (get_music_beat, librosa's tracker, is a function of the mel alone: its one-hot is an input.)
//   k_beat_motion  one workgroup per clip: the envelope with numpy's float32 bits (envelope_frame), a barrier, the strict minima.
//   k_beat_scores  one workgroup per clip: both one-hots compacted into sorted index lists (wave ballots, a running prefix), a binary
//                  search per beat, expf, fixed-order sums.
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

constexpr int R_WAVES = 4;                 // waves per workgroup of the MFMA kernels
constexpr int R_CHUNK = 64;                // clips per pass of the rhythm kernels (bounds the partials and the grid)
constexpr int D_CHUNK = 32;                // clips per pass of the critic (bounds the three pooled planes)
constexpr int R_POSE = 26;                 // pose channels
constexpr int C_WIN = 60, C_HOP = 30;      // AvgPool1d(kernel_size=60, stride=30) of the strength contour
constexpr int C_WPB = 7;                   // windows per workgroup: 30 * 6 + 60 = 240 frames
constexpr int SD_LANES = 32;               // time lanes per channel of k_sd
constexpr int B_THREADS = 256;             // threads of the beat kernels' one workgroup per clip
constexpr int B_MAX_ORDER = 64;            // largest `order` of dc_rhythm_motion_beats

// x [clips][T][26] -> part [clips][nw][32]: per wave and bin, the sum over the wave's columns of the column's periodogram
__global__ __launch_bounds__(64 * R_WAVES) void k_psd_cols(const float* __restrict__ x, const float2* __restrict__ tab, float* __restrict__ part,
                                                          int T, int ncols, int nw) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int wave = blockIdx.x * R_WAVES + (threadIdx.x >> 6);
    if (wave >= nw) return;              // wave-uniform; no barriers below
    const int col = wave * 32 + j;
    const bool valid = col < ncols;
    const int cc = valid ? col : ncols - 1;      // (columns past the clip's compute on its last one and add 0)
    const int seg = cc / R_POSE, ch = cc - seg * R_POSE;
    const float* src = x + ((size_t)blockIdx.y * T + (size_t)seg * kWelchHop) * R_POSE + ch;      // sample n at src[26 n]
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < kWelchSeg / 2; ++i) s += src[(2 * i + h) * R_POSE];
    const float mean = (s + __shfl_xor(s, 32)) * (1.f / kWelchSeg);
    f32x16 re = {}, im = {};
    const float2* t2 = tab + lane;
#pragma unroll 8
    for (int ks = 0; ks < kWelchSeg / 2; ++ks) {
        const float v = src[(2 * ks + h) * R_POSE] - mean;
        const float2 ww = t2[ks * 64];
        re = mfma2(ww.x, v, re);
        im = mfma2(ww.y, v, im);
    }
    float* dst = part + ((size_t)blockIdx.y * nw + wave) * kWelchBins;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float p = valid ? fmaf(im[r], im[r], re[r] * re[r]) : 0.f;
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) p += __shfl_xor(p, m);      // both partners add the same pair: one order for all lanes
        if (j == 0) dst[tile_channel(r, h)] = p;
    }
}

__global__ __launch_bounds__(32) void k_psd_finish(const float* __restrict__ part, float* __restrict__ psd, int nw, float count) {
    const float* p = part + (size_t)blockIdx.x * nw * kWelchBins + threadIdx.x;
    float s = 0.f;
    for (int w = 0; w < nw; ++w) s += p[(size_t)w * kWelchBins];
    psd[(size_t)blockIdx.x * kWelchBins + threadIdx.x] = s / count;
}

// x [clips][T][26] -> contour [clips][W]
__global__ __launch_bounds__(256) void k_contour(const float* __restrict__ x, float* __restrict__ contour, int T, int W) {
    __shared__ float speed[256];
    const int w0 = blockIdx.x * C_WPB, t = w0 * C_HOP + (int)threadIdx.x;
    const float* xb = x + (size_t)blockIdx.y * T * R_POSE;
    float v = 0.f;
    if (t >= 1 && t < T) {
        const float *a = xb + (size_t)(t - 1) * R_POSE, *b = a + R_POSE;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < R_POSE; ++c) s += a[c] - b[c];
        v = fabsf(s / (float)R_POSE);
    }
    speed[threadIdx.x] = v;
    __syncthreads();
    const int w = w0 + (int)threadIdx.x;
    if (threadIdx.x < C_WPB && w < W) {
        float s = 0.f;
        for (int i = 0; i < C_WIN; ++i) s += speed[threadIdx.x * C_HOP + i];
        contour[(size_t)blockIdx.y * W + w] = s / (float)C_WIN;
    }
}

// x [clips][T][26] -> sd [clips]: the mean over the channels of the unbiased standard deviation over time
__global__ __launch_bounds__(R_POSE * SD_LANES) void k_sd(const float* __restrict__ x, float* __restrict__ sd, int T) {
    __shared__ float part[SD_LANES][R_POSE];
    __shared__ float stat[R_POSE];
    const int q = threadIdx.x / R_POSE, c = threadIdx.x - q * R_POSE;
    const float* xb = x + (size_t)blockIdx.x * T * R_POSE;
    const float pivot = xb[c];           // the channel's first frame: a constant channel is 0 from here on, exactly
    float s = 0.f;
    for (int t = q; t < T; t += SD_LANES) s += xb[(size_t)t * R_POSE + c] - pivot;
    part[q][c] = s;
    __syncthreads();
    if (q == 0) {
        float m = 0.f;
        for (int i = 0; i < SD_LANES; ++i) m += part[i][c];
        stat[c] = m / (float)T;
    }
    __syncthreads();
    const float mean = stat[c];
    s = 0.f;
    for (int t = q; t < T; t += SD_LANES) {
        const float d = (xb[(size_t)t * R_POSE + c] - pivot) - mean;
        s = fmaf(d, d, s);
    }
    __syncthreads();                     // (stat and part are rewritten below)
    part[q][c] = s;
    __syncthreads();
    if (q == 0) {
        float m = 0.f;
        for (int i = 0; i < SD_LANES; ++i) m += part[i][c];
        stat[c] = sqrtf(m / (float)(T - 1));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float m = 0.f;
        for (int i = 0; i < R_POSE; ++i) m += stat[i];
        sd[blockIdx.x] = m / (float)R_POSE;
    }
}

// ---- beat consistency: the motion's beats and their alignment with supplied music beats ---------------------------------------------
struct BeatLengths {
    int len[R_CHUNK];                    // frames of each clip of a pass
};

// The summed joint speed of one frame with numpy's float32 bits: prev, cur = the 13 (x, y) pairs of frames t - 1 and t.  Every
// operation is rounded on its own (the pragma: hipcc's default would fuse dx dx into the addition), sqrtf is correctly rounded
// (hipcc's default for fp32), and the 13 norms are added in the order of numpy's pairwise reduction over 13 contiguous float32.
DEV float envelope_frame(const float2* __restrict__ prev, const float2* __restrict__ cur) {
#pragma clang fp contract(off)
    float n[R_POSE / 2];
#pragma unroll
    for (int j = 0; j < R_POSE / 2; ++j) {
        const float2 a = prev[j], b = cur[j];
        const float dx = b.x - a.x, dy = b.y - a.y;
        n[j] = sqrtf(dx * dx + dy * dy);
    }
    float s = ((n[0] + n[1]) + (n[2] + n[3])) + ((n[4] + n[5]) + (n[6] + n[7]));
#pragma unroll
    for (int j = 8; j < R_POSE / 2; ++j) s += n[j];
    return s;
}

// x [clips][T][26] -> env [clips][T], beats [clips][T]; one workgroup per clip.  The envelope goes through global memory (the
// caller's array or the workspace), so T is not bounded by LDS; the barrier between the two passes orders this workgroup's stores
// before its own loads.
__global__ __launch_bounds__(B_THREADS) void k_beat_motion(const float* __restrict__ x, float* env, uint8_t* __restrict__ beats, int T, int order,
                                                          BeatLengths bl) {
    const int L = bl.len[blockIdx.x];
    const float* xb = x + (size_t)blockIdx.x * T * R_POSE;
    float* e = env + (size_t)blockIdx.x * T;
    uint8_t* o = beats + (size_t)blockIdx.x * T;
    for (int t = threadIdx.x; t < T; t += B_THREADS) {
        float v = 0.f;
        if (t >= 1 && t < L)
            v = envelope_frame(reinterpret_cast<const float2*>(xb + (size_t)(t - 1) * R_POSE), reinterpret_cast<const float2*>(xb + (size_t)t * R_POSE));
        e[t] = v;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += B_THREADS) {
        bool beat = t < L;
        if (beat) {
            const float v = e[t];
            for (int s = 1; s <= order && beat; ++s) {      // argrelextrema's mode='clip': the index is clamped to the clip
                const int lo = t - s < 0 ? 0 : t - s, hi = t + s > L - 1 ? L - 1 : t + s;
                beat = v < e[lo] && v < e[hi];
            }
        }
        o[t] = beat ? 1 : 0;
    }
}

// idx[0 .. n): the positions of the nonzero bytes of v[0 .. N) in increasing order, n returned to every thread.  Tiles of B_THREADS
// positions: a ballot per wave, the waves' counts through `cnt` (LDS, one int per wave), a running base.  Ends with a barrier.
DEV int compact_beats(const uint8_t* __restrict__ v, int N, int* idx, int* cnt) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = 0; i0 < N; i0 += B_THREADS) {      // (the trip count is the same for every thread: barriers inside)
        const int i = i0 + (int)threadIdx.x;
        const bool on = i < N && v[i] != 0;
        const unsigned long long m = __ballot(on);
        if (lane == 0) cnt[w] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < B_THREADS / 64; ++k) {
            const int c = cnt[k];
            before += k < w ? c : 0;
            total += c;
        }
        if (on) idx[base + before + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += total;
        __syncthreads();                 // (cnt is rewritten by the next tile; the last one orders idx before its readers)
    }
    return base;
}

// exp(-d^2 / (2 sigma^2)) of the distance from position q to the nearest of the n >= 1 sorted positions scale * list[j], all in music
// frames (integers); d = (float)distance / (float)music_stride is the only rounding in front of the square.
DEV float beat_term(long long q, const int* list, int n, long long scale, float stride, float two_sigma2) {
    int lo = 0, hi = n;                  // -> the first j with scale * list[j] >= q
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (scale * list[mid] < q) lo = mid + 1;
        else hi = mid;
    }
    long long best = lo < n ? scale * list[lo] - q : q - scale * list[n - 1];
    if (lo > 0) {
        const long long below = q - scale * list[lo - 1];
        best = below < best ? below : best;
    }
    const float d = (float)best / stride;
    return expf(-(d * d) / two_sigma2);
}

// The sum of every thread's v in a fixed order: partial j + partial j + 128, then + 64, ... + 1 (a binary tree over the thread index).
DEV float block_sum(float v, float* buf) {
    buf[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = B_THREADS / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) buf[threadIdx.x] += buf[threadIdx.x + off];
        __syncthreads();
    }
    const float s = buf[0];
    __syncthreads();                     // (buf is reused by the next sum)
    return s;
}

// mot [clips][T], mus [clips][Lm] one-hots -> scores [clips][2] (BC, Beat Align), counts [clips][2] (music, motion); one workgroup
// per clip, lists [clips][T + Lm] ints in the workspace.
// Order of the sums (it depends on the positions alone, so on (Lm, T) at most): thread j of 256 adds the terms of the positions
// j, j + 256, j + 512, ... in increasing order - a position without a beat adds nothing -, then block_sum's tree over the 256
// partial sums.  Zeros behind a clip's last music beat therefore change nothing, bit for bit.
__global__ __launch_bounds__(B_THREADS) void k_beat_scores(const uint8_t* __restrict__ mot, const uint8_t* __restrict__ mus, int* lists, int T, int Lm,
                                                          int stride, float two_sigma2, float* __restrict__ scores, int* __restrict__ counts) {
    __shared__ int cnt[B_THREADS / 64];
    __shared__ float buf[B_THREADS];
    const uint8_t* mo = mot + (size_t)blockIdx.x * T;
    const uint8_t* mu = mus + (size_t)blockIdx.x * Lm;
    int* mot_idx = lists + (size_t)blockIdx.x * ((size_t)T + Lm);
    int* mus_idx = mot_idx + T;
    const int n_mot = compact_beats(mo, T, mot_idx, cnt);
    const int n_mus = compact_beats(mu, Lm, mus_idx, cnt);
    const float fs = (float)stride;
    float bc = 0.f, ba = 0.f;
    if (n_mot > 0 && n_mus > 0) {        // (block-uniform)
        for (int i = threadIdx.x; i < Lm; i += B_THREADS)
            if (mu[i]) bc += beat_term(i, mot_idx, n_mot, stride, fs, two_sigma2);
        for (int t = threadIdx.x; t < T; t += B_THREADS)
            if (mo[t]) ba += beat_term((long long)stride * t, mus_idx, n_mus, 1, fs, two_sigma2);
    }
    bc = block_sum(bc, buf);
    ba = block_sum(ba, buf);
    if (threadIdx.x == 0) {
        scores[2 * blockIdx.x] = n_mot == 0 ? 0.f : bc / (float)n_mus;            // 0 / 0 = NaN without music beats, as the reference
        scores[2 * blockIdx.x + 1] = n_mus == 0 ? 0.f : ba / (float)n_mot;
        if (counts) {
            counts[2 * blockIdx.x] = n_mus;
            counts[2 * blockIdx.x + 1] = n_mot;
        }
    }
}

// One stage of the critic.  x [clips][Lin][CIN] -> out [clips][Lout][64], Lout = (Lin - 5) / S + 1:
// out[p][o] = max over i < 5 of relu(b[o] + sum over (tap, ci) of W[o][tap CIN + ci] x[S p + i + tap - 2][ci]), x = 0 outside the clip.
template <int CIN, int S>
__global__ __launch_bounds__(64 * R_WAVES) void k_disc_conv(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                           float* __restrict__ out, int Lin, int Lout) {
    constexpr int NP = (32 - kDiscTaps) / S + 1, KS = CIN / 2;
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int p0 = (blockIdx.x * R_WAVES + (threadIdx.x >> 6)) * NP;      // first pooled frame this wave writes
    if (p0 >= Lout) return;              // wave-uniform; no barriers below
    const int t = p0 * S + j;            // this lane's conv frame (past the clip for lanes that feed no pooled frame)
    const float* xb = x + (size_t)blockIdx.y * Lin * CIN;
    const float2* w2 = reinterpret_cast<const float2*>(W) + lane;
    f32x16 a0 = {}, a1 = {};
#pragma unroll 1
    for (int tap = 0; tap < kDiscTaps; ++tap) {
        const int f = t + tap - 2;
        const bool ok = f >= 0 && f < Lin;       // Conv1d's zero padding
        const float* row = xb + (size_t)(f < 0 ? 0 : (f < Lin ? f : Lin - 1)) * CIN;
        const float2* wq = w2 + (size_t)tap * KS * 64;
        if constexpr (CIN == 64) {
            f32x4 m[16];
            load_row64(row, m);
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const float v = ok ? row_operand(m, ks, h) : 0.f;
                const float2 ww = wq[ks * 64];
                a0 = mfma2(ww.x, v, a0);
                a1 = mfma2(ww.y, v, a1);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const float v = ok ? row[2 * ks + h] : 0.f;
                const float2 ww = wq[ks * 64];
                a0 = mfma2(ww.x, v, a0);
                a1 = mfma2(ww.y, v, a1);
            }
        }
    }
    // accumulator register r of lane (j, h) = channel (r & 3) + 8 (r >> 2) + 4 h (+ 32 in the second tile): float4 groups of a row
    const int q = j / S, p = p0 + q;
    const bool keep = q * S == j && q < NP && p < Lout;
    float* dst = out + ((size_t)blockIdx.y * Lout + (keep ? p : 0)) * 64 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 y0, y1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = tile_channel(4 * g + e, h);
            const float v0 = relu(a0[4 * g + e] + bias[c]), v1 = relu(a1[4 * g + e] + bias[c + 32]);
            float m0 = v0, m1 = v1;
#pragma unroll
            for (int i = 1; i < kDiscTaps; ++i) {      // MaxPool1d(5): conv frames t .. t + 4 sit on lanes l .. l + 4
                m0 = nanmax(m0, __shfl_down(v0, i));      // (fmaxf would return the finite operand: torch's pool keeps a NaN)
                m1 = nanmax(m1, __shfl_down(v1, i));
            }
            y0[e] = m0;
            y1[e] = m1;
        }
        if (keep) {
            *reinterpret_cast<f32x4*>(dst + 8 * g) = y0;
            *reinterpret_cast<f32x4*>(dst + 8 * g + 32) = y1;
        }
    }
}

// feat [clips][L][64] -> score [clips][L]: fc.0 + ReLU, fc.2 + ReLU, fc.4.  P: the critic's image.  Frames >= L of a partial tile
// compute on frame L - 1 and are not written.
struct DiscHead {
    unsigned w[3], b[3];
};
DEV void bias_relu32(f32x16& a, const float* b, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = relu(a[r] + b[tile_channel(r, h)]);
}
__global__ __launch_bounds__(64 * R_WAVES) void k_disc_head(const float* __restrict__ feat, const float* __restrict__ P, DiscHead hd,
                                                           float* __restrict__ score, int L) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int t0 = (blockIdx.x * R_WAVES + (threadIdx.x >> 6)) * 32;
    if (t0 >= L) return;                 // wave-uniform; no barriers below
    const int t = t0 + j;
    const bool inside = t < L;
    const size_t frame = (size_t)blockIdx.y * L + (inside ? t : L - 1);
    f32x4 m[16];
    load_row64(feat + frame * 64, m);
    const float* w0 = P + hd.w[0];
    f32x16 a = {}, none = {}, unused = {};
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) a = mfma2(w0[ks * 64 + lane], row_operand(m, ks, h), a);
    bias_relu32(a, P + hd.b[0], h);
    f32x16 c = {};
    Layer<0, 16>::run<1, 16>(P + hd.w[1], lane, h, a, none, c, unused);
    bias_relu32(c, P + hd.b[1], h);
    f32x16 e = {};
    Layer<0, 16>::run<1, 16>(P + hd.w[2], lane, h, c, none, e, unused);      // one row: register 0 of the lower half
    if (inside && h == 0) score[frame] = e[0] + P[hd.b[2]];
}

__global__ __launch_bounds__(64) void k_disc_mean(const float* __restrict__ score, float* __restrict__ out, int nb, int L) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= nb) return;
    float s = 0.f;
    for (int t = 0; t < L; ++t) s += score[(size_t)b * L + t];
    out[b] = s / (float)L;
}

// feat [clips][L][64] -> out [clips][64][L] (Discriminator_1DCNN.features is channel-first)
__global__ __launch_bounds__(256) void k_disc_transpose(const float* __restrict__ feat, float* __restrict__ out, int L) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 64 * L) return;
    const int c = e / L, t = e - c * L;
    out[(size_t)blockIdx.y * 64 * L + e] = feat[((size_t)blockIdx.y * L + t) * 64 + c];
}

const char* const kWhat = "M2S-GAN critic";

}  // namespace

struct dc_rhythm {
    int device = 0;
    float* d_tab = nullptr;              // welch_table as gan_pack_frags2 fragments: [128 ks][64 lanes] (cos, sin)
    DcWorkspace ws;
};

struct dc_discriminator {
    int device = 0;
    DcParams params;
    DiscImage image;                     // offsets (the floats themselves are dropped after the upload)
    float* d_img = nullptr;
    DcWorkspace ws;
    bool finalized = false;
};

namespace {

// The one place where the critic's lengths, workgroup counts and plane offsets come from (B, T).
struct DiscPlan {
    int chunk, L[kDiscStages + 1];       // clips per pass; frames in front of stage i (L[0] = T) and behind the last
    size_t plane[kDiscStages], score;    // float offsets of the three pooled planes and of the per-frame scores
    size_t floats;
    DiscPlan(int B, int T) {
        chunk = B < D_CHUNK ? B : D_CHUNK;
        L[0] = T;
        size_t at = 0;
        for (int i = 0; i < kDiscStages; ++i) {
            L[i + 1] = disc_pooled(L[i], kDiscStride[i]);
            plane[i] = at;
            at += (size_t)chunk * L[i + 1] * 64;
        }
        score = at;
        floats = at + (((size_t)chunk * L[kDiscStages] + 63) & ~(size_t)63);
    }
    static unsigned groups(int Lout, int stride) {
        const int np = (32 - kDiscTaps) / stride + 1;
        return (unsigned)(((Lout + np - 1) / np + R_WAVES - 1) / R_WAVES);
    }
};

// motion [nb][T][26] -> the third stage's pooled plane [nb][L3][64] in the workspace
int stages_run(dc_discriminator* d, const DiscPlan& pl, const float* motion, int nb, hipStream_t st) {
    const float* P = d->d_img;
    const DiscImage& I = d->image;
    float* y[kDiscStages] = {d->ws.p + pl.plane[0], d->ws.p + pl.plane[1], d->ws.p + pl.plane[2]};
    k_disc_conv<kDiscIn, 3><<<dim3(DiscPlan::groups(pl.L[1], 3), nb), 64 * R_WAVES, 0, st>>>(motion, P + I.w[0], P + I.b[0], y[0], pl.L[0], pl.L[1]);
    k_disc_conv<kDiscC, 2><<<dim3(DiscPlan::groups(pl.L[2], 2), nb), 64 * R_WAVES, 0, st>>>(y[0], P + I.w[1], P + I.b[1], y[1], pl.L[1], pl.L[2]);
    k_disc_conv<kDiscC, 2><<<dim3(DiscPlan::groups(pl.L[3], 2), nb), 64 * R_WAVES, 0, st>>>(y[1], P + I.w[2], P + I.b[2], y[2], pl.L[2], pl.L[3]);
    DC_HIP_TRY(hipGetLastError());
    return DC_OK;
}

int disc_check(const char* fn, const dc_discriminator* d, int B, int T) {
    const std::string f(fn);
    if (!d->finalized) return dc_set_error(DC_ERR_INVALID, (f + " before dc_discriminator_finalize").c_str());
    if (B < 1) return dc_set_error(DC_ERR_INVALID, (f + ": B must be >= 1").c_str());
    if (T < kDiscMinT)
        return dc_set_error(DC_ERR_INVALID, (f + ": " + std::to_string(T) + " frames leave no pooled frame behind the third stage (T >= 41)").c_str());
    return DC_OK;
}

int rhythm_check(const char* fn, int B, int T, int min_T, const char* why) {
    const std::string f(fn);
    if (B < 1) return dc_set_error(DC_ERR_INVALID, (f + ": B must be >= 1").c_str());
    if (T < min_T) return dc_set_error(DC_ERR_INVALID, (f + ": " + std::to_string(T) + " frames; " + why).c_str());
    return DC_OK;
}

}  // namespace

extern "C" {

int dc_rhythm_create(int32_t device, dc_rhythm** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_create: out is NULL");
    *out = nullptr;
    if (const int rc = dc_check_device("dc_rhythm_create", device)) return rc;
    const std::vector<float> tab = welch_table();
    std::vector<float> frags(tab.size());
    gan_pack_frags2(tab.data(), kWelchSeg, frags.data());
    const DcDeviceGuard on(device);
    float* d_tab = nullptr;
    DC_HIP_TRY(hipMalloc((void**)&d_tab, frags.size() * sizeof(float)));
    const hipError_t e = hipMemcpy(d_tab, frags.data(), frags.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d_tab);
        return dc_set_error(DC_ERR_HIP, (std::string("dc_rhythm_create: ") + hipGetErrorString(e)).c_str());
    }
    auto* h = new dc_rhythm;
    h->device = device;
    h->d_tab = d_tab;
    *out = h;
    return DC_OK;
}

void dc_rhythm_destroy(dc_rhythm* h) {
    if (!h) return;
    const DcDeviceGuard on(h->device);
    if (h->d_tab) (void)hipFree(h->d_tab);
    h->ws.release();
    delete h;
}

int dc_rhythm_psd(dc_rhythm* h, const float* d_motion, int32_t B, int32_t T, float* d_psd, void* stream) {
    if (!h || !d_motion || !d_psd) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_psd: NULL argument");
    if (const int rc = rhythm_check("dc_rhythm_psd", B, T, kWelchSeg, "Welch's 256-frame segment needs T >= 256 (scipy would shorten the window)"))
        return rc;
    DC_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int nseg = (T - kWelchHop) / kWelchHop, ncols = nseg * R_POSE, nw = (ncols + 31) / 32;
    const int chunk = B < R_CHUNK ? B : R_CHUNK;
    if (const int rc = h->ws.reserve((size_t)chunk * nw * kWelchBins, st)) return rc;
    return dc_chunks(B, chunk, [&](int b0, int nb) -> int {
        k_psd_cols<<<dim3((unsigned)((nw + R_WAVES - 1) / R_WAVES), nb), 64 * R_WAVES, 0, st>>>(
            d_motion + (size_t)b0 * T * R_POSE, reinterpret_cast<const float2*>(h->d_tab), h->ws.p, T, ncols, nw);
        k_psd_finish<<<nb, kWelchBins, 0, st>>>(h->ws.p, d_psd + (size_t)b0 * kWelchBins, nw, (float)ncols);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

int dc_rhythm_contour(dc_rhythm* h, const float* d_motion, int32_t B, int32_t T, float* d_contour, float* d_sd, void* stream) {
    if (!h || !d_motion) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_contour: NULL argument");
    if (const int rc = rhythm_check("dc_rhythm_contour", B, T, C_WIN, "the contour's 60-frame window needs T >= 60")) return rc;
    DC_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int W = (T - C_WIN) / C_HOP + 1;
    return dc_chunks(B, R_CHUNK, [&](int b0, int nb) -> int {
        const float* x = d_motion + (size_t)b0 * T * R_POSE;
        if (d_contour) k_contour<<<dim3((unsigned)((W + C_WPB - 1) / C_WPB), nb), 256, 0, st>>>(x, d_contour + (size_t)b0 * W, T, W);
        if (d_sd) k_sd<<<nb, R_POSE * SD_LANES, 0, st>>>(x, d_sd + b0, T);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

int dc_rhythm_motion_beats(dc_rhythm* h, const float* d_motion, const int32_t* h_length, int32_t B, int32_t T, int32_t order, float* d_envelope,
                           uint8_t* d_beats, void* stream) {
    if (!h || !d_motion || !d_beats) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_motion_beats: NULL argument");
    if (const int rc = rhythm_check("dc_rhythm_motion_beats", B, T, 1, "T must be >= 1")) return rc;
    if (order < 1 || order > B_MAX_ORDER)
        return dc_set_error(DC_ERR_INVALID, ("dc_rhythm_motion_beats: order " + std::to_string(order) + " is outside 1 .. 64").c_str());
    if (h_length)
        for (int32_t b = 0; b < B; ++b)
            if (h_length[b] < 1 || h_length[b] > T)
                return dc_set_error(DC_ERR_INVALID, ("dc_rhythm_motion_beats: length " + std::to_string(h_length[b]) + " of clip " + std::to_string(b) +
                                                     " is outside [1, " + std::to_string(T) + "]").c_str());
    if (reinterpret_cast<uintptr_t>(d_motion) % 8) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_motion_beats: the motion must be 8-byte aligned");
    DC_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < R_CHUNK ? B : R_CHUNK;
    if (!d_envelope)
        if (const int rc = h->ws.reserve((size_t)chunk * T, st)) return rc;
    return dc_chunks(B, chunk, [&](int b0, int nb) -> int {
        BeatLengths bl;
        for (int i = 0; i < R_CHUNK; ++i) bl.len[i] = i < nb ? (h_length ? h_length[b0 + i] : T) : 0;
        float* env = d_envelope ? d_envelope + (size_t)b0 * T : h->ws.p;
        k_beat_motion<<<nb, B_THREADS, 0, st>>>(d_motion + (size_t)b0 * T * R_POSE, env, d_beats + (size_t)b0 * T, T, order, bl);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

int dc_rhythm_beat_scores(dc_rhythm* h, const uint8_t* d_motion_beats, int32_t B, int32_t T, const uint8_t* d_music_beats, int32_t Lm,
                          int32_t music_stride, float sigma, float* d_scores, int32_t* d_counts, void* stream) {
    if (!h || !d_motion_beats || !d_music_beats || !d_scores) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_beat_scores: NULL argument");
    if (const int rc = rhythm_check("dc_rhythm_beat_scores", B, T, 1, "T must be >= 1")) return rc;
    if (Lm < 1) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_beat_scores: Lm must be >= 1");
    if (music_stride < 1) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_beat_scores: music_stride must be >= 1");
    if (!std::isfinite(sigma) || !(sigma > 0.f)) return dc_set_error(DC_ERR_INVALID, "dc_rhythm_beat_scores: sigma must be finite and > 0");
    DC_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < R_CHUNK ? B : R_CHUNK;
    const size_t per_clip = (size_t)T + (size_t)Lm;      // the two index lists (int32, in the float workspace)
    if (const int rc = h->ws.reserve((size_t)chunk * per_clip, st)) return rc;
    const float two_sigma2 = 2.f * sigma * sigma;
    return dc_chunks(B, chunk, [&](int b0, int nb) -> int {
        k_beat_scores<<<nb, B_THREADS, 0, st>>>(d_motion_beats + (size_t)b0 * T, d_music_beats + (size_t)b0 * Lm, reinterpret_cast<int*>(h->ws.p), T, Lm,
                                               music_stride, two_sigma2, d_scores + (size_t)b0 * 2, d_counts ? d_counts + (size_t)b0 * 2 : nullptr);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

int dc_discriminator_create(int32_t device, dc_discriminator** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_discriminator_create: out is NULL");
    *out = nullptr;
    if (const int rc = dc_check_device("dc_discriminator_create", device)) return rc;
    auto* d = new dc_discriminator;
    d->device = device;
    *out = d;
    return DC_OK;
}

void dc_discriminator_destroy(dc_discriminator* d) {
    if (!d) return;
    const DcDeviceGuard on(d->device);
    if (d->d_img) (void)hipFree(d->d_img);
    d->ws.release();
    delete d;
}

int dc_discriminator_set_param(dc_discriminator* d, const char* name, const float* h_data, int64_t numel) {
    if (!d || !name || !h_data) return dc_set_error(DC_ERR_INVALID, "dc_discriminator_set_param: NULL argument");
    const std::string k(name);
    bool changed = false;
    const int rc = dc_param_take(kWhat, disc_required(), {}, k, k, h_data, numel, &d->params, &changed);
    if (changed) d->finalized = false;
    return rc;
}

int dc_discriminator_finalize(dc_discriminator* d) {
    if (!d) return dc_set_error(DC_ERR_INVALID, "dc_discriminator_finalize: NULL handle");
    d->finalized = false;
    if (const int rc = dc_param_complete(kWhat, disc_required(), d->params)) return rc;
    DC_HIP_TRY(hipSetDevice(d->device));
    d->image = disc_pack(d->params);
    const size_t bytes = d->image.img.size() * sizeof(float);
    if (!d->d_img) DC_HIP_TRY(hipMalloc((void**)&d->d_img, bytes));
    else DC_HIP_TRY(hipDeviceSynchronize());      // (work of earlier calls may still read the old weights)
    DC_HIP_TRY(hipMemcpy(d->d_img, d->image.img.data(), bytes, hipMemcpyHostToDevice));
    d->image.img = std::vector<float>();
    d->finalized = true;
    return DC_OK;
}

int dc_discriminator_features(dc_discriminator* d, const float* d_motion, int32_t B, int32_t T, float* d_feat, void* stream) {
    if (!d || !d_motion || !d_feat) return dc_set_error(DC_ERR_INVALID, "dc_discriminator_features: NULL argument");
    if (const int rc = disc_check("dc_discriminator_features", d, B, T)) return rc;
    DC_HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = (hipStream_t)stream;
    const DiscPlan pl(B, T);
    if (const int rc = d->ws.reserve(pl.floats, st)) return rc;
    const int L = pl.L[kDiscStages];
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        if (const int rc = stages_run(d, pl, d_motion + (size_t)b0 * T * R_POSE, nb, st)) return rc;
        k_disc_transpose<<<dim3((unsigned)((64 * L + 255) / 256), nb), 256, 0, st>>>(d->ws.p + pl.plane[2], d_feat + (size_t)b0 * 64 * L, L);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

int dc_discriminator_score(dc_discriminator* d, const float* d_motion, int32_t B, int32_t T, float* d_out, void* stream) {
    if (!d || !d_motion || !d_out) return dc_set_error(DC_ERR_INVALID, "dc_discriminator_score: NULL argument");
    if (const int rc = disc_check("dc_discriminator_score", d, B, T)) return rc;
    DC_HIP_TRY(hipSetDevice(d->device));
    hipStream_t st = (hipStream_t)stream;
    const DiscPlan pl(B, T);
    if (const int rc = d->ws.reserve(pl.floats, st)) return rc;
    const int L = pl.L[kDiscStages];
    DiscHead hd;
    for (int i = 0; i < 3; ++i) hd.w[i] = (unsigned)d->image.fw[i], hd.b[i] = (unsigned)d->image.fb[i];
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        if (const int rc = stages_run(d, pl, d_motion + (size_t)b0 * T * R_POSE, nb, st)) return rc;
        float* score = d->ws.p + pl.score;
        k_disc_head<<<dim3((unsigned)(((L + 31) / 32 + R_WAVES - 1) / R_WAVES), nb), 64 * R_WAVES, 0, st>>>(d->ws.p + pl.plane[2], d->d_img, hd, score, L);
        k_disc_mean<<<(unsigned)((nb + 63) / 64), 64, 0, st>>>(score, d_out + b0, nb, L);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

}  // extern "C"
