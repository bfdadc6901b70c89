// dc_mel.hip - the mel spectrogram of a waveform, the first step of "audio in, poses out", on gfx950 (MI355X).
//
// Reference (restated, not translated): extract_mel_feature, Diffusion_Stage/tools/visualization.py:152-167 =
// Contrastive_Stage/utils/music_utils.py:8-23 = ProspectiveCup/utils/music_utils.py:
//   librosa.feature.melspectrogram(y, sr, n_mels=128, hop_length=256)   STFT (n_fft 2048, periodic Hann, center=True, power 2) and
//                                                                       the Slaney filterbank
//   librosa.power_to_db(mel, ref=np.max)                                10 log10(max(p, 1e-10)) - 10 log10(max(ref, 1e-10)), clamped
//                                                                       at max - 80
//   np.flip(np.abs(dB + 80) / 80, 0)                                    channel 0 is the HIGHEST band
//   cv2.resize(.., (mel_len_90fps, 128))                                INTER_LINEAR along time
//
// Kernels (all arithmetic fp32 on tables built in fp64 on the host - dc_pack.h, mel_tables -; no atomics, every sum in a fixed order:
// a clip's numbers are bit-identical on a rerun, in any batch and in any chunking):
//   k_mel_power    one workgroup = 8 consecutive frames of ONE clip, one wave per frame, two rounds.  The 3840 samples the 8 frames
//                  span are staged in LDS once (padding applied there: zeros or the reflection), then per frame: window, the
//                  2048-point real transform as a 1024-point complex FFT of the even / odd packed samples - five radix-4 Stockham
//                  stages in LDS, no bit reversal, twiddles from the uploaded table - and the split post-pass, re^2 + im^2 of the
//                  1025 bins into LDS, the sparse triangles as one fmaf chain per band in bin order, 128 numbers out.  A frame's
//                  spectrum never goes to global memory.  The workgroup's maximum of what it wrote goes to a partials array.
//                  LDS: real and imaginary parts as separate float arrays, index i at i + (i >> 5): a stage reads lane-contiguous
//                  (t, t + 256, t + 512, t + 768: conflict-free) and writes at stride 4 s, which the skew spreads over the banks
//                  (s = 1: conflict-free, s = 4, 16: 2-way, free on a ds_write_b32).
//   k_mel_ref      one workgroup per clip: the maximum of the clip's partials (its own workgroups only), NaN kept.
//   k_mel_finish   one thread per output element: dB against the clip's ref, the clamp, |dB + 80| / 80, the flip, cv2's INTER_LINEAR.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "dc_common.h"
#include "dc_handle.h"
#include "dc_mfma_f32.h"

namespace {

constexpr int M_HALF = kMelFft / 2;                          // points of the complex transform
constexpr int M_FPW = 8;                                     // frames per workgroup
constexpr int M_WAVES = 4;                                   // waves per workgroup: one frame each, M_FPW / M_WAVES rounds
constexpr int M_TILE = (M_FPW - 1) * kMelHop + kMelFft;      // samples the workgroup's frames span
constexpr int M_SKEW = M_HALF + M_HALF / 32;                 // floats of one skewed plane
constexpr int M_CHUNK = 32;                                  // most clips per pass (bounds MelClips and the grid)
constexpr size_t M_PASS_FLOATS = (size_t)1 << 27;            // the power plane of a pass stays within 512 MiB (one clip may exceed it)
constexpr int M_REF_THREADS = 256;

struct MelClips {
    int n[M_CHUNK];                      // samples of each clip of a pass
    int tm[M_CHUNK];                     // its output frames (k_mel_finish)
};

DEV int skew(int i) { return i + (i >> 5); }

// One radix-4 Stockham stage (decimation in frequency) of a wave's 1024 points: sub-transform length 1024 / S, stride S.  Butterfly
// t = p S + q reads t + 256 k and writes q + S (4 p + k), k = 0 .. 3, times exp(-2 pi i k p S / 1024) = tw[2 k p S].
template <int S>
DEV void fft_stage(float* re, float* im, const float2* __restrict__ tw, int lane) {
    float xr[4][4], xi[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = skew(lane + 64 * j + 256 * k);
            xr[j][k] = re[a];
            xi[j][k] = im[a];
        }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = lane + 64 * j, q = t & (S - 1), ps = t - q;
        const float apcr = xr[j][0] + xr[j][2], apci = xi[j][0] + xi[j][2], amcr = xr[j][0] - xr[j][2], amci = xi[j][0] - xi[j][2];
        const float bpdr = xr[j][1] + xr[j][3], bpdi = xi[j][1] + xi[j][3], bmdr = xr[j][1] - xr[j][3], bmdi = xi[j][1] - xi[j][3];
        float yr[4], yi[4];
        yr[0] = apcr + bpdr, yi[0] = apci + bpdi;
        yr[1] = amcr + bmdi, yi[1] = amci - bmdr;        // (a - c) - i (b - d)
        yr[2] = apcr - bpdr, yi[2] = apci - bpdi;
        yr[3] = amcr - bmdi, yi[3] = amci + bmdr;        // (a - c) + i (b - d)
        if (S < 256) {                                   // (the last stage's p is 0)
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                const float2 w = tw[2 * k * ps];
                const float r = yr[k] * w.x - yi[k] * w.y, i = yr[k] * w.y + yi[k] * w.x;
                yr[k] = r, yi[k] = i;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = skew(q + 4 * ps + S * k);
            re[a] = yr[k];
            im[a] = yi[k];
        }
    }
    __syncthreads();
}

// wave [nb][N] -> pw [nb][F][128], part [nb][gridDim.x].  tab: window [2048], twiddles [2048][2], the filters' weights; idx: first,
// offset, count [128] each.
__global__ __launch_bounds__(64 * M_WAVES) void k_mel_power(const float* __restrict__ wave, const float* __restrict__ tab, const int* __restrict__ idx,
                                                           float* __restrict__ pw, float* __restrict__ part, int N, int F, int reflect, MelClips cl) {
    __shared__ __attribute__((aligned(16))) float tile[M_TILE];
    __shared__ float zr[M_WAVES][M_SKEW], zi[M_WAVES][M_SKEW];
    __shared__ float wmax[M_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.y, f0 = blockIdx.x * M_FPW;
    const int n = cl.n[b], Fb = 1 + n / kMelHop;
    float* out = pw + ((size_t)b * F + f0) * kMelBands;
    if (f0 >= Fb) {                      // block-uniform: rows behind the clip's own frames are 0 and raise no maximum
        for (int i = tid; i < M_FPW * kMelBands; i += 64 * M_WAVES)
            if (f0 + i / kMelBands < F) out[i] = 0.f;
        if (tid == 0) part[(size_t)b * gridDim.x + blockIdx.x] = 0.f;
        return;
    }
    const float* y = wave + (size_t)b * N;
    const long long g0 = (long long)f0 * kMelHop - M_HALF;      // (64-bit: 2 (n - 1) below leaves int32 for n > 2^30)
    for (int i = tid; i < M_TILE; i += 64 * M_WAVES) {
        long long g = g0 + i;
        if (reflect) g = g < 0 ? -g : (g >= n ? 2 * ((long long)n - 1) - g : g);      // y[1024 .. 1] in front, y[n - 2 .. n - 1025] behind
        tile[i] = (g >= 0 && g < n) ? y[g] : 0.f;                          // (outside after the reflection: frames >= Fb only)
    }
    __syncthreads();
    const float2* win2 = reinterpret_cast<const float2*>(tab);
    const float2* tw = reinterpret_cast<const float2*>(tab + kMelFft);
    const float* fw = tab + 3 * kMelFft;
    float* re = zr[w];
    float* im = zi[w];
    float vmax = 0.f;
    for (int round = 0; round < M_FPW / M_WAVES; ++round) {
        const int fl = round * M_WAVES + w, f = f0 + fl;
        const float2* x2 = reinterpret_cast<const float2*>(tile + fl * kMelHop);
#pragma unroll 4
        for (int j = 0; j < M_HALF / 64; ++j) {      // z[n] = x[2 n] w[2 n] + i x[2 n + 1] w[2 n + 1]
            const int i = lane + 64 * j;
            const float2 x = x2[i], ww = win2[i];
            re[skew(i)] = x.x * ww.x;
            im[skew(i)] = x.y * ww.y;
        }
        __syncthreads();
        fft_stage<1>(re, im, tw, lane);
        fft_stage<4>(re, im, tw, lane);
        fft_stage<16>(re, im, tw, lane);
        fft_stage<64>(re, im, tw, lane);
        fft_stage<256>(re, im, tw, lane);
        // X[k] = (S + T) / 2, X[1024 - k] = conj(S - T) / 2 with S = Z[k] + conj(Z[1024 - k]), T = W^k (-i)(Z[k] - conj(Z[1024 - k])),
        // W = exp(-2 pi i / 2048): lane l takes k = l + 64 j, j = 0 .. 7, lane 0 also k = 512
        float pk[9], pm[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            const int k = lane + 64 * j;
            pk[j] = pm[j] = 0.f;
            if (j < 8 || lane == 0) {
                const int ka = skew(k), kb = skew((M_HALF - k) & (M_HALF - 1));
                const float ar = re[ka], ai = im[ka], cr = re[kb], ci = im[kb];
                const float2 wk = tw[k];
                const float sr = ar + cr, si = ai - ci, orr = ai + ci, oi = cr - ar;
                const float tr = wk.x * orr - wk.y * oi, ti = wk.x * oi + wk.y * orr;
                const float ur = sr + tr, ui = si + ti, vr = sr - tr, vi = si - ti;
                pk[j] = 0.25f * (ur * ur + ui * ui);
                pm[j] = 0.25f * (vr * vr + vi * vi);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 9; ++j) {      // the power of bin k at re[k], unskewed (1025 <= M_SKEW)
            const int k = lane + 64 * j;
            if (j < 8 || lane == 0) {
                re[k] = pk[j];
                if (j < 8) re[M_HALF - k] = pm[j];
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < kMelBands / 64; ++h) {
            const int m = lane + 64 * h;
            const int first = idx[m], cnt = idx[2 * kMelBands + m];
            const float* wt = fw + idx[kMelBands + m];
            float s = 0.f;
            for (int i = 0; i < cnt; ++i) s = fmaf(wt[i], re[first + i], s);
            if (f < Fb) vmax = nanmax(vmax, s);
            if (f < F) out[(size_t)fl * kMelBands + m] = f < Fb ? s : 0.f;
        }
        __syncthreads();                 // (the next round's window pass rewrites the planes)
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) vmax = nanmax(vmax, __shfl_xor(vmax, m));
    if (lane == 0) wmax[w] = vmax;
    __syncthreads();
    if (tid == 0) {
        float v = wmax[0];
#pragma unroll
        for (int i = 1; i < M_WAVES; ++i) v = nanmax(v, wmax[i]);
        // A maximum that is not finite is NaN: an infinite sample leaves inf - inf in the reference's transform, and the whole clip NaN.
        part[(size_t)b * gridDim.x + blockIdx.x] = (v - v == 0.f) ? v : __builtin_nanf("");
    }
}

// part [nb][nwg] -> ref [nb]: the maximum over the workgroups that hold the clip's own frames, NaN kept
__global__ __launch_bounds__(M_REF_THREADS) void k_mel_ref(const float* __restrict__ part, float* __restrict__ ref, int nwg, MelClips cl) {
    __shared__ float buf[M_REF_THREADS];
    const int Fb = 1 + cl.n[blockIdx.x] / kMelHop, mine = (Fb + M_FPW - 1) / M_FPW;
    const float* p = part + (size_t)blockIdx.x * nwg;
    float v = 0.f;
    for (int i = threadIdx.x; i < mine; i += M_REF_THREADS) v = nanmax(v, p[i]);
    buf[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = M_REF_THREADS / 2; off >= 1; off >>= 1) {
        if ((int)threadIdx.x < off) buf[threadIdx.x] = nanmax(buf[threadIdx.x], buf[threadIdx.x + off]);
        __syncthreads();
    }
    if (threadIdx.x == 0) ref[blockIdx.x] = buf[0];
}

// |power_to_db + 80| / 80 of one power value: lref = 10 log10(max(ref, 1e-10)), floor_db = max_dB - 80.  Every operation rounded on
// its own (the pragma: a fused 10 log - lref would leave silence a hair off dB = 0); the maxima are numpy's, which keep a NaN.
DEV float mel_unit(float p, float lref, float floor_db) {
#pragma clang fp contract(off)
    float db = 10.f * log10f(nanmax(1e-10f, p)) - lref;
    db = nanmax(db, floor_db);
    return fabsf(db + 80.f) / 80.f;
}

// pw [nb][F][128], ref [nb] -> mel [nb][Tm][128]; one thread per element, 2 rows per workgroup
__global__ __launch_bounds__(2 * kMelBands) void k_mel_finish(const float* __restrict__ pw, const float* __restrict__ ref, float* __restrict__ mel,
                                                            int F, int Tm, MelClips cl) {
#pragma clang fp contract(off)
    const int b = blockIdx.y, c = threadIdx.x & (kMelBands - 1), j = blockIdx.x * 2 + (threadIdx.x >> 7);
    if (j >= Tm) return;
    float* dst = mel + ((size_t)b * Tm + j) * kMelBands + c;
    const int Fb = 1 + cl.n[b] / kMelHop, Tb = cl.tm[b];
    if (j >= Tb) {
        *dst = 0.f;
        return;
    }
    // cv2's INTER_LINEAR: the source coordinate in double, rounded to fp32, clamped at both ends
    const float x = (float)(((double)j + 0.5) * ((double)Fb / (double)Tb) - 0.5);
    int i = (int)floorf(x);
    float wgt = x - (float)i;
    if (i < 0) i = 0, wgt = 0.f;
    if (i >= Fb - 1) i = Fb - 1, wgt = 0.f;
    const int i1 = i + 1 < Fb ? i + 1 : Fb - 1;
    const float r = ref[b];
    const float lref = 10.f * log10f(nanmax(1e-10f, r));
    const float floor_db = (lref - lref) - 80.f;         // max_dB is the dB of ref itself: 0, or NaN with ref
    const float* src = pw + (size_t)b * F * kMelBands + (kMelBands - 1 - c);      // the flip: channel c is band 127 - c
    const float v0 = mel_unit(src[(size_t)i * kMelBands], lref, floor_db), v1 = mel_unit(src[(size_t)i1 * kMelBands], lref, floor_db);
    *dst = v0 * (1.f - wgt) + v1 * wgt;
}

int mel_pass_clips(int N) {
    const size_t per_clip = (size_t)(1 + N / kMelHop) * kMelBands;
    const size_t c = M_PASS_FLOATS / per_clip;
    return c < 1 ? 1 : (c > (size_t)M_CHUNK ? M_CHUNK : (int)c);
}

}  // namespace

struct dc_mel {
    int device = 0, sr = 22050, reflect = 0;
    float* d_tab = nullptr;              // window [2048], twiddles [2048][2], filter weights
    int* d_idx = nullptr;                // first, offset, count [128] each
    DcWorkspace ws;
};

namespace {

// What both entry points refuse, before any launch.
int mel_check(const char* fn, const dc_mel* h, const float* d_wave, const int32_t* h_lengths, int B, int N) {
    const std::string f(fn);
    if (!h || !d_wave) return dc_set_error(DC_ERR_INVALID, (f + ": NULL argument").c_str());
    if (B < 1) return dc_set_error(DC_ERR_INVALID, (f + ": B must be >= 1").c_str());
    if (N < kMelFft) return dc_set_error(DC_ERR_INVALID, (f + ": " + std::to_string(N) + " samples; one 2048-sample window needs N >= 2048").c_str());
    if (reinterpret_cast<uintptr_t>(d_wave) % 4) return dc_set_error(DC_ERR_INVALID, (f + ": the waveform must be 4-byte aligned").c_str());
    if (h_lengths)
        for (int b = 0; b < B; ++b)
            if (h_lengths[b] < kMelFft || h_lengths[b] > N)
                return dc_set_error(DC_ERR_INVALID, (f + ": length " + std::to_string(h_lengths[b]) + " of clip " + std::to_string(b) +
                                                     " is outside [2048, " + std::to_string(N) + "]").c_str());
    return DC_OK;
}

MelClips mel_clips(const int32_t* h_lengths, const int32_t* out_frames, int b0, int nb, int N) {
    MelClips cl;
    for (int i = 0; i < M_CHUNK; ++i) {
        cl.n[i] = i < nb ? (h_lengths ? h_lengths[b0 + i] : N) : kMelFft;
        cl.tm[i] = i < nb && out_frames ? out_frames[b0 + i] : 1;
    }
    return cl;
}

// the power pass of the clips [b0, b0 + nb): pw [nb][F][128], part [nb][nwg]
void power_run(const dc_mel* h, const float* d_wave, int nb, int N, int F, const MelClips& cl, float* pw, float* part, hipStream_t st) {
    const int nwg = (F + M_FPW - 1) / M_FPW;
    k_mel_power<<<dim3((unsigned)nwg, (unsigned)nb), 64 * M_WAVES, 0, st>>>(d_wave, h->d_tab, h->d_idx, pw, part, N, F, h->reflect, cl);
}

}  // namespace

extern "C" {

int dc_mel_tables(int32_t sr, float* h_window, float* h_twiddle, int32_t* h_first, int32_t* h_count, float* h_weights, int32_t max_weights,
                  int32_t* h_total) {
    if (sr < 1) return dc_set_error(DC_ERR_INVALID, "dc_mel_tables: sr must be >= 1");
    const MelTables t = mel_tables(sr);
    if (h_total) *h_total = (int32_t)t.weights.size();
    if (h_weights && (size_t)max_weights < t.weights.size())
        return dc_set_error(DC_ERR_INVALID, ("dc_mel_tables: " + std::to_string(t.weights.size()) + " weights do not fit " + std::to_string(max_weights)).c_str());
    if (h_window) std::copy(t.window.begin(), t.window.end(), h_window);
    if (h_twiddle) std::copy(t.twiddle.begin(), t.twiddle.end(), h_twiddle);
    if (h_first) std::copy(t.first.begin(), t.first.end(), h_first);
    if (h_count) std::copy(t.count.begin(), t.count.end(), h_count);
    if (h_weights) std::copy(t.weights.begin(), t.weights.end(), h_weights);
    return DC_OK;
}

int32_t dc_mel_out_frames(int64_t n, int32_t sr) { return n < 0 || sr < 1 ? 0 : mel_out_frames(n, sr); }

int32_t dc_mel_pass_clips(int32_t N) { return N < kMelFft ? 0 : mel_pass_clips(N); }

int dc_mel_create(int32_t device, int32_t sr, int32_t pad_mode, dc_mel** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_mel_create: out is NULL");
    *out = nullptr;
    if (sr < 1) return dc_set_error(DC_ERR_INVALID, ("dc_mel_create: sr " + std::to_string(sr) + " must be >= 1").c_str());
    if (pad_mode != DC_MEL_PAD_CONSTANT && pad_mode != DC_MEL_PAD_REFLECT)
        return dc_set_error(DC_ERR_INVALID, ("dc_mel_create: unknown pad_mode " + std::to_string(pad_mode) + " (0 constant, 1 reflect)").c_str());
    if (const int rc = dc_check_device("dc_mel_create", device)) return rc;
    const MelTables t = mel_tables(sr);
    std::vector<float> tab(t.window);
    tab.insert(tab.end(), t.twiddle.begin(), t.twiddle.end());
    tab.insert(tab.end(), t.weights.begin(), t.weights.end());
    std::vector<int32_t> idx(t.first);
    idx.insert(idx.end(), t.offset.begin(), t.offset.end());
    idx.insert(idx.end(), t.count.begin(), t.count.end());
    const DcDeviceGuard on(device);
    auto* h = new dc_mel;
    h->device = device, h->sr = sr, h->reflect = pad_mode == DC_MEL_PAD_REFLECT;
    hipError_t e = hipMalloc((void**)&h->d_tab, tab.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_idx, idx.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(h->d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(h->d_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (h->d_tab) (void)hipFree(h->d_tab);
        if (h->d_idx) (void)hipFree(h->d_idx);
        delete h;
        return dc_set_error(DC_ERR_HIP, (std::string("dc_mel_create: ") + hipGetErrorString(e)).c_str());
    }
    *out = h;
    return DC_OK;
}

void dc_mel_destroy(dc_mel* h) {
    if (!h) return;
    const DcDeviceGuard on(h->device);
    if (h->d_tab) (void)hipFree(h->d_tab);
    if (h->d_idx) (void)hipFree(h->d_idx);
    h->ws.release();
    delete h;
}

int dc_mel_power(dc_mel* h, const float* d_wave, const int32_t* h_lengths, int32_t B, int32_t N, float* d_pow, void* stream) {
    if (!d_pow) return dc_set_error(DC_ERR_INVALID, "dc_mel_power: NULL argument");
    if (const int rc = mel_check("dc_mel_power", h, d_wave, h_lengths, B, N)) return rc;
    DC_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int F = 1 + N / kMelHop, nwg = (F + M_FPW - 1) / M_FPW;
    const int chunk = B < M_CHUNK ? B : M_CHUNK;
    if (const int rc = h->ws.reserve((size_t)chunk * nwg, st)) return rc;
    return dc_chunks(B, chunk, [&](int b0, int nb) -> int {
        power_run(h, d_wave + (size_t)b0 * N, nb, N, F, mel_clips(h_lengths, nullptr, b0, nb, N), d_pow + (size_t)b0 * F * kMelBands, h->ws.p, st);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

int dc_mel_features(dc_mel* h, const float* d_wave, const int32_t* h_lengths, int32_t B, int32_t N, const int32_t* h_out_frames, int32_t Tm,
                    float* d_mel, void* stream) {
    if (!d_mel) return dc_set_error(DC_ERR_INVALID, "dc_mel_features: NULL argument");
    if (const int rc = mel_check("dc_mel_features", h, d_wave, h_lengths, B, N)) return rc;
    if (Tm < 1) return dc_set_error(DC_ERR_INVALID, "dc_mel_features: Tm must be >= 1");
    std::vector<int32_t> tm(B);
    for (int b = 0; b < B; ++b) {
        tm[b] = h_out_frames ? h_out_frames[b] : mel_out_frames(h_lengths ? h_lengths[b] : N, h->sr);
        if (tm[b] < 1 || tm[b] > Tm)
            return dc_set_error(DC_ERR_INVALID, (std::string("dc_mel_features: ") + (h_out_frames ? "" : "the default of ") + std::to_string(tm[b]) +
                                                 " output frames of clip " + std::to_string(b) + " is outside [1, " + std::to_string(Tm) + "]").c_str());
    }
    DC_HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int F = 1 + N / kMelHop, nwg = (F + M_FPW - 1) / M_FPW;
    const int pass = mel_pass_clips(N), chunk = B < pass ? B : pass;
    const size_t plane = (size_t)chunk * F * kMelBands, parts = (((size_t)chunk * nwg + 63) & ~(size_t)63);
    if (const int rc = h->ws.reserve(plane + parts + M_CHUNK, st)) return rc;
    float *pw = h->ws.p, *part = pw + plane, *ref = part + parts;
    return dc_chunks(B, chunk, [&](int b0, int nb) -> int {
        const MelClips cl = mel_clips(h_lengths, tm.data(), b0, nb, N);
        power_run(h, d_wave + (size_t)b0 * N, nb, N, F, cl, pw, part, st);
        k_mel_ref<<<nb, M_REF_THREADS, 0, st>>>(part, ref, nwg, cl);
        k_mel_finish<<<dim3((unsigned)((Tm + 1) / 2), (unsigned)nb), 2 * kMelBands, 0, st>>>(pw, ref, d_mel + (size_t)b0 * Tm * kMelBands, F, Tm, cl);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

}  // extern "C"
