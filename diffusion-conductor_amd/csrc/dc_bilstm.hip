// dc_bilstm.hip - the BiLSTM pose decoder of the CNN-LSTM baselines on gfx950 (MI355X).
//
// Reference (restated, not translated): PoseDecoderBiLSTM, Contrastive_Stage/models/Generator.py:7-31, in eval mode,
//   LSTM_out = nn.LSTM(In, 128, num_layers = 2, bidirectional, batch_first)(feat)     [B, T, 256]   h0 = c0 = 0, dropout = identity
//   pose     = out(LSTM_out)                                                         [B, T, 26]    Linear 256-64, ReLU, 64-64, ReLU, 64-26, Sigmoid
// One direction of one layer (torch's gate order i, f, g, o; rows 128 gate + j):
//   a_t = W_ih x_t + b_ih + W_hh h_{t-1} + b_hh,   c_t = s(a_f) c_{t-1} + s(a_i) tanh(a_g),   h_t = s(a_o) tanh(c_t)
// and layer 1 reads cat(forward, reverse) of layer 0.
//
// Kernels, per layer and pass of nb clips:
//   k_lstm_proj   G[t][d][row] = W_ih[d][row] . x[t] + (b_ih + b_hh)[d][row] for every frame and both directions: the k_gan_conv
//                 pattern (one wave = 32 frames of ONE clip x 64 of the 1024 rows, two accumulator tiles on
//                 v_mfma_f32_32x32x2_f32: exact fp32, one k-ordered chain per output from 0, the folded bias added behind it).
//   k_lstm_rec    the recurrence: ONE workgroup of 512 threads per (direction, clip).  Thread r owns gate row r: its 128 weights of
//                 W_hh[d] stay in registers for the whole sequence (256 KiB per direction do not fit the LDS).  A step: every
//                 thread reads h_{t-1} from LDS (float4 reads of one address per wave: broadcasts) and runs
//                 a = G[t][r]; for k = 0 .. 127: a = fmaf(W[k], h[k], a); a -> LDS; barrier; threads 0 .. 127 form c_t (kept in
//                 a register) and h_t, write it to the other LDS buffer and to H[t][128 d + j]; barrier.  G[t][r] is read
//                 kRing steps ahead into a register ring (a step is shorter than a trip to L2 / HBM); the barriers are raw
//                 s_barrier behind lgkmcnt(0) only, so the ring's loads stay in flight across them.
//   k_lstm_head   `out` on H of layer 1: the k_gan_head pattern with a 256-wide first layer.
// The recurrent kernel has no communication between workgroups, no atomics and no spin-wait; its only synchronisation is the
// workgroup barrier, in uniform control flow, 2 T + 1 of them for every thread.  A clip's result depends on that clip alone and
// is bit-identical in any batch and on every rerun.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "dc_common.h"
#include "dc_handle.h"
#include "dc_mfma_f32.h"

namespace {

using namespace dc_f32;

constexpr int L_WAVES = 4;                 // waves (frame tiles of one clip) per workgroup of the projection and the head
constexpr int kRing = 8;                   // steps a gate row's G is read ahead of its use
constexpr int L_CAP = 128;                 // clips per pass at most
constexpr size_t L_WS_FLOATS = (size_t)1 << 28;      // 1 GiB of workspace

// x [clips][T][K] -> G [clips][T][1024] (see the head of the file).  W: lstm_pack_proj image over k_pad columns, bias [1024].
// ROW64: K is a multiple of 64 and x 16-byte aligned - rows are read as float4s (load_row64); else one float per k-step.  Both
// forms feed the same chain in the same order.  Frames >= T of a partial tile compute on frame T - 1 and are not written.
template <bool ROW64>
__global__ __launch_bounds__(64 * L_WAVES) void k_lstm_proj(const float* __restrict__ x, int K, int k_pad, const float* __restrict__ W,
                                                           const float* __restrict__ bias, float* __restrict__ G, int T) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int t0 = (blockIdx.x * L_WAVES + (threadIdx.x >> 6)) * 32;
    if (t0 >= T) return;                 // wave-uniform; no barriers below
    const int t = t0 + j, rg = blockIdx.z;
    const bool inside = t < T;
    const size_t frame = (size_t)blockIdx.y * T + (inside ? t : T - 1);
    const float* row = x + frame * K;
    const float2* w2 = reinterpret_cast<const float2*>(W + (size_t)rg * 64 * k_pad) + lane;
    f32x16 a0 = {}, a1 = {};
    if (ROW64) {
#pragma unroll 1
        for (int cc = 0; cc < K / 64; ++cc) {
            f32x4 m[16];
            load_row64(row + cc * 64, m);
            const float2* wq = w2 + (size_t)cc * 32 * 64;
#pragma unroll
            for (int ks = 0; ks < 32; ++ks) {
                const float v = row_operand(m, ks, h);      // feature 64 cc + 2 ks + h
                const float2 ww = wq[ks * 64];
                a0 = mfma2(ww.x, v, a0);
                a1 = mfma2(ww.y, v, a1);
            }
        }
    } else {
#pragma unroll 1
        for (int ks = 0; ks < k_pad / 2; ++ks) {
            const int k = 2 * ks + h;
            const float v = k < K ? row[k] : 0.f;            // (the pad column of an odd K: weight 0 times 0)
            const float2 ww = w2[ks * 64];
            a0 = mfma2(ww.x, v, a0);
            a1 = mfma2(ww.y, v, a1);
        }
    }
    if (!inside) return;
    // accumulator register r of lane (j, h) = row (r & 3) + 8 (r >> 2) + 4 h (+ 32 in the second tile): float4 groups
    const float* b = bias + 64 * rg;
    float* dst = G + frame * 1024 + 64 * rg + 4 * h;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 y0, y1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = tile_channel(4 * q + e, h);
            y0[e] = a0[4 * q + e] + b[c];
            y1[e] = a1[4 * q + e] + b[c + 32];
        }
        *reinterpret_cast<f32x4*>(dst + 8 * q) = y0;
        *reinterpret_cast<f32x4*>(dst + 8 * q + 32) = y1;
    }
}

// expf / tanhf of the device library (no fast-math forms); NaN in, NaN out
DEV float sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// a workgroup barrier that orders LDS traffic only: the ring's global loads stay in flight across it (__syncthreads would wait for them)
DEV void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// G [clips][T][2][512], Whh [2][512][128] -> H [clips][T][256] (see the head of the file).  grid (2, clips), 512 threads.
__global__ __launch_bounds__(512) void k_lstm_rec(const float* __restrict__ G, const float* __restrict__ Whh, float* __restrict__ H, int T) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 128 + 512];      // h (two buffers), the step's 512 gate pre-activations
    const int tid = threadIdx.x, d = blockIdx.x;
    float w[128];
    {
        const f32x4* wp = reinterpret_cast<const f32x4*>(Whh + ((size_t)d * 512 + tid) * 128);
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            const f32x4 v = wp[q];
            w[4 * q] = v[0], w[4 * q + 1] = v[1], w[4 * q + 2] = v[2], w[4 * q + 3] = v[3];
        }
    }
    // step s works on frame s (forward) or T - 1 - s (reverse); steps past the end re-read the last one (loaded, never used)
    const auto frame = [&](int s) {
        s = s < T ? s : T - 1;
        return (size_t)(d ? T - 1 - s : s);
    };
    const float* g = G + (size_t)blockIdx.y * T * 1024 + d * 512 + tid;
    float* hout = H + (size_t)blockIdx.y * T * 256 + d * 128 + tid;
    float ring[kRing];
#pragma unroll
    for (int i = 0; i < kRing; ++i) ring[i] = g[frame(i) * 1024];
    if (tid < 128) lds[tid] = 0.f;       // h_{-1} = 0
    float c = 0.f;
    // One step; slot = t % kRing, a constant where this is called (ring[] stays in registers).
    const auto step = [&](int t, int slot) __attribute__((always_inline)) {
        // The slot's load was issued kRing steps ago; the kRing - 1 loads behind it may stay in flight (memory operations of a
        // wave complete in order, so the stores of h that waves 0 and 1 have issued since only make this wait earlier than
        // needed).  The wait names the slot's register, so no copy of it can be scheduled in front of the wait.
        asm volatile("s_waitcnt vmcnt(%1)" : "+v"(ring[slot]) : "n"(kRing - 1) : "memory");
        float a = ring[slot];
        ring[slot] = g[frame(t + kRing) * 1024];
        const f32x4* hp = reinterpret_cast<const f32x4*>(lds + (t & 1) * 128);
#pragma unroll
        for (int q = 0; q < 32; ++q) {
            const f32x4 hv = hp[q];
            a = fmaf(w[4 * q], hv[0], a);
            a = fmaf(w[4 * q + 1], hv[1], a);
            a = fmaf(w[4 * q + 2], hv[2], a);
            a = fmaf(w[4 * q + 3], hv[3], a);
        }
        lds[256 + tid] = a;
        lds_barrier();
        if (tid < 128) {
            const float ai = lds[256 + tid], af = lds[384 + tid], ag = lds[512 + tid], ao = lds[640 + tid];
            c = fmaf(sigmoid(af), c, sigmoid(ai) * tanhf(ag));
            const float hn = sigmoid(ao) * tanhf(c);
            lds[((t + 1) & 1) * 128 + tid] = hn;
            hout[frame(t) * 256] = hn;
        }
        lds_barrier();
    };
    // The weights and the ring's first loads have landed before the loop: inside it the compiler's counted vmcnt waits then
    // cover the ring alone (a wait left over from the weight loads would drain the ring at every turn).
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    lds_barrier();
    // T steps for every thread of the workgroup (t is uniform): whole turns of the ring, then the T % kRing steps left
    int t0 = 0;
#pragma unroll 1
    for (; t0 + kRing <= T; t0 += kRing) {
#pragma unroll
        for (int i = 0; i < kRing; ++i) step(t0 + i, i);
    }
#pragma unroll
    for (int i = 0; i < kRing - 1; ++i) {
        if (t0 + i >= T) break;
        step(t0 + i, i);
    }
}

// H [clips][T][256] -> pose [clips][T][26]: out.0 + ReLU, out.2 + ReLU, out.4 + sigmoid.  P: the decoder's image, hd its head
// offsets.  Frames >= T of a partial tile compute on frame T - 1 and are not written.
struct LstmHead {
    unsigned w[3], b[3];
};
__global__ __launch_bounds__(64 * L_WAVES) void k_lstm_head(const float* __restrict__ hid, const float* __restrict__ P, LstmHead hd,
                                                           float* __restrict__ pose, int T) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int t0 = (blockIdx.x * L_WAVES + (threadIdx.x >> 6)) * 32;
    if (t0 >= T) return;                 // wave-uniform; no barriers below
    const int t = t0 + j;
    const bool inside = t < T;
    const size_t frame = (size_t)blockIdx.y * T + (inside ? t : T - 1);
    const float* w0 = P + hd.w[0] + lane;
    f32x16 a0 = {}, a1 = {};
#pragma unroll 1
    for (int cc = 0; cc < 4; ++cc) {
        f32x4 m[16];
        load_row64(hid + frame * 256 + cc * 64, m);
#pragma unroll
        for (int ks = 0; ks < 32; ++ks) {
            const float v = row_operand(m, ks, h);          // channel 64 cc + 2 ks + h
            a0 = mfma2(w0[(cc * 32 + ks) * 64], v, a0);
            a1 = mfma2(w0[(128 + cc * 32 + ks) * 64], v, a1);
        }
    }
    add_bias<true>(a0, a1, P + hd.b[0], h);
    f32x16 c0 = {}, c1 = {};
    Layer<0, 32>::run<2, 32>(P + hd.w[1], lane, h, a0, a1, c0, c1);
    add_bias<true>(c0, c1, P + hd.b[1], h);
    f32x16 p0 = {}, p1 = {};
    Layer<0, 32>::run<1, 32>(P + hd.w[2], lane, h, c0, c1, p0, p1);      // 26 rows of one tile
    const float* b = P + hd.b[2];
    if (!inside) return;
    float* dst = pose + frame * 26;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = tile_channel(r, h);
        if (o < 26) dst[o] = sigmoid(p0[r] + b[o]);
    }
}

const char* const kWhat = "BiLSTM decoder";

}  // namespace

struct dc_bilstm {
    int device = 0;
    DcParams params;
    LstmImage image;                     // offsets (the floats themselves are dropped after the upload)
    float* d_img = nullptr;
    size_t img_floats = 0;
    DcWorkspace ws;
    bool finalized = false;
};

namespace {

// The one place where the pass size, the workgroup counts and the plane sizes come from (B, T).
struct LstmPlan {
    int chunk;                           // clips per pass: min(B, 128, floor(2^28 / (1536 T))), at least 1
    unsigned gx32;                       // workgroups per clip of the projection and the head (32-frame tiles, L_WAVES per workgroup)
    size_t frames;                       // chunk * T
    LstmPlan(int B, int T) {
        const size_t fit = L_WS_FLOATS / ((size_t)T * (kLstmRows + 4 * kLstmH));
        chunk = (int)(fit < 1 ? 1 : (fit < (size_t)L_CAP ? fit : (size_t)L_CAP));
        if (B < chunk) chunk = B;
        gx32 = (unsigned)(((T + 31) / 32 + L_WAVES - 1) / L_WAVES);
        frames = (size_t)chunk * T;
    }
    size_t floats() const { return frames * (kLstmRows + 4 * kLstmH); }      // G, H of layer 0, H of layer 1
};

// feat [nb][T][In] -> the LSTM's output after `layers` layers, [nb][T][256] at *hid (one of the workspace planes)
int lstm_run(dc_bilstm* m, const LstmPlan& pl, const float* feat, int nb, int T, int layers, const float** hid, hipStream_t st) {
    float* G = m->ws.p;
    float* Hs[2] = {G + pl.frames * kLstmRows, G + pl.frames * (kLstmRows + 2 * kLstmH)};
    const float* P = m->d_img;
    const LstmImage& I = m->image;
    const dim3 gp(pl.gx32, nb, kLstmRows / 64);
    const float* x = feat;
    for (int l = 0; l < layers; ++l) {
        const int K = l ? 2 * kLstmH : I.in;
        if (K % 64 == 0 && !((uintptr_t)x & 15))
            k_lstm_proj<true><<<gp, 64 * L_WAVES, 0, st>>>(x, K, I.k_pad[l], P + I.wih[l], P + I.bias[l], G, T);
        else
            k_lstm_proj<false><<<gp, 64 * L_WAVES, 0, st>>>(x, K, I.k_pad[l], P + I.wih[l], P + I.bias[l], G, T);
        k_lstm_rec<<<dim3(2, nb), 512, 0, st>>>(G, P + I.whh[l], Hs[l], T);
        x = Hs[l];
    }
    DC_HIP_TRY(hipGetLastError());
    *hid = x;
    return DC_OK;
}

int check_call(const char* fn, const dc_bilstm* m, int B, int T) {
    const std::string f(fn);
    if (!m->finalized) return dc_set_error(DC_ERR_INVALID, (f + " before dc_bilstm_finalize").c_str());
    if (B < 1) return dc_set_error(DC_ERR_INVALID, (f + ": B must be >= 1").c_str());
    if (T < 1) return dc_set_error(DC_ERR_INVALID, (f + ": T must be >= 1").c_str());
    return DC_OK;
}

}  // namespace

extern "C" {

int dc_bilstm_create(int32_t device, dc_bilstm** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_bilstm_create: out is NULL");
    *out = nullptr;
    if (const int rc = dc_check_device("dc_bilstm_create", device)) return rc;
    auto* m = new dc_bilstm;
    m->device = device;
    *out = m;
    return DC_OK;
}

void dc_bilstm_destroy(dc_bilstm* m) {
    if (!m) return;
    const DcDeviceGuard on(m->device);
    if (m->d_img) (void)hipFree(m->d_img);
    m->ws.release();
    delete m;
}

int dc_bilstm_set_param(dc_bilstm* m, const char* name, const float* h_data, int64_t numel) {
    if (!m || !name || !h_data) return dc_set_error(DC_ERR_INVALID, "dc_bilstm_set_param: NULL argument");
    const std::string k(name);
    bool changed = false;
    int rc;
    if (k == "LSTM.weight_ih_l0" || k == "LSTM.weight_ih_l0_reverse") {      // [512, In]: In is fixed at finalize
        if (numel < kLstmGates || numel % kLstmGates || numel / kLstmGates > kLstmMaxIn)
            return dc_set_error(DC_ERR_PARAM, (std::string(kWhat) + " parameter " + k + " has " + std::to_string(numel) +
                                               " elements, expected 512 x an input size of 1 .. 128").c_str());
        m->params[k].assign(h_data, h_data + numel);
        changed = true;
        rc = DC_OK;
    } else {
        rc = dc_param_take(kWhat, lstm_required(1), {}, k, k, h_data, numel, &m->params, &changed);
    }
    if (changed) m->finalized = false;
    return rc;
}

int dc_bilstm_finalize(dc_bilstm* m) {
    if (!m) return dc_set_error(DC_ERR_INVALID, "dc_bilstm_finalize: NULL handle");
    m->finalized = false;
    const auto w0 = m->params.find("LSTM.weight_ih_l0");
    if (w0 == m->params.end()) return dc_set_error(DC_ERR_PARAM, (std::string(kWhat) + " parameter LSTM.weight_ih_l0 was not set").c_str());
    const int in = (int)(w0->second.size() / kLstmGates);
    const DcParamList need = lstm_required(in);
    if (const int rc = dc_param_complete(kWhat, need, m->params)) return rc;
    for (const auto& r : need)
        if (m->params[r.first].size() != r.second)
            return dc_set_error(DC_ERR_PARAM, (std::string(kWhat) + " parameter " + r.first + " has " + std::to_string(m->params[r.first].size()) +
                                               " elements, expected " + std::to_string(r.second) + " (input size " + std::to_string(in) + ")").c_str());
    DC_HIP_TRY(hipSetDevice(m->device));
    m->image = lstm_pack(m->params, in);
    const size_t n = m->image.img.size();
    if (m->d_img && m->img_floats != n) {
        DC_HIP_TRY(hipDeviceSynchronize());     // (work of earlier calls may still read the old image)
        DC_HIP_TRY(hipFree(m->d_img));
        m->d_img = nullptr;
    }
    if (!m->d_img) DC_HIP_TRY(hipMalloc((void**)&m->d_img, n * sizeof(float)));
    m->img_floats = n;
    DC_HIP_TRY(hipMemcpy(m->d_img, m->image.img.data(), n * sizeof(float), hipMemcpyHostToDevice));
    m->image.img = std::vector<float>();
    m->finalized = true;
    return DC_OK;
}

int32_t dc_bilstm_input_size(const dc_bilstm* m) { return m && m->finalized ? m->image.in : 0; }

int dc_bilstm_decode(dc_bilstm* m, const float* d_feat, int32_t B, int32_t T, float* d_pose, void* stream) {
    if (!m || !d_feat || !d_pose) return dc_set_error(DC_ERR_INVALID, "dc_bilstm_decode: NULL argument");
    if (const int rc = check_call("dc_bilstm_decode", m, B, T)) return rc;
    DC_HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    const LstmPlan pl(B, T);
    if (const int rc = m->ws.reserve(pl.floats(), st)) return rc;
    LstmHead hd;
    for (int i = 0; i < 3; ++i) hd.w[i] = (unsigned)m->image.hw[i], hd.b[i] = (unsigned)m->image.hb[i];
    const int in = m->image.in;
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        const float* hid = nullptr;
        if (const int rc = lstm_run(m, pl, d_feat + (size_t)b0 * T * in, nb, T, 2, &hid, st)) return rc;
        k_lstm_head<<<dim3(pl.gx32, nb), 64 * L_WAVES, 0, st>>>(hid, m->d_img, hd, d_pose + (size_t)b0 * T * kLstmPose, T);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

int dc_bilstm_hidden(dc_bilstm* m, const float* d_feat, int32_t B, int32_t T, int32_t layers, float* d_h, void* stream) {
    if (!m || !d_feat || !d_h) return dc_set_error(DC_ERR_INVALID, "dc_bilstm_hidden: NULL argument");
    if (const int rc = check_call("dc_bilstm_hidden", m, B, T)) return rc;
    if (layers < 1 || layers > 2) return dc_set_error(DC_ERR_INVALID, "dc_bilstm_hidden: layers must be 1 or 2");
    DC_HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    const LstmPlan pl(B, T);
    if (const int rc = m->ws.reserve(pl.floats(), st)) return rc;
    const int in = m->image.in;
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        const float* hid = nullptr;
        if (const int rc = lstm_run(m, pl, d_feat + (size_t)b0 * T * in, nb, T, layers, &hid, st)) return rc;
        DC_HIP_TRY(hipMemcpyAsync(d_h + (size_t)b0 * T * 256, hid, (size_t)nb * T * 256 * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DC_OK;
    });
}

int32_t dc_bilstm_pass_clips(int32_t B, int32_t T) { return B < 1 || T < 1 ? 0 : LstmPlan(B, T).chunk; }

}  // extern "C"
