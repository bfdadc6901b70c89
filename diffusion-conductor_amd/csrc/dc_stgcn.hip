// dc_stgcn.hip - M2SNet's ST-GCN motion encoder (the evaluation metrics' latent space) on gfx950 (MI355X).
//
// Reference (restated, not translated): Diffusion_Stage/trainers/ddpm_trainer.py:27-63 MotionEncoder_STGCN,
// models/ST_GCN/ST_GCN.py (ST_GCN, mode 'M2S', and st_gcn), models/ST_GCN/st_gcn_utils/tgcn.py (ConvTemporalGraphical),
// in eval mode (BatchNorm on running statistics, eps 1e-5; dropout 0):
//   x [N, T, 13, 2] -> data_bn (BatchNorm1d over 26 channels v*2 + c)
//   10 st_gcn blocks (2 -> 32, then 32 -> 32):  y = relu( BN3( tconv3( relu( BN0( mix_A( conv1x1(x) ) ) ) ) ) + res(x) )
//      mix_A: y[c, t, w] = sum_v y[c, t, v] Ahat[v, w],  Ahat = A (.) edge_importance[l]  (uniform strategy: K = 1)
//      tconv3: kernel (3, 1), zero padding 1;  res: none in block 0, identity after
//   [N, 32, T, 13] -> 416 channels per frame (c*13 + v) -> Conv1d 416 -> 64 + BatchNorm1d  = the latent [N, 64, T]
//
// Folding (host, fp64, at finalize).  BN0 follows the graph mix, which is linear over joints, so it folds into the 1x1 conv:
//   W1' = s0 W1,  b1'[c, w] = s0[c] b1[c] sum_v Ahat[v, w] + h0[c]   (the conv bias goes through the mix)
// BN3 folds into the temporal conv (W2' = s3 W2, b2' = s3 b2 + h3), the fc BatchNorm into the fc conv, and data_bn becomes a
// per-(joint, coord) affine applied while block 0 stages its input.  The mix is applied to the block INPUT (it commutes with
// the 1x1 conv): x_w = sum_v Ahat[v, w] x_v on the VALU, then one K = C_in GEMM per joint.
//
// Kernels.  Activations between blocks are fp32 [b][v][c][t] (frames contiguous).  k_stgcn_block: one workgroup = 30 output
// frames of ONE clip, 13 waves (wave w = joint w).  It stages the block input of frames f0-1 .. f0+30 (one halo frame each
// side) in LDS; each wave mixes its joint's input from LDS straight into v_mfma_f32_32x32x2_f32 B operands (32 frames on the
// lanes), runs the 1x1 conv (16 MFMAs; block 0: one), adds b1', ReLU, zeroes frames outside [0, T) (the temporal conv's zero
// padding), writes its own 32 x 34 activation tile to LDS and runs the temporal conv as three shifted K = 32 products
// (48 MFMAs), then b2', residual, ReLU and the store of frames f0 .. f0+29 (tile columns 1 .. 30).  k_stgcn_fc: the 416 -> 64
// conv, one wave per 32 frames, the weights as lane-major fragments read from L2.
// Precision: every product is an exact-fp32 MFMA (a k-ordered fmaf chain); no reduction crosses clips, so a clip's latent is
// bit-identical alone and at any position in any batch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/dc_ddim.h"
#include "dc_common.h"

int dc_set_error(int code, const char* msg);      // dc_api.hip: sets dc_last_error's message

namespace {

#define DEV __device__ __forceinline__

constexpr int SG_V = 13, SG_C = 32, SG_L = 10, SG_OUT = 64, SG_K = SG_C * SG_V;   // joints, channels, blocks, latent, fc K
constexpr int SG_F = 30;                   // output frames per block workgroup (a 32-frame MFMA tile minus the two halo frames)
constexpr int SG_AS = 34;                  // LDS row of one channel's activations: halo slot, 32 tile frames, halo slot
constexpr int SG_WAVES = SG_V;
constexpr int SG_THREADS = 64 * SG_WAVES;
constexpr int SG_FC_WAVES = 4;
constexpr int SG_CHUNK = 64;               // clips per pass (bounds the ping-pong activation planes: 2 x 64 x 416 x T floats)

// device parameter image (floats).  Per block: W1 fragments [16 kk][64 lanes] (lane l = W1'[l & 31][2 kk + (l >> 5)]; block 0
// uses kk = 0 only), W2 fragments [3 tap][16 kk][64], b1' [13 w][32 c], b2' [32], Ahat [13 w][13 v] (+ pad).
constexpr int OFF_W1 = 0, OFF_W2 = OFF_W1 + 16 * 64, OFF_B1 = OFF_W2 + 3 * 16 * 64, OFF_B2 = OFF_B1 + SG_V * SG_C,
              OFF_AH = OFF_B2 + SG_C, BLK_FLOATS = OFF_AH + 176;
constexpr int OFF_DBN = SG_L * BLK_FLOATS;                 // data_bn scale [26] at +0, shift [26] at +32
constexpr int OFF_FCW = OFF_DBN + 64;                      // fc fragments [2 mt][208 ks][64]: lane l = W'[32 mt + (l & 31)][2 ks + (l >> 5)]
constexpr int OFF_FCB = OFF_FCW + 2 * (SG_K / 2) * 64;     // fc bias' [64]
constexpr int PAR_FLOATS = OFF_FCB + SG_OUT;

DEV f32x16 mfma2(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
// torch.relu: NaN stays NaN.  (fmaxf is v_max_f32, which in the kernels' IEEE mode returns the non-NaN operand: max(NaN, 0) = 0.)
DEV float relu(float y) { return y < 0.f ? 0.f : y; }

// One st_gcn block for frames [30 blockIdx.x, +30) of clip blockIdx.y.  FIRST: `in` is the motion [B][T][13][2] and data_bn is
// applied on load; otherwise `in` is the previous block's [B][13][32][T].  out: [B][13][32][T].
template <bool FIRST>
__global__ __launch_bounds__(SG_THREADS) void k_stgcn_block(const float* __restrict__ in, float* __restrict__ out,
                                                            const float* __restrict__ P, const float* __restrict__ dbn, int T) {
    __shared__ float xs[SG_V][SG_C][32];           // block input, slot s = frame f0 - 1 + s
    __shared__ float as[SG_WAVES][SG_C][SG_AS];    // per wave: its joint's activations, slot u = frame f0 - 2 + u
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, f0 = blockIdx.x * SG_F;

    float w2[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) w2[i] = P[OFF_W2 + i * 64 + lane];

    if (FIRST) {
        for (int e = tid; e < SG_V * 2 * 32; e += SG_THREADS) {
            const int s = e & 31, vc = e >> 5, f = f0 - 1 + s;
            xs[vc >> 1][vc & 1][s] = (f >= 0 && f < T) ? fmaf(in[((size_t)b * T + f) * 26 + vc], dbn[vc], dbn[32 + vc]) : 0.f;
        }
    } else {
        const float* src = in + (size_t)b * SG_V * SG_C * T;
        for (int e = tid; e < SG_V * SG_C * 32; e += SG_THREADS) {
            const int s = e & 31, vc = e >> 5, f = f0 - 1 + s;
            xs[vc >> 5][vc & 31][s] = (f >= 0 && f < T) ? src[(size_t)vc * T + f] : 0.f;
        }
    }
    __syncthreads();

    // graph mix of joint w's input (Ahat's zero entries skipped: wave-uniform branches) -> 1x1 conv
    const float* ah = P + OFF_AH + w * SG_V;
    f32x16 acc = {};
    if (FIRST) {
        float bop = 0.f;
        for (int v = 0; v < SG_V; ++v) {
            const float a = ah[v];
            if (a != 0.f) bop = fmaf(a, xs[v][h][j], bop);
        }
        acc = mfma2(P[OFF_W1 + lane], bop, acc);
    } else {
        float bop[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) bop[kk] = 0.f;
        for (int v = 0; v < SG_V; ++v) {
            const float a = ah[v];
            if (a != 0.f) {
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) bop[kk] = fmaf(a, xs[v][2 * kk + h][j], bop[kk]);
            }
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = mfma2(P[OFF_W1 + kk * 64 + lane], bop[kk], acc);
    }

    // + b1', ReLU; frames outside the clip are the temporal conv's zero padding
    const int f = f0 - 1 + j;
    const bool inside = f >= 0 && f < T;
    const float* b1 = P + OFF_B1 + w * SG_C;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float y = acc[r] + b1[c];
        as[w][c][j + 1] = inside ? relu(y) : 0.f;
    }
    if (lane < 32) {
        as[w][lane][0] = 0.f;
        as[w][lane][SG_AS - 1] = 0.f;
    }
    __syncthreads();

    // temporal conv: out column j reads activation columns j - 1, j, j + 1 = slots j, j + 1, j + 2
    f32x16 acc2 = {};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc2 = mfma2(w2[k * 16 + kk], as[w][2 * kk + h][j + k], acc2);

    if (j >= 1 && j <= SG_F && f < T) {
        float* dst = out + (size_t)b * SG_V * SG_C * T + (size_t)w * SG_C * T + f;
        const float* b2 = P + OFF_B2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = (r & 3) + 8 * (r >> 2) + 4 * h;
            float y = acc2[r] + b2[c];
            if (!FIRST) y += xs[w][c][j];
            dst[(size_t)c * T] = relu(y);
        }
    }
}

// fc: Conv1d 416 -> 64 (+ folded BatchNorm1d) on [B][13][32][T] -> latent [B][64][T]; one wave per 32 frames.
__global__ __launch_bounds__(64 * SG_FC_WAVES) void k_stgcn_fc(const float* __restrict__ in, float* __restrict__ out,
                                                               const float* __restrict__ P, int T) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int t0 = (blockIdx.x * SG_FC_WAVES + (threadIdx.x >> 6)) * 32;
    if (t0 >= T) return;                 // wave-uniform; no barriers below
    const int b = blockIdx.y, t = t0 + j;
    const bool tv = t < T;
    const float* src = in + (size_t)b * SG_V * SG_C * T + (tv ? t : 0);
    const float* wf = P + OFF_FCW;
    f32x16 acc0 = {}, acc1 = {};
    for (int ks = 0; ks < SG_K / 2; ++ks) {
        const int k = 2 * ks + h, c = k / SG_V, v = k - c * SG_V;     // fc channel k = c*13 + v
        const float x = tv ? src[(size_t)(v * SG_C + c) * T] : 0.f;
        acc0 = mfma2(wf[ks * 64 + lane], x, acc0);
        acc1 = mfma2(wf[(SG_K / 2 + ks) * 64 + lane], x, acc1);
    }
    if (!tv) return;
    float* dst = out + (size_t)b * SG_OUT * T + t;
    const float* bf = P + OFF_FCB;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = (r & 3) + 8 * (r >> 2) + 4 * h;
        dst[(size_t)o * T] = acc0[r] + bf[o];
        dst[(size_t)(o + 32) * T] = acc1[r] + bf[o + 32];
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------

struct Spec {
    size_t numel;
    bool used;        // read by the encoder (st_gcn.fcn.* and num_batches_tracked are state_dict entries it never applies)
};

const std::map<std::string, Spec>& param_table() {
    static const std::map<std::string, Spec> tab = [] {
        std::map<std::string, Spec> t;
        auto bn = [&](const std::string& p, size_t n) {
            for (const char* s : {"weight", "bias", "running_mean", "running_var"}) t[p + s] = {n, true};
            t[p + "num_batches_tracked"] = {1, false};
        };
        t["st_gcn.A"] = {SG_V * SG_V, true};
        bn("st_gcn.data_bn.", 2 * SG_V);
        for (int l = 0; l < SG_L; ++l) {
            const std::string p = "st_gcn.st_gcn_networks." + std::to_string(l) + ".";
            t[p + "gcn.conv.weight"] = {(size_t)SG_C * (l == 0 ? 2 : SG_C), true};
            t[p + "gcn.conv.bias"] = {SG_C, true};
            bn(p + "tcn.0.", SG_C);
            t[p + "tcn.2.weight"] = {SG_C * SG_C * 3, true};
            t[p + "tcn.2.bias"] = {SG_C, true};
            bn(p + "tcn.3.", SG_C);
            t["st_gcn.edge_importance." + std::to_string(l)] = {SG_V * SG_V, true};
        }
        t["st_gcn.fcn.weight"] = {32 * 256, false};
        t["st_gcn.fcn.bias"] = {32, false};
        t["fc.0.weight"] = {SG_OUT * SG_K, true};
        t["fc.0.bias"] = {SG_OUT, true};
        bn("fc.1.", SG_OUT);
        return t;
    }();
    return tab;
}

// eval-mode BatchNorm as y = s x + h
void bn_affine(const std::map<std::string, std::vector<float>>& P, const std::string& p, size_t n, std::vector<double>& s,
               std::vector<double>& h) {
    const auto &g = P.at(p + "weight"), &be = P.at(p + "bias"), &rm = P.at(p + "running_mean"), &rv = P.at(p + "running_var");
    s.resize(n);
    h.resize(n);
    for (size_t i = 0; i < n; ++i) {
        s[i] = (double)g[i] / std::sqrt((double)rv[i] + 1e-5);
        h[i] = (double)be[i] - (double)rm[i] * s[i];
    }
}

std::vector<float> fold(const std::map<std::string, std::vector<float>>& P) {
    std::vector<float> img(PAR_FLOATS, 0.f);
    const auto& A = P.at("st_gcn.A");
    std::vector<double> s0, h0, s3, h3;
    for (int l = 0; l < SG_L; ++l) {
        const std::string p = "st_gcn.st_gcn_networks." + std::to_string(l) + ".";
        const int cin = l == 0 ? 2 : SG_C;
        float* blk = img.data() + (size_t)l * BLK_FLOATS;
        const auto& E = P.at("st_gcn.edge_importance." + std::to_string(l));
        const auto &W1 = P.at(p + "gcn.conv.weight"), &bb1 = P.at(p + "gcn.conv.bias");
        const auto &W2 = P.at(p + "tcn.2.weight"), &bb2 = P.at(p + "tcn.2.bias");
        bn_affine(P, p + "tcn.0.", SG_C, s0, h0);
        bn_affine(P, p + "tcn.3.", SG_C, s3, h3);
        double colsum[SG_V];
        for (int w = 0; w < SG_V; ++w) {
            colsum[w] = 0.0;
            for (int v = 0; v < SG_V; ++v) {
                const float a = A[v * SG_V + w] * E[v * SG_V + w];      // the reference's A * importance, in fp32
                blk[OFF_AH + w * SG_V + v] = a;
                colsum[w] += a;
            }
        }
        for (int lane = 0; lane < 64; ++lane) {
            const int c = lane & 31, hh = lane >> 5;
            for (int kk = 0; kk < (l == 0 ? 1 : 16); ++kk) {
                const int ci = 2 * kk + hh;
                blk[OFF_W1 + kk * 64 + lane] = (float)(s0[c] * W1[c * cin + ci]);
            }
            for (int k = 0; k < 3; ++k)
                for (int kk = 0; kk < 16; ++kk) {
                    const int ci = 2 * kk + hh;     // tcn.2.weight [c][ci][k][0]
                    blk[OFF_W2 + (k * 16 + kk) * 64 + lane] = (float)(s3[c] * W2[(c * SG_C + ci) * 3 + k]);
                }
        }
        for (int w = 0; w < SG_V; ++w)
            for (int c = 0; c < SG_C; ++c) blk[OFF_B1 + w * SG_C + c] = (float)(s0[c] * bb1[c] * colsum[w] + h0[c]);
        for (int c = 0; c < SG_C; ++c) blk[OFF_B2 + c] = (float)(s3[c] * bb2[c] + h3[c]);
    }
    std::vector<double> sd, hd, sf, hf;
    bn_affine(P, "st_gcn.data_bn.", 2 * SG_V, sd, hd);
    for (int i = 0; i < 2 * SG_V; ++i) {
        img[OFF_DBN + i] = (float)sd[i];
        img[OFF_DBN + 32 + i] = (float)hd[i];
    }
    bn_affine(P, "fc.1.", SG_OUT, sf, hf);
    const auto &Wf = P.at("fc.0.weight"), &bf = P.at("fc.0.bias");
    for (int mt = 0; mt < 2; ++mt)
        for (int ks = 0; ks < SG_K / 2; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int o = 32 * mt + (lane & 31), k = 2 * ks + (lane >> 5);
                img[OFF_FCW + ((size_t)mt * (SG_K / 2) + ks) * 64 + lane] = (float)(sf[o] * Wf[(size_t)o * SG_K + k]);
            }
    for (int o = 0; o < SG_OUT; ++o) img[OFF_FCB + o] = (float)(sf[o] * bf[o] + hf[o]);
    return img;
}

#define SG_TRY(expr)                                                                                                  \
    do {                                                                                                              \
        hipError_t e_ = (expr);                                                                                       \
        if (e_ != hipSuccess) return dc_set_error(DC_ERR_HIP, (std::string(#expr) + " failed: " + hipGetErrorString(e_)).c_str()); \
    } while (0)

}  // namespace

struct dc_motion_encoder {
    int device = 0;
    std::map<std::string, std::vector<float>> params;
    float* d_par = nullptr;
    float* d_ws = nullptr;
    size_t ws_floats = 0;
};

extern "C" {

int dc_motion_encoder_create(int32_t device, dc_motion_encoder** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return dc_set_error(DC_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_create: bad device ordinal");
    auto* e = new dc_motion_encoder;
    e->device = device;
    *out = e;
    return DC_OK;
}

void dc_motion_encoder_destroy(dc_motion_encoder* e) {
    if (!e) return;
    hipSetDevice(e->device);
    if (e->d_par) hipFree(e->d_par);
    if (e->d_ws) hipFree(e->d_ws);
    delete e;
}

int dc_motion_encoder_set_param(dc_motion_encoder* e, const char* name, const float* h_data, int64_t numel) {
    if (!e || !name || !h_data) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_set_param: NULL argument");
    const auto& tab = param_table();
    auto it = tab.find(name);
    if (it == tab.end()) return dc_set_error(DC_ERR_PARAM, (std::string("unknown motion encoder parameter ") + name).c_str());
    if (numel != (int64_t)it->second.numel)
        return dc_set_error(DC_ERR_PARAM, (std::string("motion encoder parameter ") + name + " has " + std::to_string(numel) +
                                           " elements, expected " + std::to_string(it->second.numel)).c_str());
    if (it->second.used) e->params[name].assign(h_data, h_data + numel);
    return DC_OK;
}

int dc_motion_encoder_finalize(dc_motion_encoder* e) {
    if (!e) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_finalize: NULL encoder");
    for (const auto& kv : param_table())
        if (kv.second.used && !e->params.count(kv.first))
            return dc_set_error(DC_ERR_PARAM, ("motion encoder parameter " + kv.first + " was not set").c_str());
    const std::vector<float> img = fold(e->params);
    SG_TRY(hipSetDevice(e->device));
    if (!e->d_par) SG_TRY(hipMalloc((void**)&e->d_par, img.size() * sizeof(float)));
    SG_TRY(hipMemcpy(e->d_par, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    return DC_OK;
}

int dc_motion_encoder_encode(dc_motion_encoder* e, const float* d_motion, int32_t B, int32_t T, float* d_out, void* stream) {
    if (!e || !d_motion || !d_out) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_encode: NULL argument");
    if (!e->d_par) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_encode before dc_motion_encoder_finalize");
    if (B < 1 || T < 1) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_encode: B and T must be >= 1");
    SG_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < SG_CHUNK ? B : SG_CHUNK;
    const size_t plane = (size_t)chunk * SG_K * T;
    if (e->ws_floats < 2 * plane) {
        if (e->d_ws) {
            SG_TRY(hipStreamSynchronize(st));    // (the previous call's work on this stream may still read the old planes)
            SG_TRY(hipFree(e->d_ws));
            e->d_ws = nullptr;
            e->ws_floats = 0;
        }
        SG_TRY(hipMalloc((void**)&e->d_ws, 2 * plane * sizeof(float)));
        e->ws_floats = 2 * plane;
    }
    float* buf[2] = {e->d_ws, e->d_ws + plane};
    const float* P = e->d_par;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = B - b0 < chunk ? B - b0 : chunk;
        const dim3 gb((T + SG_F - 1) / SG_F, nb);
        k_stgcn_block<true><<<gb, SG_THREADS, 0, st>>>(d_motion + (size_t)b0 * T * 2 * SG_V, buf[0], P, P + OFF_DBN, T);
        for (int l = 1; l < SG_L; ++l)
            k_stgcn_block<false><<<gb, SG_THREADS, 0, st>>>(buf[(l - 1) & 1], buf[l & 1], P + (size_t)l * BLK_FLOATS, nullptr, T);
        const dim3 gf(((T + 31) / 32 + SG_FC_WAVES - 1) / SG_FC_WAVES, nb);
        k_stgcn_fc<<<gf, 64 * SG_FC_WAVES, 0, st>>>(buf[(SG_L - 1) & 1], d_out + (size_t)b0 * SG_OUT * T, P, T);
        SG_TRY(hipGetLastError());
    }
    return DC_OK;
}

}  // extern "C"
