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
// Folding (host, fp64, at finalize: dc_pack.h, stgcn_pack).  BN0 follows the graph mix, which is linear over joints, so it folds
// into the 1x1 conv:
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

#include <string>
#include <vector>

#include "dc_common.h"
#include "dc_handle.h"
#include "dc_mfma_f32.h"

namespace {

using namespace dc_f32;

constexpr int SG_F = 30;                   // output frames per block workgroup (a 32-frame MFMA tile minus the two halo frames)
constexpr int SG_AS = 34;                  // LDS row of one channel's activations: halo slot, 32 tile frames, halo slot
constexpr int SG_WAVES = kStgcnV;
constexpr int SG_THREADS = 64 * SG_WAVES;
constexpr int SG_FC_WAVES = 4;
constexpr int SG_CHUNK = 64;               // clips per pass (bounds the ping-pong activation planes: 2 x 64 x 416 x T floats)

// One st_gcn block for frames [30 blockIdx.x, +30) of clip blockIdx.y.  FIRST: `in` is the motion [B][T][13][2] and data_bn is
// applied on load; otherwise `in` is the previous block's [B][13][32][T].  out: [B][13][32][T].  P: the block's part of the image.
template <bool FIRST>
__global__ __launch_bounds__(SG_THREADS) void k_stgcn_block(const float* __restrict__ in, float* __restrict__ out,
                                                            const float* __restrict__ P, const float* __restrict__ dbn, int T) {
    __shared__ float xs[kStgcnV][kStgcnC][32];     // block input, slot s = frame f0 - 1 + s
    __shared__ float as[SG_WAVES][kStgcnC][SG_AS]; // per wave: its joint's activations, slot u = frame f0 - 2 + u
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, f0 = blockIdx.x * SG_F;

    float w2[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) w2[i] = P[kStgcnW2 + i * 64 + lane];

    if (FIRST) {
        for (int e = tid; e < kStgcnV * 2 * 32; e += SG_THREADS) {
            const int s = e & 31, vc = e >> 5, f = f0 - 1 + s;
            xs[vc >> 1][vc & 1][s] = (f >= 0 && f < T) ? fmaf(in[((size_t)b * T + f) * 26 + vc], dbn[vc], dbn[32 + vc]) : 0.f;
        }
    } else {
        const float* src = in + (size_t)b * kStgcnK * T;
        for (int e = tid; e < kStgcnK * 32; e += SG_THREADS) {
            const int s = e & 31, vc = e >> 5, f = f0 - 1 + s;
            xs[vc >> 5][vc & 31][s] = (f >= 0 && f < T) ? src[(size_t)vc * T + f] : 0.f;
        }
    }
    __syncthreads();

    // graph mix of joint w's input (Ahat's zero entries skipped: wave-uniform branches) -> 1x1 conv
    const float* ah = P + kStgcnAhat + w * kStgcnV;
    f32x16 acc = {};
    if (FIRST) {
        float bop = 0.f;
        for (int v = 0; v < kStgcnV; ++v) {
            const float a = ah[v];
            if (a != 0.f) bop = fmaf(a, xs[v][h][j], bop);
        }
        acc = mfma2(P[kStgcnW1 + lane], bop, acc);
    } else {
        float bop[16];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) bop[kk] = 0.f;
        for (int v = 0; v < kStgcnV; ++v) {
            const float a = ah[v];
            if (a != 0.f) {
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) bop[kk] = fmaf(a, xs[v][2 * kk + h][j], bop[kk]);
            }
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) acc = mfma2(P[kStgcnW1 + kk * 64 + lane], bop[kk], acc);
    }

    // + b1', ReLU; frames outside the clip are the temporal conv's zero padding
    const int f = f0 - 1 + j;
    const bool inside = f >= 0 && f < T;
    const float* b1 = P + kStgcnB1 + w * kStgcnC;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = tile_channel(r, h);
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
        float* dst = out + (size_t)b * kStgcnK * T + (size_t)w * kStgcnC * T + f;
        const float* b2 = P + kStgcnB2;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = tile_channel(r, h);
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
    const float* src = in + (size_t)b * kStgcnK * T + (tv ? t : 0);
    const float* wf = P + kStgcnFcW;
    f32x16 acc0 = {}, acc1 = {};
    for (int ks = 0; ks < kStgcnK / 2; ++ks) {
        const int k = 2 * ks + h, c = k / kStgcnV, v = k - c * kStgcnV;     // fc channel k = c*13 + v
        const float x = tv ? src[(size_t)(v * kStgcnC + c) * T] : 0.f;
        acc0 = mfma2(wf[ks * 64 + lane], x, acc0);
        acc1 = mfma2(wf[(kStgcnK / 2 + ks) * 64 + lane], x, acc1);
    }
    if (!tv) return;
    add_bias<false>(acc0, acc1, P + kStgcnFcB, h);
    float* dst = out + (size_t)b * kStgcnOut * T + t;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = tile_channel(r, h);
        dst[(size_t)o * T] = acc0[r];
        dst[(size_t)(o + 32) * T] = acc1[r];
    }
}

const char* const kWhat = "motion encoder";
const DcParamList& required() {
    static const DcParamList r = stgcn_required();
    return r;
}

}  // namespace

struct dc_motion_encoder {
    int device = 0;
    DcParams params;
    float* d_par = nullptr;
    DcWorkspace ws;                      // two ping-pong planes [chunk][13][32][T]
};

extern "C" {

int dc_motion_encoder_create(int32_t device, dc_motion_encoder** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_create: out is NULL");
    *out = nullptr;
    if (const int rc = dc_check_device("dc_motion_encoder_create", device)) return rc;
    auto* e = new dc_motion_encoder;
    e->device = device;
    *out = e;
    return DC_OK;
}

void dc_motion_encoder_destroy(dc_motion_encoder* e) {
    if (!e) return;
    const DcDeviceGuard on(e->device);
    if (e->d_par) (void)hipFree(e->d_par);
    e->ws.release();
    delete e;
}

int dc_motion_encoder_set_param(dc_motion_encoder* e, const char* name, const float* h_data, int64_t numel) {
    if (!e || !name || !h_data) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_set_param: NULL argument");
    return dc_param_take(kWhat, required(), stgcn_ignored(), name, name, h_data, numel, &e->params);
}

int dc_motion_encoder_finalize(dc_motion_encoder* e) {
    if (!e) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_finalize: NULL encoder");
    if (const int rc = dc_param_complete(kWhat, required(), e->params)) return rc;
    const std::vector<float> img = stgcn_pack(e->params);
    DC_HIP_TRY(hipSetDevice(e->device));
    if (!e->d_par) DC_HIP_TRY(hipMalloc((void**)&e->d_par, img.size() * sizeof(float)));
    DC_HIP_TRY(hipMemcpy(e->d_par, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    return DC_OK;
}

int dc_motion_encoder_encode(dc_motion_encoder* e, const float* d_motion, int32_t B, int32_t T, float* d_out, void* stream) {
    if (!e || !d_motion || !d_out) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_encode: NULL argument");
    if (!e->d_par) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_encode before dc_motion_encoder_finalize");
    if (B < 1 || T < 1) return dc_set_error(DC_ERR_INVALID, "dc_motion_encoder_encode: B and T must be >= 1");
    DC_HIP_TRY(hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const int chunk = B < SG_CHUNK ? B : SG_CHUNK;
    const size_t plane = (size_t)chunk * kStgcnK * T;
    if (const int rc = e->ws.reserve(2 * plane, st)) return rc;
    float* buf[2] = {e->ws.p, e->ws.p + plane};
    const float* P = e->d_par;
    return dc_chunks(B, chunk, [&](int b0, int nb) -> int {
        const dim3 gb((T + SG_F - 1) / SG_F, nb);
        k_stgcn_block<true><<<gb, SG_THREADS, 0, st>>>(d_motion + (size_t)b0 * T * 2 * kStgcnV, buf[0], P, P + kStgcnDbn, T);
        for (int l = 1; l < kStgcnL; ++l)
            k_stgcn_block<false><<<gb, SG_THREADS, 0, st>>>(buf[(l - 1) & 1], buf[l & 1], P + (size_t)l * kStgcnBlockFloats, nullptr, T);
        const dim3 gf(((T + 31) / 32 + SG_FC_WAVES - 1) / SG_FC_WAVES, nb);
        k_stgcn_fc<<<gf, 64 * SG_FC_WAVES, 0, st>>>(buf[(kStgcnL - 1) & 1], d_out + (size_t)b0 * kStgcnOut * T, P, T);
        DC_HIP_TRY(hipGetLastError());
        return DC_OK;
    });
}

}  // extern "C"
