// dc_loss.hip - the forward value of the denoising objective (include/dc_ddim.h, "Held-out denoising losses"): the forward noising
// q_sample and the per-clip reductions of GaussianDiffusion.training_losses / DDPMTrainer.backward_G.  Three small bandwidth-bound
// kernels of their own; nothing here is on the sampling path.
//
// Reductions: ONE workgroup of DC_LOSS_THREADS threads per clip.  A thread walks its clip in strides of DC_LOSS_THREADS vector
// elements and keeps one fp32 partial per term (a serial chain of additions); the 256 partials are combined in a fixed tree - six
// butterfly levels inside each wave, then (w0 + w1) + (w2 + w3) over the four waves.  No atomics: a rerun is bit-identical, and a
// clip's numbers do not depend on the batch around it.
//
// What a test may assume about the rounding (tests/test_gpu_losses.py states the same constants):
//   motion terms  vector element = 2 floats (one float2; 26 is even, so a pair never leaves its frame or its channel group);
//                 longest chain = ceil(13 T / 256) additions + 1 (the pair's own sum);  tree depth 8
//   latent L1     vector element = 4 floats;  longest chain = ceil(16 T / 256) + 2 (the quad's own tree);  tree depth 8
// Every difference is taken in fp64 and rounded ONCE to fp32 after squaring (or after fabs), so a term whose differences cancel
// (slot 5: target velocity minus predicted velocity) carries one rounding per element like the others; one more for the final
// division.  relative error <= (chain + depth + 3) * 2^-24 for sums of non-negative terms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "dc_common.h"
#include "dc_handle.h"
#include "dc_launch.h"

// No contraction anywhere in this file: hipcc's default (-ffp-contract=fast) fuses a product into the addition that consumes it.
// HIP's __fmul_rn / __fadd_rn do not prevent that - they are inline functions of plain operators compiled under the default, and
// came out of k_q_sample as one v_pk_fma_f32 - so the arithmetic below is written with plain operators under this pragma: every
// product and every sum is rounded on its own, in the order written.
#pragma clang fp contract(off)

#define DC_LOSS_THREADS 256
#define DC_LOSS_CHUNK 64        // clips per launch: their per-clip host scalars travel BY VALUE in the kernel arguments (no copy, no
                                // allocation, nothing for a stream capture to trip over)

namespace {

struct ClipScalars {
    float a[DC_LOSS_CHUNK], s[DC_LOSS_CHUNK];
};
struct ClipLengths {
    int len[DC_LOSS_CHUNK];
};

// x_t = a_b x0 + s_b noise (gaussian_diffusion.py:398-416): two rounded products and one rounded sum, never contracted - the bits
// of the reference's fp32 tensor expression.  blockIdx.y = clip of this chunk.  `noise` may alias `xt` (the seeded path without
// d_noise_out draws into xt first): every thread reads its elements before it writes them.
template <bool VEC>
__global__ __launch_bounds__(256) void k_q_sample(const float* __restrict__ x0, const float* noise, float* xt, size_t per_clip,
                                                  ClipScalars cs) {
    const float a = cs.a[blockIdx.y], s = cs.s[blockIdx.y];
    const size_t base = (size_t)blockIdx.y * per_clip;
    if (VEC) {
        const size_t nv = per_clip >> 2;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (size_t)gridDim.x * 256) {
            const float4 x = reinterpret_cast<const float4*>(x0 + base)[i];
            const float4 z = reinterpret_cast<const float4*>(noise + base)[i];
            float4 o;
            o.x = a * x.x + s * z.x;
            o.y = a * x.y + s * z.y;
            o.z = a * x.z + s * z.z;
            o.w = a * x.w + s * z.w;
            reinterpret_cast<float4*>(xt + base)[i] = o;
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per_clip; i += (size_t)gridDim.x * 256)
            xt[base + i] = a * x0[base + i] + s * noise[base + i];
    }
}

// the fixed tree: butterflies over the wave's 64 lanes (every lane ends with the wave's sum), then the four waves
template <int N>
__device__ void block_tree(float (&v)[N], float (*lds)[N]) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = (v[k] + __shfl_xor(v[k], off, 64));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) lds[w][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (lds[0][k] + lds[1][k]) + (lds[2][k] + lds[3][k]);
}

__device__ __forceinline__ float sq1(double d) { return (float)(d * d); }      // exact difference in, ONE rounding out

// One workgroup per clip (blockIdx.x = clip of this chunk).  pred / target [B][T][26]; terms [B][DC_LOSS_TERMS].
__global__ __launch_bounds__(DC_LOSS_THREADS) void k_motion_loss_terms(const float* __restrict__ pred, const float* __restrict__ target,
                                                                       float* __restrict__ terms, int T, ClipLengths cl) {
    __shared__ float lds[4][6];
    const int len = cl.len[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * T * 26;
    const float2* p2 = reinterpret_cast<const float2*>(pred + base);
    const float2* t2 = reinterpret_cast<const float2*>(target + base);
    const int npair = T * 13;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // mse, rec, body, elbow, head, velocity
#pragma unroll 4
    for (int i = threadIdx.x; i < npair; i += DC_LOSS_THREADS) {
        const int t = i / 13, c = 2 * (i - 13 * t);      // frame, first channel of the pair
        const float2 p = p2[i], g = t2[i];
        const float d2 = (sq1((double)g.x - (double)p.x) + sq1((double)g.y - (double)p.y));
        acc[0] = (acc[0] + d2);
        if (t < len) acc[1] = (acc[1] + d2);
        if (t + 1 < T) {
            const float2 pn = p2[i + 13], gn = t2[i + 13];
            const double vpx = (double)pn.x - (double)p.x, vpy = (double)pn.y - (double)p.y;
            const float v2 = (sq1(vpx) + sq1(vpy));
            const int slot = c < 10 ? 4 : (c < 14 || c >= 22) ? 2 : 3;      // head 0..9, body 10..13 and 22..25, elbow 14..21
            acc[slot] = (acc[slot] + v2);
            const double vtx = (double)gn.x - (double)g.x, vty = (double)gn.y - (double)g.y;
            acc[5] = acc[5] + (sq1(vtx - vpx) + sq1(vty - vpy));
        }
    }
    block_tree<6>(acc, lds);
    if (threadIdx.x == 0) {
        float* o = terms + (size_t)blockIdx.x * DC_LOSS_TERMS;
        const float nv = (float)(T - 1);
        o[0] = acc[0] / (float)(T * 26);
        o[1] = acc[1] / 26.0f;
        o[2] = acc[2] / (nv * 8.0f);
        o[3] = acc[3] / (nv * 8.0f);
        o[4] = acc[4] / (nv * 10.0f);
        o[5] = acc[5] / (nv * 26.0f);
        o[6] = 0.f;
        o[7] = 0.f;
    }
}

// One workgroup per clip: mean |a - b| over the clip's [64][T] latent.
__global__ __launch_bounds__(DC_LOSS_THREADS) void k_latent_l1(const float* __restrict__ a, const float* __restrict__ b,
                                                               float* __restrict__ out, int T) {
    __shared__ float lds[4][1];
    const size_t base = (size_t)blockIdx.x * 64 * T;
    const float4* a4 = reinterpret_cast<const float4*>(a + base);
    const float4* b4 = reinterpret_cast<const float4*>(b + base);
    const int nquad = 16 * T;
    float acc[1] = {0.f};
#pragma unroll 4
    for (int i = threadIdx.x; i < nquad; i += DC_LOSS_THREADS) {
        const float4 x = a4[i], y = b4[i];
        const float q = (fabsf(x.x - y.x) + fabsf(x.y - y.y)) + (fabsf(x.z - y.z) + fabsf(x.w - y.w));
        acc[0] = (acc[0] + q);
    }
    block_tree<1>(acc, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = acc[0] / (float)(64 * T);
}

inline bool aligned(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace

extern "C" {

int dc_q_sample_coefficients(int32_t n_train, const double* h_alphas_cumprod, const int32_t* h_timesteps, int32_t B, float* h_a,
                             float* h_s) {
    if (!h_alphas_cumprod || !h_timesteps || !h_a || !h_s) return dc_set_error(DC_ERR_INVALID, "dc_q_sample_coefficients: NULL argument");
    if (n_train < 1 || B < 1) return dc_set_error(DC_ERR_INVALID, "dc_q_sample_coefficients: n_train and B must be >= 1");
    for (int32_t b = 0; b < B; ++b)
        if (h_timesteps[b] < 0 || h_timesteps[b] >= n_train)
            return dc_set_error(DC_ERR_INVALID, ("dc_q_sample_coefficients: timestep " + std::to_string(h_timesteps[b]) + " of clip " +
                                                 std::to_string(b) + " is outside [0, " + std::to_string(n_train) + ")").c_str());
    for (int32_t b = 0; b < B; ++b) {
        const double ab = h_alphas_cumprod[h_timesteps[b]];
        h_a[b] = (float)std::sqrt(ab);
        h_s[b] = (float)std::sqrt(1.0 - ab);
    }
    return DC_OK;
}

int dc_q_sample(const float* d_x0, const float* d_noise, const float* h_a, const float* h_s, int32_t B, int32_t T, int32_t P, uint64_t seed,
                int32_t iteration, uint64_t first_element, float* d_noise_out, float* d_xt, void* stream) {
    if (!d_x0 || !d_xt || !h_a || !h_s) return dc_set_error(DC_ERR_INVALID, "dc_q_sample: NULL argument");
    if (B < 1 || T < 1 || P < 1) return dc_set_error(DC_ERR_INVALID, "dc_q_sample: B, T and P must be >= 1");
    if (d_noise && d_noise_out) return dc_set_error(DC_ERR_INVALID, "dc_q_sample: d_noise_out receives the library's own draws (d_noise must be NULL)");
    if (!d_noise && iteration < 0) return dc_set_error(DC_ERR_INVALID, "dc_q_sample: iteration must be >= 0");
    if (d_xt == d_x0 || d_noise_out == d_x0 || (d_noise_out && d_noise_out == d_xt))
        return dc_set_error(DC_ERR_INVALID, "dc_q_sample: d_xt and d_noise_out must be buffers of their own");
    hipStream_t st = (hipStream_t)stream;
    const size_t per_clip = (size_t)T * P;
    const float* nz = d_noise;
    if (!nz) {
        // the draws of dc_step_noise_fill, by the same kernel; without d_noise_out they land in d_xt and are replaced in place
        float* buf = d_noise_out ? d_noise_out : d_xt;
        DC_HIP_TRY(dc_launch_step_noise(st, buf, (size_t)B * per_clip, seed, nullptr, nullptr, iteration, nullptr, first_element));
        nz = buf;
    }
    const bool vec = (per_clip & 3) == 0 && aligned(d_x0, 16) && aligned(nz, 16) && aligned(d_xt, 16);
    const size_t work = vec ? per_clip >> 2 : per_clip;
    const unsigned gx = (unsigned)std::min<size_t>((work + 255) / 256, 1024);
    for (int32_t b0 = 0; b0 < B; b0 += DC_LOSS_CHUNK) {
        const int nb = std::min<int32_t>(DC_LOSS_CHUNK, B - b0);
        ClipScalars cs;
        for (int i = 0; i < DC_LOSS_CHUNK; ++i) cs.a[i] = i < nb ? h_a[b0 + i] : 0.f, cs.s[i] = i < nb ? h_s[b0 + i] : 0.f;
        const size_t off = (size_t)b0 * per_clip;
        if (vec)
            k_q_sample<true><<<dim3(gx ? gx : 1, nb), dim3(256), 0, st>>>(d_x0 + off, nz + off, d_xt + off, per_clip, cs);
        else
            k_q_sample<false><<<dim3(gx ? gx : 1, nb), dim3(256), 0, st>>>(d_x0 + off, nz + off, d_xt + off, per_clip, cs);
        DC_HIP_TRY(hipGetLastError());
    }
    return DC_OK;
}

int dc_motion_loss_terms(const float* d_pred, const float* d_target, const int32_t* h_length, int32_t B, int32_t T, int32_t P,
                         float* d_terms, void* stream) {
    if (!d_pred || !d_target || !d_terms) return dc_set_error(DC_ERR_INVALID, "dc_motion_loss_terms: NULL argument");
    if (P != 26) return dc_set_error(DC_ERR_INVALID, "dc_motion_loss_terms: the channel groups are those of 13 joints x 2 (P must be 26)");
    if (B < 1) return dc_set_error(DC_ERR_INVALID, "dc_motion_loss_terms: B must be >= 1");
    if (T < 2) return dc_set_error(DC_ERR_INVALID, "dc_motion_loss_terms: T must be >= 2 (the velocity means run over T - 1 frames; the reference returns NaN at T = 1)");
    if ((int64_t)T * 13 > INT32_MAX) return dc_set_error(DC_ERR_INVALID, "dc_motion_loss_terms: T is too large");
    if (h_length)
        for (int32_t b = 0; b < B; ++b)
            if (h_length[b] < 1 || h_length[b] > T)
                return dc_set_error(DC_ERR_INVALID, ("dc_motion_loss_terms: length " + std::to_string(h_length[b]) + " of clip " +
                                                     std::to_string(b) + " is outside [1, " + std::to_string(T) + "]").c_str());
    if (!aligned(d_pred, 8) || !aligned(d_target, 8)) return dc_set_error(DC_ERR_INVALID, "dc_motion_loss_terms: the tensors must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    for (int32_t b0 = 0; b0 < B; b0 += DC_LOSS_CHUNK) {
        const int nb = std::min<int32_t>(DC_LOSS_CHUNK, B - b0);
        ClipLengths cl;
        for (int i = 0; i < DC_LOSS_CHUNK; ++i) cl.len[i] = i < nb ? (h_length ? h_length[b0 + i] : T) : 0;
        const size_t off = (size_t)b0 * T * 26;
        k_motion_loss_terms<<<dim3(nb), dim3(DC_LOSS_THREADS), 0, st>>>(d_pred + off, d_target + off, d_terms + (size_t)b0 * DC_LOSS_TERMS, T, cl);
        DC_HIP_TRY(hipGetLastError());
    }
    return DC_OK;
}

int dc_latent_l1(const float* d_a, const float* d_b, int32_t B, int32_t T, float* d_out, void* stream) {
    if (!d_a || !d_b || !d_out) return dc_set_error(DC_ERR_INVALID, "dc_latent_l1: NULL argument");
    if (B < 1 || T < 1) return dc_set_error(DC_ERR_INVALID, "dc_latent_l1: B and T must be >= 1");
    if ((int64_t)T * 16 > INT32_MAX) return dc_set_error(DC_ERR_INVALID, "dc_latent_l1: T is too large");
    if (!aligned(d_a, 16) || !aligned(d_b, 16)) return dc_set_error(DC_ERR_INVALID, "dc_latent_l1: the latents must be 16-byte aligned");
    k_latent_l1<<<dim3(B), dim3(DC_LOSS_THREADS), 0, (hipStream_t)stream>>>(d_a, d_b, d_out, T);
    DC_HIP_TRY(hipGetLastError());
    return DC_OK;
}

}  // extern "C"
