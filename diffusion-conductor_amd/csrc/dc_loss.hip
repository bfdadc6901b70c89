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
//
// The variational bound (dc_vb_terms, dc_prior_kl; include/dc_ddim.h, "The variational bound").  An element costs about 150
// instructions (two tanhf, three logf, three expf), so ONE workgroup per clip is too few: a clip of n = T P elements is cut into
// G = min(DC_VB_MAX_GROUPS = 32, ceil(ceil(n / 2) / DC_VB_SPAN = 2048)) contiguous ranges of per = ceil(ceil(n / 2) / G) pairs - a
// function of the clip's size only, never of the batch - one workgroup each, reduced with the same chain and tree to DC_VB_SUMS = 4
// partial sums (kl, decoder nll, x0 error, epsilon error; slot 0 of the result is one of the first two, so a fifth partial would
// repeat one); a second launch adds a clip's G partials in index order, divides and writes the slots.  No atomics.
//   vector element = 2 floats (float2 when n is even and the pointers are 8-byte aligned, else two scalar loads of the same pair: the
//                    order of additions is the same; an odd n leaves the last pair with one element)
//   longest chain  = ceil(per / 256) additions + 1 (the pair's own sum) + (G - 1) (the combine);  tree depth 8
//   dc_prior_kl    = one workgroup per clip: chain ceil(ceil(n / 2) / 256) + 1, tree depth 8
// The per-element arithmetic is the reference's fp32 expressions in the reference's order (nothing is taken in fp64 here: where fp32
// tanh saturates, cdf_delta is 0 and the clamp gives log 1e-12, and that is the reference's number).  Roundings on an element's path,
// each at most 2^-24 of its result, an expf / logf / tanhf counted as 2 (HIP documents 1 ULP = 2 x 2^-24 for each), BEHIND the two
// means and pred_xstart (affine fp32 expressions whose bits a test reproduces exactly):
//   log-variance of LEARNED_RANGE 5;  kl: m1 - m2, its square, exp(-lv2), their product, lv1 - lv2, exp, three sums = 12 -> 17
//   nll: x0 - mean 1, exp(-log_scale) 2, then per cdf +-1/255, the product, the cube 2, its scale, two sums, the 0.79 scale, tanh 2,
//        1 + tanh = 11, twice; cdf_plus - cdf_min 1 (or 1 - cdf_min), log 2 -> 5 + 3 + 22 + 3 = 33 at most, 28 with a fixed variance
//   DC_VB_K = 32 is what tests/test_gpu_vb.py uses for both (the learned-range log-variance and the two cdfs share roundings)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

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
#define DC_VB_SUMS 4            // partial sums per workgroup of dc_vb_terms
#define DC_VB_SPAN 2048         // pairs per workgroup before a clip is cut further
#define DC_VB_MAX_GROUPS 32     // workgroups per clip at most

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

// ---- the variational bound (include/dc_ddim.h, "The variational bound") -------------------------------------------------------------
struct VbScalars {      // per clip of a chunk, BY VALUE like ClipScalars: 8 x 256 B
    float c1[DC_LOSS_CHUNK], c2[DC_LOSS_CHUNK], lv1[DC_LOSS_CHUNK], lvm[DC_LOSS_CHUNK], rc[DC_LOSS_CHUNK], rm1[DC_LOSS_CHUNK],
        r1[DC_LOSS_CHUNK], r21[DC_LOSS_CHUNK];
};
struct VbFlags {
    int t0[DC_LOSS_CHUNK];
};
struct VbClip {
    float c1, c2, lv1, lvm, rc, rm1, r1, r21;
};

// th.clamp keeps a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp_min(float v, float lo) { return v < lo ? lo : v; }

// approx_standard_normal_cdf (gaussian_diffusion.py:191-196): 0.5 (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))), th.pow(x, 3) = (x x) x
__device__ __forceinline__ float vb_cdf(float x) {
    const float kS = (float)0.79788456080286535588;      // (float)np.sqrt(2.0 / np.pi)
    return 0.5f * (1.0f + tanhf(kS * (x + 0.044715f * ((x * x) * x))));
}

// One element of _vb_terms_bpd (gaussian_diffusion.py:967-1000) behind p_mean_variance (:442-536), and of the two errors calc_bpd_loop
// adds (:1149-1151): the reference's fp32 expressions in the reference's order.  Adds to e[0..3] = kl, decoder nll (nats), (pred_xstart -
// x0)^2, (eps - noise)^2.  The branches are uniform over the launch.
__device__ __forceinline__ void vb_element(float x0, float xt, float mo, float vv, float nz, const VbClip& c, int mean_type, int var_type,
                                           bool clip, bool has_noise, float (&e)[DC_VB_SUMS]) {
    float pred;      // :497-521
    if (mean_type == DC_VB_MEAN_START_X)
        pred = mo;
    else if (mean_type == DC_VB_MEAN_EPSILON)
        pred = c.rc * xt - c.rm1 * mo;
    else
        pred = c.r1 * mo - c.r21 * xt;
    if (clip) pred = pred < -1.0f ? -1.0f : (pred > 1.0f ? 1.0f : pred);
    const float m2 = mean_type == DC_VB_MEAN_PREVIOUS_X ? mo : c.c1 * pred + c.c2 * xt;      // :522-530
    const float m1 = c.c1 * x0 + c.c2 * xt;                                                   // :418-440
    float lv2;      // :472-503
    if (var_type == DC_VB_VAR_LEARNED)
        lv2 = vv;
    else if (var_type == DC_VB_VAR_LEARNED_RANGE) {
        const float frac = (vv + 1.0f) / 2.0f;
        lv2 = frac * c.lvm + (1.0f - frac) * c.lv1;
    } else
        lv2 = c.lvm;
    const float d = m1 - m2;      // normal_kl (:162-188)
    e[0] = 0.5f * ((((-1.0f + lv2) - c.lv1) + expf(c.lv1 - lv2)) + (d * d) * expf(-lv2));
    // discretized_gaussian_log_likelihood (:199-225) with log_scales = 0.5 log_variance (:992)
    const float kBin = (float)(1.0 / 255.0);
    const float cen = x0 - m2;
    const float inv = expf(-(0.5f * lv2));
    const float cp = vb_cdf(inv * (cen + kBin));
    const float cm = vb_cdf(inv * (cen - kBin));
    const float lcp = logf(clamp_min(cp, 1e-12f));
    const float l1m = logf(clamp_min(1.0f - cm, 1e-12f));
    const float ldl = logf(clamp_min(cp - cm, 1e-12f));
    e[1] = -(x0 < -0.999f ? lcp : (x0 > 0.999f ? l1m : ldl));
    const float dx = pred - x0;      // :1149
    e[2] = dx * dx;
    e[3] = 0.f;
    if (has_noise) {      // :1150-1151 with _predict_eps_from_xstart
        const float de = (c.rc * xt - pred) / c.rm1 - nz;
        e[3] = de * de;
    }
}

// Workgroup blockIdx.x of clip blockIdx.y (of this chunk) reduces pairs [blockIdx.x * per, +per) of the clip's ceil(n / 2) pairs and
// writes its DC_VB_SUMS partial sums to part[clip][blockIdx.x][.].  VEC: float2 loads (n even, 8-byte aligned pointers); else scalar
// loads of the same pairs, so both forms add in the same order.  vv / nz are not read unless the variance is learned / has_noise.
template <bool VEC>
__global__ __launch_bounds__(DC_LOSS_THREADS) void k_vb_partials(const float* __restrict__ x0, const float* __restrict__ xt,
                                                                 const float* __restrict__ mo, const float* __restrict__ vv,
                                                                 const float* __restrict__ nz, float* __restrict__ part, int n, int per,
                                                                 int mean_type, int var_type, int clip, VbScalars cs) {
    __shared__ float lds[4][DC_VB_SUMS];
    const int b = blockIdx.y;
    const VbClip c = {cs.c1[b], cs.c2[b], cs.lv1[b], cs.lvm[b], cs.rc[b], cs.rm1[b], cs.r1[b], cs.r21[b]};
    const size_t base = (size_t)b * n;
    const bool learned = var_type == DC_VB_VAR_LEARNED || var_type == DC_VB_VAR_LEARNED_RANGE, has_noise = nz != nullptr;
    const int npair = (n + 1) >> 1;
    const int lo = blockIdx.x * per, hi = min(lo + per, npair);
    float acc[DC_VB_SUMS] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lo + threadIdx.x; i < hi; i += DC_LOSS_THREADS) {
        const size_t j = base + 2 * (size_t)i;
        const bool two = 2 * i + 1 < n;
        float2 a, t, m, v = {0.f, 0.f}, z = {0.f, 0.f};
        if (VEC) {
            a = *reinterpret_cast<const float2*>(x0 + j);
            t = *reinterpret_cast<const float2*>(xt + j);
            m = *reinterpret_cast<const float2*>(mo + j);
            if (learned) v = *reinterpret_cast<const float2*>(vv + j);
            if (has_noise) z = *reinterpret_cast<const float2*>(nz + j);
        } else {
            a.x = x0[j], t.x = xt[j], m.x = mo[j];
            a.y = two ? x0[j + 1] : 0.f, t.y = two ? xt[j + 1] : 0.f, m.y = two ? mo[j + 1] : 0.f;
            if (learned) v.x = vv[j], v.y = two ? vv[j + 1] : 0.f;
            if (has_noise) z.x = nz[j], z.y = two ? nz[j + 1] : 0.f;
        }
        float e0[DC_VB_SUMS], e1[DC_VB_SUMS];
        vb_element(a.x, t.x, m.x, v.x, z.x, c, mean_type, var_type, clip != 0, has_noise, e0);
        if (VEC || two) {
            vb_element(a.y, t.y, m.y, v.y, z.y, c, mean_type, var_type, clip != 0, has_noise, e1);
#pragma unroll
            for (int k = 0; k < DC_VB_SUMS; ++k) acc[k] = acc[k] + (e0[k] + e1[k]);
        } else {
#pragma unroll
            for (int k = 0; k < DC_VB_SUMS; ++k) acc[k] = acc[k] + e0[k];
        }
    }
    block_tree<DC_VB_SUMS>(acc, lds);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < DC_VB_SUMS; ++k) part[((size_t)b * gridDim.x + blockIdx.x) * DC_VB_SUMS + k] = acc[k];
}

// One wave per clip: the G partials of each sum in index order, the mean, bits for the two likelihood terms (:989, :995), and the
// selection of :999.
__global__ __launch_bounds__(64) void k_vb_combine(const float* __restrict__ part, float* __restrict__ terms, int G, int n, int has_noise,
                                                   VbFlags fl) {
    __shared__ float s[DC_VB_SUMS];
    const int b = blockIdx.x;
    if (threadIdx.x < DC_VB_SUMS) {
        const float* p = part + (size_t)b * G * DC_VB_SUMS + threadIdx.x;
        float v = p[0];
        for (int g = 1; g < G; ++g) v = v + p[(size_t)g * DC_VB_SUMS];
        v = v / (float)n;
        if (threadIdx.x < 2) v = v / (float)0.69314718055994530942;      // np.log(2.0)
        s[threadIdx.x] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float* o = terms + (size_t)b * DC_VB_TERMS;
        o[0] = fl.t0[b] ? s[1] : s[0];
        o[1] = s[0];
        o[2] = s[1];
        o[3] = s[2];
        o[4] = has_noise ? s[3] : 0.f;
        o[5] = 0.f;
        o[6] = 0.f;
        o[7] = 0.f;
    }
}

// _prior_bpd (:1092-1108): normal_kl(a x0, logvar, 0, 0) per element, one workgroup per clip (blockIdx.x = clip of this chunk).
template <bool VEC>
__global__ __launch_bounds__(DC_LOSS_THREADS) void k_prior_kl(const float* __restrict__ x0, float* __restrict__ out, int n, ClipScalars cs) {
    __shared__ float lds[4][1];
    const float a = cs.a[blockIdx.x], lv1 = cs.s[blockIdx.x];
    const size_t base = (size_t)blockIdx.x * n;
    const int npair = (n + 1) >> 1;
    const float lead = ((-1.0f + 0.0f) - lv1) + expf(lv1 - 0.0f);
    float acc[1] = {0.f};
    for (int i = threadIdx.x; i < npair; i += DC_LOSS_THREADS) {
        const size_t j = base + 2 * (size_t)i;
        const bool two = 2 * i + 1 < n;
        float2 x;
        if (VEC)
            x = *reinterpret_cast<const float2*>(x0 + j);
        else
            x.x = x0[j], x.y = two ? x0[j + 1] : 0.f;
        const float m0 = a * x.x - 0.0f, m1 = a * x.y - 0.0f;
        const float k0 = 0.5f * (lead + (m0 * m0) * 1.0f), k1 = 0.5f * (lead + (m1 * m1) * 1.0f);
        acc[0] = acc[0] + ((VEC || two) ? (k0 + k1) : k0);
    }
    block_tree<1>(acc, lds);
    if (threadIdx.x == 0) out[blockIdx.x] = (acc[0] / (float)n) / (float)0.69314718055994530942;
}

inline int vb_groups(int64_t n) {      // workgroups per clip: a function of the clip's size only
    // (DC_VB_GROUPS=g lowers the cap for a process: tools/time_vb.py measures one workgroup per clip against the split with it)
    static const int cap = getenv("DC_VB_GROUPS") ? std::max(1, std::min(DC_VB_MAX_GROUPS, atoi(getenv("DC_VB_GROUPS")))) : DC_VB_MAX_GROUPS;
    const int64_t npair = (n + 1) / 2;
    return (int)std::min<int64_t>(cap, std::max<int64_t>(1, (npair + DC_VB_SPAN - 1) / DC_VB_SPAN));
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

int dc_vb_coefficients(int32_t n_train, const double* h_betas, int32_t var_type, const int32_t* h_timesteps, int32_t B, float* h_coef) {
    if (!h_betas || !h_timesteps || !h_coef) return dc_set_error(DC_ERR_INVALID, "dc_vb_coefficients: NULL argument");
    if (n_train < 1 || B < 1) return dc_set_error(DC_ERR_INVALID, "dc_vb_coefficients: n_train and B must be >= 1");
    if (var_type < DC_VB_VAR_LEARNED || var_type > DC_VB_VAR_LEARNED_RANGE)
        return dc_set_error(DC_ERR_INVALID, "dc_vb_coefficients: var_type must be one of DC_VB_VAR_*");
    if (var_type == DC_VB_VAR_FIXED_LARGE && n_train < 2)
        return dc_set_error(DC_ERR_INVALID, "dc_vb_coefficients: FIXED_LARGE reads posterior_variance[1] (n_train must be >= 2)");
    for (int32_t t = 0; t < n_train; ++t)
        if (!(h_betas[t] > 0.0 && h_betas[t] <= 1.0)) return dc_set_error(DC_ERR_INVALID, "dc_vb_coefficients: betas must be inside (0, 1]");
    for (int32_t b = 0; b < B; ++b)
        if (h_timesteps[b] < 0 || h_timesteps[b] >= n_train)
            return dc_set_error(DC_ERR_INVALID, ("dc_vb_coefficients: timestep " + std::to_string(h_timesteps[b]) + " of clip " +
                                                 std::to_string(b) + " is outside [0, " + std::to_string(n_train) + ")").c_str());
    // the constructor tables of :328-379, in its order of operations
    std::vector<double> ac(n_train);
    double run = 1.0;
    for (int32_t t = 0; t < n_train; ++t) ac[t] = run = run * (1.0 - h_betas[t]);
    auto prev = [&](int32_t t) { return t == 0 ? 1.0 : ac[t - 1]; };
    auto post_var = [&](int32_t t) { return h_betas[t] * (1.0 - prev(t)) / (1.0 - ac[t]); };
    for (int32_t b = 0; b < B; ++b) {
        const int32_t t = h_timesteps[b];
        float* o = h_coef + (size_t)b * DC_VB_COEF;
        const double c1 = h_betas[t] * std::sqrt(prev(t)) / (1.0 - ac[t]);
        const double c2 = (1.0 - prev(t)) * std::sqrt(1.0 - h_betas[t]) / (1.0 - ac[t]);
        const double plv = n_train > 1 ? std::log(post_var(std::max(t, 1))) : std::log(std::max(post_var(t), 1e-20));
        o[0] = (float)c1;
        o[1] = (float)c2;
        o[2] = (float)plv;
        o[3] = var_type == DC_VB_VAR_FIXED_SMALL   ? (float)plv
               : var_type == DC_VB_VAR_FIXED_LARGE ? (float)std::log(t == 0 ? post_var(1) : h_betas[t])
               : var_type == DC_VB_VAR_LEARNED_RANGE ? (float)std::log(h_betas[t])
                                                     : 0.f;
        o[4] = (float)std::sqrt(1.0 / ac[t]);
        o[5] = (float)std::sqrt(1.0 / ac[t] - 1);
        o[6] = t == 0 ? 1.f : 0.f;
        o[7] = (float)(1.0 / c1);
        o[8] = (float)(c2 / c1);
        for (int k = 9; k < DC_VB_COEF; ++k) o[k] = 0.f;
    }
    return DC_OK;
}

int64_t dc_vb_workspace_floats(int32_t B, int32_t T, int32_t P) {
    if (B < 1 || T < 1 || P < 1) return 0;
    return (int64_t)B * vb_groups((int64_t)T * P) * DC_VB_SUMS;
}

int dc_vb_terms(const float* d_x0, const float* d_xt, const float* d_model_out, const float* d_var_values, const float* d_noise,
                const float* h_coef, int32_t mean_type, int32_t var_type, int32_t clip_denoised, int32_t B, int32_t T, int32_t P,
                float* d_workspace, float* d_terms, void* stream) {
    if (!d_x0 || !d_xt || !d_model_out || !h_coef || !d_workspace || !d_terms) return dc_set_error(DC_ERR_INVALID, "dc_vb_terms: NULL argument");
    if (B < 1 || T < 1 || P < 1) return dc_set_error(DC_ERR_INVALID, "dc_vb_terms: B, T and P must be >= 1");
    if ((int64_t)T * P > INT32_MAX - 1) return dc_set_error(DC_ERR_INVALID, "dc_vb_terms: T * P is too large");
    if (mean_type < DC_VB_MEAN_PREVIOUS_X || mean_type > DC_VB_MEAN_EPSILON)
        return dc_set_error(DC_ERR_INVALID, "dc_vb_terms: mean_type must be one of DC_VB_MEAN_*");
    if (var_type < DC_VB_VAR_LEARNED || var_type > DC_VB_VAR_LEARNED_RANGE)
        return dc_set_error(DC_ERR_INVALID, "dc_vb_terms: var_type must be one of DC_VB_VAR_*");
    const bool learned = var_type == DC_VB_VAR_LEARNED || var_type == DC_VB_VAR_LEARNED_RANGE;
    if (learned && !d_var_values) return dc_set_error(DC_ERR_INVALID, "dc_vb_terms: a learned variance needs d_var_values");
    if (!learned && d_var_values) return dc_set_error(DC_ERR_INVALID, "dc_vb_terms: d_var_values beside a fixed variance (must be NULL)");
    hipStream_t st = (hipStream_t)stream;
    const int n = T * P;
    const int G = vb_groups(n);
    const int npair = (n + 1) >> 1;
    const int per = (npair + G - 1) / G;
    const bool vec = (n & 1) == 0 && aligned(d_x0, 8) && aligned(d_xt, 8) && aligned(d_model_out, 8) &&
                     (!d_var_values || aligned(d_var_values, 8)) && (!d_noise || aligned(d_noise, 8));
    for (int32_t b0 = 0; b0 < B; b0 += DC_LOSS_CHUNK) {
        const int nb = std::min<int32_t>(DC_LOSS_CHUNK, B - b0);
        VbScalars cs;
        VbFlags fl;
        for (int i = 0; i < DC_LOSS_CHUNK; ++i) {
            const float* c = h_coef + (size_t)(b0 + std::min(i, nb - 1)) * DC_VB_COEF;      // (slots past nb are never read)
            cs.c1[i] = c[0], cs.c2[i] = c[1], cs.lv1[i] = c[2], cs.lvm[i] = c[3], cs.rc[i] = c[4], cs.rm1[i] = c[5], cs.r1[i] = c[7],
            cs.r21[i] = c[8];
            fl.t0[i] = c[6] != 0.f;
        }
        const size_t off = (size_t)b0 * n;
        float* part = d_workspace + (size_t)b0 * G * DC_VB_SUMS;
        const float* vv = d_var_values ? d_var_values + off : nullptr;
        const float* nz = d_noise ? d_noise + off : nullptr;
        if (vec)
            k_vb_partials<true><<<dim3(G, nb), dim3(DC_LOSS_THREADS), 0, st>>>(d_x0 + off, d_xt + off, d_model_out + off, vv, nz, part, n, per,
                                                                              mean_type, var_type, clip_denoised != 0, cs);
        else
            k_vb_partials<false><<<dim3(G, nb), dim3(DC_LOSS_THREADS), 0, st>>>(d_x0 + off, d_xt + off, d_model_out + off, vv, nz, part, n, per,
                                                                               mean_type, var_type, clip_denoised != 0, cs);
        DC_HIP_TRY(hipGetLastError());
        k_vb_combine<<<dim3(nb), dim3(64), 0, st>>>(part, d_terms + (size_t)b0 * DC_VB_TERMS, G, n, d_noise != nullptr, fl);
        DC_HIP_TRY(hipGetLastError());
    }
    return DC_OK;
}

int dc_prior_kl(const float* d_x0, const float* h_a, const float* h_logvar, int32_t B, int32_t T, int32_t P, float* d_out, void* stream) {
    if (!d_x0 || !h_a || !h_logvar || !d_out) return dc_set_error(DC_ERR_INVALID, "dc_prior_kl: NULL argument");
    if (B < 1 || T < 1 || P < 1) return dc_set_error(DC_ERR_INVALID, "dc_prior_kl: B, T and P must be >= 1");
    if ((int64_t)T * P > INT32_MAX - 1) return dc_set_error(DC_ERR_INVALID, "dc_prior_kl: T * P is too large");
    hipStream_t st = (hipStream_t)stream;
    const int n = T * P;
    const bool vec = (n & 1) == 0 && aligned(d_x0, 8);
    for (int32_t b0 = 0; b0 < B; b0 += DC_LOSS_CHUNK) {
        const int nb = std::min<int32_t>(DC_LOSS_CHUNK, B - b0);
        ClipScalars cs;
        for (int i = 0; i < DC_LOSS_CHUNK; ++i) cs.a[i] = i < nb ? h_a[b0 + i] : 0.f, cs.s[i] = i < nb ? h_logvar[b0 + i] : 0.f;
        if (vec)
            k_prior_kl<true><<<dim3(nb), dim3(DC_LOSS_THREADS), 0, st>>>(d_x0 + (size_t)b0 * n, d_out + b0, n, cs);
        else
            k_prior_kl<false><<<dim3(nb), dim3(DC_LOSS_THREADS), 0, st>>>(d_x0 + (size_t)b0 * n, d_out + b0, n, cs);
        DC_HIP_TRY(hipGetLastError());
    }
    return DC_OK;
}

}  // extern "C"
