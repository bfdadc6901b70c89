// dc_music.hip - MusicEncoder + encode_music on gfx950 (MI355X), hand-written MFMA kernels.
//
// Reference (restated, not translated): Diffusion_Stage/models/transformer.py
//   :289-311 Conv2dResLayer   reflect-pad 3x3 conv -> BatchNorm2d(eval) -> ReLU, plus identity / 1x1-conv+BN residual
//   :313-340 MusicEncoder     conv1 (1->16->16->16) pool(5,5)/(1,2); conv2 (16->32->32) pool(5,5)/(3,2);
//                             conv3 (32->32->32) pool(3,3)/(1,2); [B,32,T,16] -> [B,512,T] -> Conv1d 512->64 + BatchNorm1d
//   :447-459 encode_music     x = music_encoder(mel); x_proj = proj(x)   (eval mode: no token dropout)
//
// Layout.  mel is [B][Tm][128] fp32 = an image with H = time, W = mel bin, one channel.  Every activation lives in HBM
// as TWO bf16 planes (hi, lo: x ~ hi + lo, 16 mantissa bits) in pixel-major order [b][y][x][c]; a pixel's 16 channels of
// one plane are 32 contiguous bytes, i.e. exactly one k-step of a v_mfma_f32_32x32x16_bf16 B operand:
//   lane (n = l & 31, kh = l >> 5) loads the 16 bytes of channels 8kh..8kh+7 of pixel x0 + n (+ tap offset)
// so the implicit GEMM needs no staging or transposition: out[co][pixel] += W_tap[co][ci] * in[ci][pixel + tap] with the
// folded weights as the A operand (LDS-resident, natural-k fragments) and 3 MFMAs per k-step (hi*hi + lo*hi + hi*lo,
// "bf16x3": ~1e-5 relative, the conditioning must not cost the sampler its 1e-3 parity budget).
// A wave owns 32 consecutive pixels of one image row; the accumulator tile has the output channels on registers
// (row (r&3) + 8(r>>2) + 4(l>>5)) and those pixels on lanes, so bias / ReLU / residual / the hi-lo split are per-lane and
// the stores are 8-byte pieces that tile the row's bytes without gaps.
// Neighbouring taps re-read the same lines from L1/L2; HBM sees each plane about once per layer.
#include "dc_music.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "dc_common.h"   // DEV, relu, nanmax
#include "dc_launch.h"   // dc_lds_optin, dc_cu_count

namespace {

DEV f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
DEV f32x16 mma3(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x16 acc) {
    acc = mfma(ah, bh, acc);
    acc = mfma(al, bh, acc);
    return mfma(ah, bl, acc);
}
DEV int reflect(int i, int n) {        // torch 'reflect' padding of width 1 (no edge repeat)
    i = i < 0 ? -i : i;
    // (callers also ask for halo rows of tiles that reach past the image - up to ROWS + 2 beyond it, values nobody uses: with fewer rows
    // than that in the image the single reflection would leave it on the other side, hence the clamp)
    return max(i >= n ? 2 * n - 2 - i : i, 0);
}
DEV void split8(const float (&v)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h = (__bf16)v[j];
        hi[j] = h;
        lo[j] = (__bf16)(v[j] - (float)h);
    }
}
// relu (dc_common.h) as two pinned instructions: in k_me_stem's phase A at 128 registers the compiler's own pair costs 12 more spilled registers
// (k_me_stem<8, 64, false>: 752 -> 847 us per 32 clips; pinned: the parent's 10 spills)
DEV float relu_pinned(float y) {
    float r;
    asm("v_cmp_gt_f32 vcc, 0, %1\n\tv_cndmask_b32_e64 %0, %1, 0, vcc" : "=v"(r) : "v"(y) : "vcc");
    return r;
}
DEV f32x16 zero16() {
    f32x16 x;
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = 0.f;
    return x;
}

// ---------------------------------------------------------------------------------------------------------
// Plane formats.  SP = true: the split form above (two bf16 planes, three MFMAs per k-step: ~6e-6 at the encoder's output).
// SP = false: ONE fp16 plane and fp16 weights, one MFMA per k-step, half the LDS reads and half the HBM bytes: every activation is
// rounded to 11 bits once per layer - 3.7e-4 relative at the encoder's output, 1.3e-4 of x0 after DDIM-50 (tests/study_encoder_fp16.py
// reproduces both on the CPU), i.e. the order of the fp16 operand rounding the fp16 sampler applies to these features anyway.
// dc_music_encode picks the format per call (dc_music_set_format / DC_ME_PREC); the kernels are the same templates.
// ---------------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
template <bool SP> struct PL;
template <> struct PL<true> {
    using e = __bf16;
    using v8 = bf16x8;
    using v4 = bf16x4;
    static constexpr int N = 2;
};
template <> struct PL<false> {
    using e = _Float16;
    using v8 = f16x8;
    using v4 = f16x4;
    static constexpr int N = 1;
};
DEV f32x16 mfma(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
// one k-step: split planes hi*hi + lo*hi + hi*lo; single plane one product (al, bl are then dead values and their loads disappear)
DEV f32x16 mma(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x16 acc) { return mma3(ah, al, bh, bl, acc); }
DEV f32x16 mma(f16x8 ah, f16x8, f16x8 bh, f16x8, f32x16 acc) { return mfma(ah, bh, acc); }
// four values -> one 8-byte piece per plane
DEV void put4(const float (&v)[4], __bf16* hi, __bf16* lo) {
    bf16x4 oh, ol;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const __bf16 h = (__bf16)v[e];
        oh[e] = h;
        ol[e] = (__bf16)(v[e] - (float)h);
    }
    *reinterpret_cast<bf16x4*>(hi) = oh;
    *reinterpret_cast<bf16x4*>(lo) = ol;
}
DEV void put4(const float (&v)[4], _Float16* hi, _Float16*) {
    f16x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (_Float16)v[e];
    *reinterpret_cast<f16x4*>(hi) = o;
}
// value of element e of an 8-byte piece (pair)
DEV float val4(const bf16x4& h, const bf16x4& l, int e) { return (float)h[e] + (float)l[e]; }
DEV float val4(const f16x4& h, const f16x4&, int e) { return (float)h[e]; }

// ---------------------------------------------------------------------------------------------------------
// 3x3 reflect-padded convolution + folded BatchNorm + ReLU (+ residual).  RES: 0 none, 1 identity, 2 1x1 conv + BN.
// Weight fragments (A operand, natural k = tap*CIN + ci): [hi: NKS][lo: NKS] then for RES == 2 [hi: KC][lo: KC].
// ---------------------------------------------------------------------------------------------------------
// conv1.0 alone (1 -> 16 channels, no residual; the first of DC_ME_NO_STEM=1's three launches, split planes): it reads the fp32 mel
// directly, its single k-step holds the 9 taps (k = tap), split in registers.  A wave owns 32 consecutive pixels of one image row.
__global__ __launch_bounds__(256) void k_me_conv10(const float* __restrict__ mel, __bf16* __restrict__ out_hi, __bf16* __restrict__ out_lo,
                                                   const bf16x8* __restrict__ w /* hi, lo */, const float* __restrict__ bias_ft, int Bc, int H,
                                                   int W, int tiles_per_wave) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    bf16x8* wl = reinterpret_cast<bf16x8*>(lds);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 31, kh = lane >> 5;
    for (int f = wave; f < 2; f += 4) wl[f * 64 + lane] = w[f * 64 + lane];
    __syncthreads();
    f32x16 bias;
#pragma unroll
    for (int r = 0; r < 16; ++r) bias[r] = bias_ft[kh * 16 + r];
    const int xt_per_row = W / 32;
    const long long total = (long long)Bc * H * xt_per_row;
    const long long t0 = ((long long)blockIdx.x * 4 + wave) * tiles_per_wave;
    for (int i = 0; i < tiles_per_wave; ++i) {
        const long long tile = t0 + i;
        if (tile >= total) break;
        const int xt = (int)(tile % xt_per_row);
        const int y = (int)((tile / xt_per_row) % H);
        const int b = (int)(tile / ((long long)xt_per_row * H));
        const int x = xt * 32 + n;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int t = 8 * kh + j;
            const int yy = reflect(y + t / 3 - 1, H), xx = reflect(x + t % 3 - 1, W);
            v[j] = t < 9 ? mel[((size_t)b * H + yy) * W + xx] : 0.f;
        }
        bf16x8 bh, bl;
        split8(v, bh, bl);
        const f32x16 acc = mma3(wl[lane], wl[64 + lane], bh, bl, zero16());
        const size_t pix = ((size_t)b * H + y) * W + x;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int c0 = 8 * q + 4 * kh;          // this lane's 4 consecutive output channels of register group q
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = relu(acc[4 * q + e] + bias[4 * q + e]);
            put4(o, out_hi + pix * 16 + c0, out_lo + pix * 16 + c0);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The layers with CIN >= 16, from an LDS-resident input tile.  Reading every tap of every pixel from L1 / L2 is 18 KiB
// of loads per 2 KiB of unique input (2.3 TB/s of HBM at best); here a persistent 4-wave workgroup
// copies a (ROWS + 2) x (32 NXS + 2)-pixel halo tile of both planes into LDS by LDS-DMA (reflect padding by index) once
// and feeds all nine taps from there.  LDS piece order [plane][16-channel chunk][channel half][row][pixel] x 16 B: the
// B operand of one tap is 32 consecutive pieces per channel half - conflict-free ds_read_b128 - and a tap shift is a
// piece offset.  The weight fragments of a k-step are read once per wave for its ROWS NXS / 4 wave tiles; the identity
// residual and the 1x1 residual convolution take the centre pixels from the same tile.  Two workgroups per CU: one
// fills while the other computes.
// ---------------------------------------------------------------------------------------------------------
DEV void me_dma16(const void* gsrc /*per-lane*/, const char* lds_dst /*wave-uniform*/) {
    const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(const __attribute__((address_space(3))) char*)lds_dst);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(dst)
                 : "memory");
}
template <int CIN, int COUT, int RES, int ROWS, int NXS, bool SP>
__global__ __launch_bounds__(256, 2) void k_me_conv_t(const typename PL<SP>::v8* __restrict__ in_hi, const typename PL<SP>::v8* __restrict__ in_lo,
                                                      typename PL<SP>::e* __restrict__ out_hi, typename PL<SP>::e* __restrict__ out_lo,
                                                      const typename PL<SP>::v8* __restrict__ w, const float* __restrict__ bias_ft,
                                                      const float* __restrict__ rbias_ft, int H, int W, int ntiles) {
    using V8 = typename PL<SP>::v8;
    using V4 = typename PL<SP>::v4;
    constexpr int NPL = PL<SP>::N;                  // planes (weights: [hi: NKS][lo: NKS][res hi: KC][res lo: KC], single plane: [NKS][res: KC])
    constexpr int KC = CIN / 16, NKS = 9 * KC, NF = NPL * NKS + (RES == 2 ? NPL * KC : 0);
    constexpr int TX = 32 * NXS, PXW = TX + 2, RH = ROWS + 2;
    constexpr int SEL = RH * PXW;                    // pieces per (plane, chunk, half)
    constexpr int NP = NPL * KC * 2 * SEL;
    constexpr int NDMA = (NP + 63) / 64;
    constexpr int TPW = ROWS * NXS / 4;
    static_assert(ROWS * NXS % 4 == 0, "wave tiles divide over 4 waves");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    V8* wl = reinterpret_cast<V8*>(lds);
    V8* tl = wl + NF * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 31, kh = lane >> 5;
    for (int f = wave; f < NF; f += 4) wl[f * 64 + lane] = w[f * 64 + lane];
    f32x16 bias, rbias;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        bias[r] = bias_ft[kh * 16 + r];
        rbias[r] = RES == 2 ? rbias_ft[kh * 16 + r] : 0.f;
    }
    const int txn = W / TX, tyn = (H + ROWS - 1) / ROWS;
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = t % txn, ty = (t / txn) % tyn, b = t / (txn * tyn);
        const int x0 = tx * TX, y0 = ty * ROWS;
        for (int j = wave; j < NDMA; j += 4) {
            const int p = 64 * j + lane;
            if (p < NP) {
                const int px = p % PXW, row = (p / PXW) % RH, sel = p / SEL;
                const int yy = reflect(y0 - 1 + row, H), xx = reflect(x0 - 1 + px, W);
                const V8* src = ((sel >= 2 * KC) ? in_lo : in_hi) + (((size_t)b * H + yy) * W + xx) * (CIN / 8) + (sel % (2 * KC));
                me_dma16(src, reinterpret_cast<const char*>(tl + 64 * j));
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        f32x16 acc[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) acc[i] = zero16();
        // piece of (plane, chunk kc, this lane's half, tile row r + dy, pixel 32 seg + n + dx), halo coordinates
        auto piece = [&](int plane, int kc, int r, int seg, int dy, int dx) {
            return tl[((plane * KC + kc) * 2 + kh) * SEL + (r + dy) * PXW + seg * 32 + n + dx];
        };
        constexpr int LO = NPL - 1;                  // the second plane (single plane: the same piece, a dead value)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) {
                const int ks = tap * KC + kc;
                const V8 ah = wl[ks * 64 + lane], al = wl[(LO * NKS + ks) * 64 + lane];
#pragma unroll
                for (int i = 0; i < TPW; ++i) {
                    const int wt = wave * TPW + i, r = wt / NXS, seg = wt % NXS;
                    acc[i] = mma(ah, al, piece(0, kc, r, seg, tap / 3, tap % 3), piece(LO, kc, r, seg, tap / 3, tap % 3), acc[i]);
                }
            }
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int wt = wave * TPW + i, r = wt / NXS, seg = wt % NXS;
            const int y = y0 + r, x = x0 + seg * 32 + n;
            f32x16 res = zero16();
            if constexpr (RES == 2) {
#pragma unroll
                for (int kc = 0; kc < KC; ++kc)
                    res = mma(wl[(NPL * NKS + kc) * 64 + lane], wl[(NPL * NKS + LO * KC + kc) * 64 + lane], piece(0, kc, r, seg, 1, 1),
                              piece(LO, kc, r, seg, 1, 1), res);
            }
            if (y >= H) continue;
            const size_t pix = ((size_t)b * H + y) * W + x;
#pragma unroll
            for (int q = 0; q < COUT / 8; ++q) {
                const int c0 = 8 * q + 4 * kh;          // this lane's 4 consecutive output channels of register group q
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu(acc[i][4 * q + e] + bias[4 * q + e]);
                if constexpr (RES == 1) {               // input channels c0 .. c0+3 of the centre pixel: half kh of piece (q >> 1, q & 1)
                    const int pc = ((q >> 1) * 2 + (q & 1)) * SEL + (r + 1) * PXW + seg * 32 + n + 1;
                    const V4 xh = reinterpret_cast<const V4*>(tl + pc)[kh];
                    const V4 xl = reinterpret_cast<const V4*>(tl + LO * 2 * KC * SEL + pc)[kh];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += val4(xh, xl, e);
                }
                if constexpr (RES == 2) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += res[4 * q + e] + rbias[4 * q + e];
                }
                put4(v, out_hi + pix * COUT + c0, out_lo + pix * COUT + c0);
            }
        }
        __syncthreads();          // everyone is done with the tile before the next fill lands
    }
}

// ---------------------------------------------------------------------------------------------------------
// conv1 (1 -> 16 -> 16 -> 16 at full mel resolution) as ONE kernel: the three layers' activations of an 8 x 64-pixel
// output tile never leave the CU.  Separately they write / read 708 MB each per 16 clips (3.9 GB for the three layers);
// fused, HBM sees the mel (44 MB) and the third layer's output.  A persistent 8-wave workgroup per CU:
//   A: conv1.0 on the tile grown by 2 pixels (12 x 68), from mel (global, 9 taps per lane)       -> LDS tile TA
//   B: conv1.1 on the tile grown by 1 (10 x 66), taps + identity residual from TA                -> LDS tile TB
//   C: conv1.2 on the tile, taps + residual from TB                                              -> HBM
// Reflect padding: a position outside the image holds the layer's value AT THE REFLECTED POSITION, so the grown tiles are
// computed at reflected coordinates (a lane reads its taps around the reflected position's place in the tile below).
// 16 output channels = one v_mfma_f32_16x16x32_bf16 row block; a k-step holds two taps x 16 channels (lane group q4: tap
// 2 ks + (q4 >> 1), channels 8 (q4 & 1) ..): 5 k-steps x 3 split products per 16 pixels, none of it padding rows.
// The D tile has the pixel on the lane and channels 4 q4 .. 4 q4 + 3 in registers: one 8-byte piece per plane, the four
// lane groups complete a pixel's 32 bytes in one store instruction.
// ---------------------------------------------------------------------------------------------------------
DEV f32x4 mfma16b(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
DEV f32x4 mfma16b(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
DEV f32x4 mma_16(bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl, f32x4 acc) {
    acc = mfma16b(ah, bh, acc);
    acc = mfma16b(al, bh, acc);
    return mfma16b(ah, bl, acc);
}
DEV f32x4 mma_16(f16x8 ah, f16x8, f16x8 bh, f16x8, f32x4 acc) { return mfma16b(ah, bh, acc); }
// SP = false (one fp16 plane): 51 KiB of LDS and two workgroups per CU - one's phase A (vector ALU) beside the other's MFMA phases.
template <int ROWS, int TX, bool SP>
__global__ __launch_bounds__(512, SP ? 2 : 4) void k_me_stem(const float* __restrict__ mel, typename PL<SP>::e* __restrict__ out_hi,
                                                               typename PL<SP>::e* __restrict__ out_lo,
                                                    const typename PL<SP>::v8* __restrict__ w /* split: 22 fragments (conv1.0: hi, lo; conv1.1: 5 hi, 5 lo; conv1.2: 5 hi, 5 lo); single plane: 10 (conv1.1: 5, conv1.2: 5) */,
                                                    const float* __restrict__ bias /*[3][16]*/,
                                                    const float* __restrict__ wa32 /* conv1.0 folded weights [16][9] */, int H, int W, int ntiles) {
    using E = typename PL<SP>::e;
    using V8 = typename PL<SP>::v8;
    using V4 = typename PL<SP>::v4;
    constexpr int NPL = PL<SP>::N, LO = NPL - 1;
    constexpr int RAH = ROWS + 4, RAW = TX + 4, NA = RAH * RAW;       // conv1.0 region
    constexpr int RBH = ROWS + 2, RBW = TX + 2, NB = RBH * RBW;       // conv1.1 region
    constexpr int NBP = (NB + 15) / 16 * 16;                          // plane stride of TB: a multiple of 256 B keeps the reads conflict-free
    constexpr int NC = ROWS * TX;
    constexpr int MH = ROWS + 6, MW = TX + 6, NM = MH * MW;           // mel region; positions outside the image hold the reflected values
    static_assert(NA % 16 == 0, "plane stride of TA");
    static_assert(NM <= 1024, "two mel values per thread");
    static_assert(TX == 64 && NC % 128 == 0, "phase C walks two rows per step");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* TA = lds;                                // pieces [plane][half][NA] x 16 B
    char* TB = TA + 2 * NPL * NA * 16;             // pieces [plane][half][NBP] x 16 B
    float* MT = reinterpret_cast<float*>(TB + 2 * NPL * NBP * 16);
    float* WA = MT + NM;                           // single plane: conv1.0's 144 weights (two workgroups per CU leave 128 registers per lane)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = lane & 15, q4 = lane >> 4;
    // conv1.1 / conv1.2 weight fragments stay in registers (the B operands are the only LDS reads of the MFMA phases)
    V8 wb_h[5], wb_l[5], wc_h[5], wc_l[5];
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
        if constexpr (SP) {
            wb_h[ks] = w[(2 + ks) * 64 + lane];
            wb_l[ks] = w[(7 + ks) * 64 + lane];
            wc_h[ks] = w[(12 + ks) * 64 + lane];
            wc_l[ks] = w[(17 + ks) * 64 + lane];
        } else {
            wb_h[ks] = wb_l[ks] = w[ks * 64 + lane];
            wc_h[ks] = wc_l[ks] = w[(5 + ks) * 64 + lane];
        }
    }
    const f32x4 bb = *reinterpret_cast<const f32x4*>(bias + 16 + 4 * q4), bc = *reinterpret_cast<const f32x4*>(bias + 32 + 4 * q4);
    // phase A runs on the vector ALU in fp32: thread = (pixel, channel quad); its quad's 36 weights in registers
    const int quad = tid & 3;
    float wa[4][9];
    if constexpr (SP) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int k = 0; k < 9; ++k) wa[c][k] = wa32[(4 * quad + c) * 9 + k];
    } else if (tid < 144) {
        WA[tid] = wa32[tid];
    }
    const f32x4 ba = *reinterpret_cast<const f32x4*>(bias + 4 * quad);
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    // k-step ks of this lane: tap 2 ks + (q4 >> 1) (the ninth tap's partner slot has zero weights: it re-reads tap 8), channel half q4 & 1
    int ckA[5], ckB[5];          // piece offsets relative to the centre piece (TA: centre = the position itself; TB: centre = tile origin)
#pragma unroll
    for (int ks = 0; ks < 5; ++ks) {
        const int tap = min(2 * ks + (q4 >> 1), 8);
        ckA[ks] = ((q4 & 1) * NA + (tap / 3 - 1) * RAW + tap % 3 - 1) * 16;
        ckB[ks] = ((q4 & 1) * NBP + (tap / 3) * RBW + tap % 3) * 16;
    }
    const int hp = (q4 >> 1), ho = (q4 & 1) * 8;         // this lane's output channels 4 q4 .. +3: half hp, byte offset ho of the piece
    const int txn = W / TX, tyn = (H + ROWS - 1) / ROWS;
    // mel region of tile t: thread i holds elements i and i + 512
    auto mel_fetch = [&](int t, float (&mv)[2]) {
        const int tx = t % txn, ty = (t / txn) % tyn, b = t / (txn * tyn);
        const float* mb = mel + (size_t)b * H * W;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = tid + 512 * k;
            mv[k] = 0.f;
            if (i < NM) mv[k] = mb[(size_t)reflect(ty * ROWS - 3 + i / MW, H) * W + reflect(tx * TX - 3 + i % MW, W)];
        }
    };
    float mv[2];
    if ((int)blockIdx.x < ntiles) mel_fetch(blockIdx.x, mv);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = t % txn, ty = (t / txn) % tyn, b = t / (txn * tyn);
        const int x0 = tx * TX, y0 = ty * ROWS;
        MT[tid] = mv[0];
        if (tid + 512 < NM) MT[tid + 512] = mv[1];
        __syncthreads();            // also: everyone has left the previous tile's phase C (TB) and phase A (MT)
        if (t + (int)gridDim.x < ntiles) mel_fetch(t + gridDim.x, mv);      // lands during the three phases
        // local coordinate of image position (tile origin - g + i) reflected into the image, in a region that starts at origin - G
        auto local = [](int i, int o0, int g, int G, int size, int lim) {
            const int r = reflect(o0 - g + i, size) - (o0 - G);
            return min(max(r, 1), lim - 2);
        };
        // ---- A: conv1.0 at the reflected positions of the 2-pixel-grown tile (fp32 FMAs; taps are plain neighbours in MT)
#ifndef DC_DIAG_STEM_SKIP
#define DC_DIAG_STEM_SKIP 0          // diagnostic builds (timing only, results invalid): bit 0 / 1 / 2 = phase A / B / C does not run
#endif
        if (!(DC_DIAG_STEM_SKIP & 1)) {
            if constexpr (!SP) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
#pragma unroll
                    for (int k = 0; k < 9; ++k) wa[c][k] = WA[(4 * quad + c) * 9 + k];
            }
            int row = (tid >> 2) / RAW, px = (tid >> 2) % RAW;
            for (int p = tid >> 2; p < NA; p += 128) {
                const int cy = local(row, y0, 2, 3, H, MH), cx = local(px, x0, 2, 3, W, MW);
                const float* m0 = MT + cy * MW + cx;
                f32x4 acc = ba;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    const float mval = m0[(k / 3 - 1) * MW + k % 3 - 1];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[c] = fmaf(wa[c][k], mval, acc[c]);
                }
                float v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = relu_pinned(acc[c]);
                char* dst = TA + (size_t)(((quad >> 1) * NA + p) * 16 + (quad & 1) * 8);
                put4(v, reinterpret_cast<E*>(dst), reinterpret_cast<E*>(dst + 2 * NA * 16));
                px += 128 - RAW;
                row += 1;
                if (px >= RAW) {
                    px -= RAW;
                    row += 1;
                }
            }
        }
        __syncthreads();
        // ---- B: conv1.1 at the reflected positions of the 1-pixel-grown tile, from TA
        if (!(DC_DIAG_STEM_SKIP & 2)) {
            int row = (wave * 16 + n) / RBW, px = (wave * 16 + n) % RBW;
            for (int f = wave * 16 + n; f < NBP; f += 128) {
                const int rr = min(row, RBH - 1);
                const int ly = local(rr, y0, 1, 2, H, RAH), lx = local(px, x0, 1, 2, W, RAW);
                const char* ctr = TA + (size_t)(ly * RAW + lx) * 16;
                f32x4 acc = z4;
#pragma unroll
                for (int ks = 0; ks < 5; ++ks) {
                    const V8 bh = *reinterpret_cast<const V8*>(ctr + ckA[ks]);
                    const V8 bl = *reinterpret_cast<const V8*>(ctr + ckA[ks] + LO * 2 * NA * 16);
                    acc = mma_16(wb_h[ks], wb_l[ks], bh, bl, acc);
                }
                const V4 rh = *reinterpret_cast<const V4*>(ctr + hp * NA * 16 + ho);
                const V4 rl = *reinterpret_cast<const V4*>(ctr + (LO * 2 + hp) * NA * 16 + ho);
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu(acc[e] + bb[e]) + val4(rh, rl, e);
                if (f < NB) {
                    char* dst = TB + (size_t)((hp * NBP + f) * 16 + ho);
                    put4(v, reinterpret_cast<E*>(dst), reinterpret_cast<E*>(dst + 2 * NBP * 16));
                }
                px += 128 - RBW;
                row += 1;
                if (px >= RBW) {
                    px -= RBW;
                    row += 1;
                }
            }
        }
        __syncthreads();
        // ---- C: conv1.2 on the tile, from TB (its halo already holds the reflected values); two tile rows per step
        if (!(DC_DIAG_STEM_SKIP & 4)) {
            const int row0 = wave >> 2, px = (wave & 3) * 16 + n;
            const char* org = TB + (size_t)(row0 * RBW + px) * 16;
            size_t pix = ((size_t)b * H + y0 + row0) * W + x0 + px;
            constexpr int UNR = SP ? ROWS / 2 : 1;          // (single plane: 128 registers per lane)
#pragma unroll(UNR)
            for (int k = 0; k < ROWS / 2; ++k) {
                f32x4 acc = z4;
#pragma unroll
                for (int ks = 0; ks < 5; ++ks) {
                    const V8 bh = *reinterpret_cast<const V8*>(org + ckB[ks]);
                    const V8 bl = *reinterpret_cast<const V8*>(org + ckB[ks] + LO * 2 * NBP * 16);
                    acc = mma_16(wc_h[ks], wc_l[ks], bh, bl, acc);
                }
                const char* ctr = org + (RBW + 1) * 16;
                const V4 rh = *reinterpret_cast<const V4*>(ctr + hp * NBP * 16 + ho);
                const V4 rl = *reinterpret_cast<const V4*>(ctr + (LO * 2 + hp) * NBP * 16 + ho);
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu(acc[e] + bc[e]) + val4(rh, rl, e);
                if (y0 + row0 + 2 * k < H) put4(v, out_hi + pix * 16 + 4 * q4, out_lo + pix * 16 + 4 * q4);
                org += 2 * RBW * 16;
                pix += 2 * (size_t)W;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// conv2 (16 -> 32 with the 1x1-convolution residual, then 32 -> 32 with the identity residual, at 5400 x 64) as ONE kernel, built
// like k_me_stem: a persistent 8-wave workgroup per CU keeps the 32-channel intermediate of an 8 x 32-pixel tile (grown by one
// pixel) in LDS, so its 1.4 GB per 32 clips are neither written nor read back.
//   fill: the input tile grown by 2 (12 x 36 pixels, both planes) by LDS-DMA, reflect padding by index          -> TA
//   B:    conv2.0 + residual at the reflected positions of the 1-pixel-grown tile (10 x 34), taps from TA        -> TB
//   C:    conv2.1 + identity residual on the tile, taps from TB; the next tile's fill is in flight meanwhile     -> HBM
// v_mfma_f32_32x32x16_bf16 (32 output channels = the tile's rows), weights of both layers in LDS (56 KiB).
// ---------------------------------------------------------------------------------------------------------
// SP = false (one fp16 plane): 64 KiB of LDS, two workgroups per CU.
template <int ROWS, int TX, bool SP>
__global__ __launch_bounds__(512, SP ? 2 : 4) void k_me_mid(const typename PL<SP>::v8* __restrict__ in_hi, const typename PL<SP>::v8* __restrict__ in_lo,
                                                   typename PL<SP>::e* __restrict__ out_hi, typename PL<SP>::e* __restrict__ out_lo,
                                                   const typename PL<SP>::v8* __restrict__ w0 /* conv2.0: 9 hi, 9 lo, residual hi, lo (single plane: 9, residual) */,
                                                   const float* __restrict__ bias0_ft, const float* __restrict__ rbias0_ft,
                                                   const typename PL<SP>::v8* __restrict__ w1 /* conv2.1: 18 hi, 18 lo (single plane: 18) */,
                                                   const float* __restrict__ bias1_ft, int H, int W, int ntiles) {
    using V8 = typename PL<SP>::v8;
    using V4 = typename PL<SP>::v4;
    using E = typename PL<SP>::e;
    constexpr int NPL = PL<SP>::N, LO = NPL - 1;
    static_assert(TX == 32 && ROWS == 8, "phase C: one tile row per wave");
    constexpr int RAH = ROWS + 4, RAW = TX + 4, NA = RAH * RAW;           // input region (16 channels: halves kh)
    constexpr int RBH = ROWS + 2, RBW = TX + 2, NB = RBH * RBW;           // conv2.0 region (32 channels: chunks kc, halves kh)
    constexpr int NBP = (NB + 15) / 16 * 16;
    constexpr int NPA = 2 * NPL * NA;                                      // 16-byte pieces of TA: [plane][kh][NA]
    constexpr int NDMA = (NPA + 63) / 64;
    constexpr int NW0 = 10 * NPL, NW1 = 18 * NPL;
    static_assert(NA % 16 == 0, "plane stride of TA");
    extern __shared__ __attribute__((aligned(16))) char lds[];
    V8* wl0 = reinterpret_cast<V8*>(lds);                                  // 20 (10) fragments
    V8* wl1 = wl0 + NW0 * 64;                                              // 36 (18) fragments
    V8* TA = wl1 + NW1 * 64;                                               // pieces [plane][kh][NA]
    V8* TB = TA + NDMA * 64;                                               // pieces [plane][kc][kh][NBP]
    float* BL = reinterpret_cast<float*>(TB + NPL * 4 * NBP);              // single plane: the three bias vectors (128 registers per lane)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = lane & 31, kh = lane >> 5;
    for (int f = wave; f < NW0; f += 8) wl0[f * 64 + lane] = w0[f * 64 + lane];
    for (int f = wave; f < NW1; f += 8) wl1[f * 64 + lane] = w1[f * 64 + lane];      // (in registers instead: 4.36 vs 4.25 ms per 32 clips)
    f32x16 bias0, rbias0, bias1;
    if constexpr (SP) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            bias0[r] = bias0_ft[kh * 16 + r];
            rbias0[r] = rbias0_ft[kh * 16 + r];
            bias1[r] = bias1_ft[kh * 16 + r];
        }
    } else if (tid < 96) {
        BL[tid] = tid < 32 ? bias0_ft[tid] : tid < 64 ? rbias0_ft[tid - 32] : bias1_ft[tid - 64];
    }
    auto ld16 = [&](int which) {                                           // one bias vector of this lane's half from LDS
        f32x16 v;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x4 t4 = *reinterpret_cast<const f32x4*>(BL + which * 32 + kh * 16 + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[4 * q + e] = t4[e];
        }
        return v;
    };
    const int txn = W / TX, tyn = (H + ROWS - 1) / ROWS;
    auto fill = [&](int t) {
        const int tx = t % txn, ty = (t / txn) % tyn, b = t / (txn * tyn);
        for (int j = wave; j < NDMA; j += 8) {
            const int p = 64 * j + lane;
            if (p < NPA) {
                const int idx = p % NA, sel = p / NA;                      // sel = plane * 2 + kh
                const int yy = reflect(ty * ROWS - 2 + idx / RAW, H), xx = reflect(tx * TX - 2 + idx % RAW, W);
                const V8* src = ((sel >> 1) ? in_lo : in_hi) + (((size_t)b * H + yy) * W + xx) * 2 + (sel & 1);
                me_dma16(src, reinterpret_cast<const char*>(TA + 64 * j));
            }
        }
    };
    auto local = [](int i, int o0, int g, int G, int size, int lim) {      // as in k_me_stem
        const int r = reflect(o0 - g + i, size) - (o0 - G);
        return min(max(r, 1), lim - 2);
    };
    if ((int)blockIdx.x < ntiles) fill(blockIdx.x);
    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = t % txn, ty = (t / txn) % tyn, b = t / (txn * tyn);
        const int x0 = tx * TX, y0 = ty * ROWS;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                // TA has landed; everyone has left the previous tile's phase C (TB)
        // ---- B: conv2.0 (+ 1x1 residual) at the reflected positions of the 1-pixel-grown tile
        for (int f0 = wave * 32; f0 < NB; f0 += 256) {
            const int f = f0 + n, fr = min(f, NB - 1);
            const int row = fr / RBW, px = fr % RBW;
            const int ly = local(row, y0, 1, 2, H, RAH), lx = local(px, x0, 1, 2, W, RAW);
            const V8* ctr = TA + kh * NA + ly * RAW + lx;
            f32x16 acc = zero16();
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int o = (tap / 3 - 1) * RAW + tap % 3 - 1;
                acc = mma(wl0[tap * 64 + lane], wl0[(LO * 9 + tap) * 64 + lane], ctr[o], ctr[LO * 2 * NA + o], acc);
            }
            const f32x16 res = mma(wl0[NPL * 9 * 64 + lane], wl0[(NPL * 9 + LO) * 64 + lane], ctr[0], ctr[LO * 2 * NA], zero16());
            if constexpr (!SP) {
                bias0 = ld16(0);
                rbias0 = ld16(1);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {           // output channels 8 q + 4 kh .. + 3: chunk q >> 1, half q & 1, byte offset 8 kh
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = relu(acc[4 * q + e] + bias0[4 * q + e]) + res[4 * q + e] + rbias0[4 * q + e];
                if (f < NB) {
                    V8* dst = TB + ((q >> 1) * 2 + (q & 1)) * NBP + f;
                    put4(v, reinterpret_cast<E*>(dst) + 4 * kh, reinterpret_cast<E*>(dst + 4 * NBP) + 4 * kh);
                }
            }
        }
        __syncthreads();
        if (t + (int)gridDim.x < ntiles) fill(t + gridDim.x);       // TA is free: the next tile's input lands during phase C
        // ---- C: conv2.1 + identity residual: wave = tile row
        {
            const int row = wave;
            const V8* org = TB + kh * NBP + row * RBW + n;          // piece of (kc 0, this half, halo row `row`, halo column n)
            f32x16 acc = zero16();
#pragma unroll
            for (int tap = 0; tap < 9; ++tap)
#pragma unroll
                for (int kc = 0; kc < 2; ++kc) {
                    const int ks = tap * 2 + kc, o = kc * 2 * NBP + (tap / 3) * RBW + tap % 3;
                    acc = mma(wl1[ks * 64 + lane], wl1[(LO * 18 + ks) * 64 + lane], org[o], org[LO * 4 * NBP + o], acc);
                }
            const int y = y0 + row;
            if constexpr (!SP) bias1 = ld16(2);
            if (y < H) {
                const size_t pix = ((size_t)b * H + y) * W + x0 + n;
                const V8* ctr = TB + (row + 1) * RBW + n + 1;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const V4 xh = reinterpret_cast<const V4*>(ctr + ((q >> 1) * 2 + (q & 1)) * NBP)[kh];
                    const V4 xl = reinterpret_cast<const V4*>(ctr + (LO * 4 + (q >> 1) * 2 + (q & 1)) * NBP)[kh];
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = relu(acc[4 * q + e] + bias1[4 * q + e]) + val4(xh, xl, e);
                    put4(v, out_hi + pix * 32 + 8 * q + 4 * kh, out_lo + pix * 32 + 8 * q + 4 * kh);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// max_pool2d; padding never wins (torch pads with -inf) and a NaN always does.  One thread per (pixel, 8 channels).
// Sliding window along time: a thread owns (clip, output column, 8 channels) and walks NY consecutive output rows,
// keeping the last KH row maxima (each the maximum over the KW taps of one input row) in registers; an output row
// costs SH new input rows instead of KH (5x5 stride 1: 5x fewer loads than one thread per output).
// (Two adjacent output columns per thread share 3 of their 10 loads per input row, at 173 VGPRs instead of 48: no faster,
// profiles/r05_ab_pool.txt.)
// ---------------------------------------------------------------------------------------------------------
// The window of a plane pair: eight fp32 values under nanmax.  hi + lo is exact in fp32 (<= 17 significant bits), so the maximum
// re-splits into the very planes it came from.
struct PoolWinS {
    float m[8];
};
DEV void pool_clear(PoolWinS& w) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w.m[j] = -INFINITY;
}
DEV void pool_take(PoolWinS& w, bf16x8 h, bf16x8 l) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w.m[j] = nanmax(w.m[j], (float)h[j] + (float)l[j]);
}
DEV void pool_merge(PoolWinS& w, const PoolWinS& o) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w.m[j] = nanmax(w.m[j], o.m[j]);
}
DEV void pool_put(const PoolWinS& w, bf16x8* hi, bf16x8* lo, size_t o) {
    bf16x8 oh, ol;
    split8(w.m, oh, ol);
    hi[o] = oh;
    lo[o] = ol;
}
// The window of ONE fp16 plane: the maximum of fp16 values is one of them, so the window works on the packed values
// (v_pk_max_f16: 4 instructions per 8 channels and tap, 4 registers per row maximum) and the output is exact.
// v_pk_max_f16 drops a NaN like fmaxf, and max_pool2d keeps it: beside the maximum the window carries a = fma(x, 0, a), +0 until a
// value is NaN (v_pk_fma_f16: one more instruction per tap; the magnitude bits through v_pk_max_u16 cost two and 46 us per 32 clips),
// and the output is m | a: the maximum's own bits, or a NaN.  An infinity in the window gives NaN as well (inf x 0) where max_pool2d
// returns it or, for -inf, a finite maximum: the plane holds one only after an fp16 overflow, and either way the output is not finite.
typedef __attribute__((ext_vector_type(8))) short i16x8;
struct PoolWin {
    f16x8 m;           // maximum of the non-NaN values
    f16x8 a;           // +0, or NaN
};
DEV void pool_clear(PoolWin& w) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        w.m[j] = (_Float16)(-INFINITY);
        w.a[j] = (_Float16)0.f;
    }
}
DEV void pool_take(PoolWin& w, f16x8 x, f16x8) {
    f16x8 z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (_Float16)0.f;
    w.m = __builtin_elementwise_max(w.m, x);
    w.a = __builtin_elementwise_fma(x, z, w.a);
}
DEV void pool_merge(PoolWin& w, const PoolWin& o) {
    w.m = __builtin_elementwise_max(w.m, o.m);
    w.a = w.a + o.a;
}
DEV f16x8 pool_value(const PoolWin& w) { return __builtin_bit_cast(f16x8, __builtin_bit_cast(i16x8, w.m) | __builtin_bit_cast(i16x8, w.a)); }
DEV void pool_put(const PoolWin& w, f16x8* hi, f16x8*, size_t o) { hi[o] = pool_value(w); }

template <int KH, int KW, int SH, int SW, int PH, int PW, bool SP>
__global__ __launch_bounds__(256) void k_me_pool(const typename PL<SP>::v8* __restrict__ in_hi, const typename PL<SP>::v8* __restrict__ in_lo,
                                                 typename PL<SP>::v8* __restrict__ out_hi, typename PL<SP>::v8* __restrict__ out_lo, int Bc, int H,
                                                 int W, int C8, int Ho, int Wo, int NY) {
    using Win = std::conditional_t<SP, PoolWinS, PoolWin>;
    constexpr int LO = PL<SP>::N - 1;           // single plane: the lo operand is the hi one again, a dead value
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    const int strips = (Ho + NY - 1) / NY;
    const long long total = (long long)Bc * strips * Wo * C8;
    if (idx >= total) return;
    const int c8 = (int)(idx % C8);
    const int xo = (int)((idx / C8) % Wo);
    const int sy = (int)((idx / ((long long)C8 * Wo)) % strips);
    const int b = (int)(idx / ((long long)C8 * Wo * strips));
    Win none;
    pool_clear(none);
    Win ring[KH];                               // ring[k] = row maximum of input row (next_row - KH + k) over the window's columns, oldest first
    auto row_max = [&](int yy) {
        Win m = none;
        if (yy < 0 || yy >= H) return m;
#pragma unroll
        for (int c = 0; c < KW; ++c) {
            const int xx = xo * SW - PW + c;
            if (xx < 0 || xx >= W) continue;
            const size_t o = (((size_t)b * H + yy) * W + xx) * C8 + c8;
            pool_take(m, in_hi[o], (LO ? in_lo : in_hi)[o]);
        }
        return m;
    };
    const int yo0 = sy * NY, yo1 = min(yo0 + NY, Ho);
#pragma unroll
    for (int k = 0; k < KH; ++k) ring[k] = row_max(yo0 * SH - PH + k);
    for (int yo = yo0; yo < yo1; ++yo) {
        Win m = ring[0];
#pragma unroll
        for (int k = 1; k < KH; ++k) pool_merge(m, ring[k]);
        pool_put(m, out_hi, out_lo, (((size_t)b * Ho + yo) * Wo + xo) * C8 + c8);
        if (yo + 1 < yo1) {              // advance the window by SH input rows
#pragma unroll
            for (int k = 0; k + SH < KH; ++k) ring[k] = ring[k + SH];
#pragma unroll
            for (int k = (KH > SH ? KH - SH : 0); k < KH; ++k) ring[k] = row_max((yo + 1) * SH - PH + k);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// conv4: Conv1d(512 -> 64, k=1) + BatchNorm1d over the flattened (channel, bin) axis.  The planes hold a frame's 512
// features in (bin, channel) order, so the host permutes the weight columns instead of moving data.
// One wave = 32 frames; weights (natural-k fragments [ot][ks], hi then lo) stream from L2.
// Single fp16 plane: the weights stay split (fp16 hi + lo, two products per k-step) - the layer is 1 % of the encoder.
// ---------------------------------------------------------------------------------------------------------
template <bool SP>
__global__ __launch_bounds__(256) void k_me_head(const typename PL<SP>::v8* __restrict__ in_hi, const typename PL<SP>::v8* __restrict__ in_lo,
                                                 const typename PL<SP>::v8* __restrict__ w4, const float* __restrict__ bias_ft,
                                                 float* __restrict__ xf_out, int M) {
    using V8 = typename PL<SP>::v8;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 31, kh = lane >> 5;
    const int tok = (blockIdx.x * 4 + wave) * 32 + n;
    const size_t t = tok < M ? tok : M - 1;
    f32x16 acc[2] = {zero16(), zero16()};
#pragma unroll 4
    for (int ks = 0; ks < 32; ++ks) {
        const V8 bh = in_hi[t * 64 + 2 * ks + kh];
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) {
            const V8 ah = w4[(ot * 32 + ks) * 64 + lane], al = w4[(64 + ot * 32 + ks) * 64 + lane];
            if constexpr (SP) {
                acc[ot] = mma3(ah, al, bh, in_lo[t * 64 + 2 * ks + kh], acc[ot]);
            } else {
                acc[ot] = mfma(ah, bh, acc[ot]);
                acc[ot] = mfma(al, bh, acc[ot]);
            }
        }
    }
    if (tok >= M) return;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[ot][4 * q + e] + bias_ft[(ot * 2 + kh) * 16 + 4 * q + e];
            *reinterpret_cast<f32x4*>(xf_out + (size_t)tok * 64 + 32 * ot + 8 * q + 4 * kh) = v;
        }
}

// proj: Linear(64 -> 64) on the fp32 features (transformer.py:457), operands split in registers.
__global__ __launch_bounds__(256) void k_me_proj(const float* __restrict__ xf, const bf16x8* __restrict__ wp,
                                                 const float* __restrict__ bias_ft, float* __restrict__ xf_proj, int M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int n = lane & 31, kh = lane >> 5;
    const int tok = (blockIdx.x * 4 + wave) * 32 + n;
    const size_t t = tok < M ? tok : M - 1;
    f32x16 acc[2] = {zero16(), zero16()};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        float v[8];
        const f32x4 a = *reinterpret_cast<const f32x4*>(xf + t * 64 + 16 * ks + 8 * kh);
        const f32x4 c = *reinterpret_cast<const f32x4*>(xf + t * 64 + 16 * ks + 8 * kh + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            v[e] = a[e];
            v[4 + e] = c[e];
        }
        bf16x8 bh, bl;
        split8(v, bh, bl);
#pragma unroll
        for (int ot = 0; ot < 2; ++ot)
            acc[ot] = mma3(wp[(ot * 4 + ks) * 64 + lane], wp[(8 + ot * 4 + ks) * 64 + lane], bh, bl, acc[ot]);
    }
    if (tok >= M) return;
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[ot][4 * q + e] + bias_ft[(ot * 2 + kh) * 16 + 4 * q + e];
            *reinterpret_cast<f32x4*>(xf_proj + (size_t)tok * 64 + 32 * ot + 8 * q + 4 * kh) = v;
        }
}

// ---- host side ------------------------------------------------------------------------------------------
struct ConvDev {
    const bf16x8* w = nullptr;            // split planes: bf16 hi + lo fragments
    const f16x8* w16 = nullptr;           // single plane: fp16 fragments (conv1.1 ... conv3.1)
    const float *bias = nullptr, *rbias = nullptr;
};

}  // namespace

struct dc_music {
    uint8_t* arena = nullptr;
    ConvDev conv[7];
    const bf16x8 *w4 = nullptr, *wp = nullptr;
    const f16x8* w4_16 = nullptr;         // conv4 as fp16 hi + lo fragments (single-plane format)
    const float *b4 = nullptr, *bp = nullptr;
    const bf16x8* stem_w = nullptr;       // k_me_stem: 22 fragments (conv1.0: hi, lo; conv1.1: 5 hi, 5 lo; conv1.2: 5 hi, 5 lo)
    const f16x8* stem_w16 = nullptr;      // single-plane format: 10 fp16 fragments (conv1.1: 5, conv1.2: 5)
    const float* stem_b = nullptr;        // [3][16] folded biases
    const float* stem_wa = nullptr;       // conv1.0 folded weights [16][9] fp32 (that layer runs on the vector ALU)
    // ping-pong plane pairs, sized for `cap` clips of `cap_tm` mel frames
    bf16x8 *a_hi = nullptr, *a_lo = nullptr, *b_hi = nullptr, *b_lo = nullptr;
    int cap = 0, cap_tm = 0;
    long long ws_bytes = 0;
    int format = 0;                       // 0: split bf16 planes, 1: one fp16 plane (dc_music_set_format)
    bool pinned = false;                  // dc_music_pin_format: `format` holds whatever DC_ME_PREC says
};

std::vector<std::pair<std::string, size_t>> dc_music_required(int music_dim, bool with_proj) {
    std::vector<std::pair<std::string, size_t>> r;
    const std::string me = "music_encoder.";
    for (const MusicConvSpec& c : kMusicConvs) {
        const std::string p = me + c.name;
        r.push_back({p + ".conv2d_layer.0.weight", (size_t)c.cout * c.cin * 9});
        r.push_back({p + ".conv2d_layer.0.bias", (size_t)c.cout});
        for (const char* s : {"weight", "bias", "running_mean", "running_var"}) r.push_back({p + ".conv2d_layer.1." + s, (size_t)c.cout});
        if (c.res_conv) {
            r.push_back({p + ".residual.0.weight", (size_t)c.cout * c.cin});
            r.push_back({p + ".residual.0.bias", (size_t)c.cout});
            for (const char* s : {"weight", "bias", "running_mean", "running_var"}) r.push_back({p + ".residual.1." + s, (size_t)c.cout});
        }
    }
    r.push_back({me + "conv4.0.weight", (size_t)music_dim * 512});
    r.push_back({me + "conv4.0.bias", (size_t)music_dim});
    for (const char* s : {"weight", "bias", "running_mean", "running_var"}) r.push_back({me + "conv4.1." + s, (size_t)music_dim});
    if (with_proj) {
        r.push_back({"proj.weight", (size_t)music_dim * music_dim});
        r.push_back({"proj.bias", (size_t)music_dim});
    }
    return r;
}

bool dc_music_check(const DcParams& params, int music_dim, std::string* err, bool with_proj) {
    if (music_dim != DC_C) {
        *err = "music encoder kernels are built for 64 output channels";
        return false;
    }
    for (const auto& rq : dc_music_required(music_dim, with_proj)) {
        auto it = params.find(rq.first);
        if (it == params.end()) {
            *err = "missing parameter '" + rq.first + "'";
            return false;
        }
        if (it->second.size() != rq.second) {
            *err = "parameter '" + rq.first + "' has the wrong size";
            return false;
        }
    }
    return true;
}

// Folding and packing are music_pack (dc_pack.h, no HIP call); here the image is uploaded and the pointers into it are resolved.
dc_music* dc_music_build(const DcParams& params, int music_dim, std::string* err, bool with_proj) {
    if (!dc_music_check(params, music_dim, err, with_proj)) return nullptr;
    const MusicImage I = music_pack(params, with_proj);
    const std::vector<uint8_t>& host = I.arena.host;
    dc_music* m = new dc_music();
    if (hipMalloc((void**)&m->arena, host.size()) != hipSuccess ||
        hipMemcpy(m->arena, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) {
        *err = "device allocation/upload of the music encoder weights failed";
        dc_music_destroy(m);
        return nullptr;
    }
    m->ws_bytes = (long long)host.size();
    const auto at = [&](auto& dst, size_t off) { dst = reinterpret_cast<std::remove_reference_t<decltype(dst)>>(m->arena + off); };
    for (int i = 0; i < 7; ++i) {
        at(m->conv[i].w, I.conv[i].w);
        at(m->conv[i].w16, I.conv[i].w16);
        at(m->conv[i].bias, I.conv[i].bias);
        if (I.conv[i].rbias != MusicImage::kNone) at(m->conv[i].rbias, I.conv[i].rbias);
    }
    at(m->stem_w, I.stem_w);
    at(m->stem_w16, I.stem_w16);
    at(m->stem_b, I.stem_b);
    at(m->stem_wa, I.stem_wa);
    at(m->w4, I.w4);
    at(m->w4_16, I.w4_16);
    at(m->b4, I.b4);
    if (with_proj) {
        at(m->wp, I.wp);
        at(m->bp, I.bp);
    }
    return m;
}

void dc_music_destroy(dc_music* m) {
    if (!m) return;
    for (void* p : {(void*)m->arena, (void*)m->a_hi, (void*)m->a_lo, (void*)m->b_hi, (void*)m->b_lo})
        if (p) hipFree(p);
    delete m;
}

int dc_music_frames(int Tm) { return (Tm - 1) / 3 + 1; }   // max_pool2d (5,5), stride 3, padding 2 along time
long long dc_music_workspace_bytes(const dc_music* m) { return m ? m->ws_bytes : 0; }

namespace {

#define ME_TRY(x)                         \
    do {                                  \
        hipError_t e_ = (x);              \
        if (e_ != hipSuccess) return e_;  \
    } while (0)

// a plane pair in HBM (single plane: lo = nullptr), its element view for the kernels' stores, and a format's copy of a weight held in both
template <bool SP>
struct Planes {
    typename PL<SP>::v8 *hi, *lo;
};
template <bool SP>
typename PL<SP>::e* elems(typename PL<SP>::v8* p) { return reinterpret_cast<typename PL<SP>::e*>(p); }
template <bool SP>
auto frags(const bf16x8* w, const f16x8* w16) {
    if constexpr (SP) return w; else return w16;
}

// Every launcher: the mel has 128 bins, so W is 128, 64 or 32 and a multiple of the kernel's tile width; any other W is an error.
hipError_t launch_conv10(hipStream_t st, const ConvDev& c, const float* mel, const Planes<true>& out, int Bc, int H, int W) {
    constexpr int TPW = 4;
    if (W % 32 != 0) return hipErrorInvalidValue;
    const long long tiles = (long long)Bc * H * (W / 32);
    const unsigned grid = (unsigned)((tiles + 4 * TPW - 1) / (4 * TPW));
    k_me_conv10<<<dim3(grid), dim3(256), 2 * 1024, st>>>(mel, elems<true>(out.hi), elems<true>(out.lo), c.w, c.bias, Bc, H, W, TPW);
    return hipGetLastError();
}
// LDS-tiled form (CIN >= 16)
template <int CIN, int COUT, int RES, int ROWS, int NXS, bool SP>
hipError_t launch_conv_t(hipStream_t st, const ConvDev& c, const Planes<SP>& in, const Planes<SP>& out, int Bc, int H, int W) {
    constexpr int NPL = PL<SP>::N, KC = CIN / 16, NF = NPL * (9 * KC + (RES == 2 ? KC : 0));
    constexpr int NP = NPL * KC * 2 * (ROWS + 2) * (32 * NXS + 2), NDMA = (NP + 63) / 64;
    constexpr int SHM = (NF + NDMA) * 1024;
    static unsigned long long optin = 0;
    int ncu = 0;
    ME_TRY(dc_cu_count(&ncu));
    if (W % (32 * NXS) != 0) return hipErrorInvalidValue;
    const auto fn = k_me_conv_t<CIN, COUT, RES, ROWS, NXS, SP>;
    ME_TRY(dc_lds_optin((const void*)fn, SHM, optin));
    const long long ntiles = (long long)Bc * ((H + ROWS - 1) / ROWS) * (W / (32 * NXS));
    const unsigned grid = (unsigned)std::min<long long>(ntiles, 2LL * ncu);
    fn<<<dim3(grid), dim3(256), SHM, st>>>(in.hi, in.lo, elems<SP>(out.hi), elems<SP>(out.lo), frags<SP>(c.w, c.w16), c.bias, c.rbias, H, W,
                                           (int)ntiles);
    return hipGetLastError();
}
// conv1.0 -> conv1.1 -> conv1.2 fused (W a multiple of 64); DC_ME_NO_STEM=1 keeps the three separate launches (split planes only)
template <bool SP>
hipError_t launch_stem(hipStream_t st, const dc_music* m, const float* mel, const Planes<SP>& out, int Bc, int H, int W) {
    constexpr int ROWS = 8, TX = 64, NPL = PL<SP>::N;
    constexpr int NBP = ((ROWS + 2) * (TX + 2) + 15) / 16 * 16;
    constexpr int SHM = 2 * NPL * (ROWS + 4) * (TX + 4) * 16 + 2 * NPL * NBP * 16 + (ROWS + 6) * (TX + 6) * 4 + (SP ? 0 : 144 * 4);
    static unsigned long long optin = 0;
    int ncu = 0;
    ME_TRY(dc_cu_count(&ncu));
    if (W % TX != 0) return hipErrorInvalidValue;
    ME_TRY(dc_lds_optin((const void*)k_me_stem<ROWS, TX, SP>, SHM, optin));
    const long long ntiles = (long long)Bc * ((H + ROWS - 1) / ROWS) * (W / TX);
    const unsigned grid = (unsigned)std::min<long long>(ntiles, (SP ? 1 : 2) * (long long)ncu);
    k_me_stem<ROWS, TX, SP><<<dim3(grid), dim3(512), SHM, st>>>(mel, elems<SP>(out.hi), elems<SP>(out.lo), frags<SP>(m->stem_w, m->stem_w16),
                                                                m->stem_b, m->stem_wa, H, W, (int)ntiles);
    return hipGetLastError();
}
// conv2.0 -> conv2.1 fused (W a multiple of 32); DC_ME_NO_MID=1 keeps the two separate launches (split planes only)
template <bool SP>
hipError_t launch_mid(hipStream_t st, const dc_music* m, const Planes<SP>& in, const Planes<SP>& out, int Bc, int H, int W) {
    constexpr int ROWS = 8, TX = 32, NPL = PL<SP>::N;
    constexpr int NPA = 2 * NPL * (ROWS + 4) * (TX + 4), NDMA = (NPA + 63) / 64, NBP = ((ROWS + 2) * (TX + 2) + 15) / 16 * 16;
    constexpr int SHM = 28 * NPL * 1024 + NDMA * 1024 + 4 * NPL * NBP * 16 + (SP ? 0 : 96 * 4);
    static unsigned long long optin = 0;
    int ncu = 0;
    ME_TRY(dc_cu_count(&ncu));
    if (W % TX != 0) return hipErrorInvalidValue;
    ME_TRY(dc_lds_optin((const void*)k_me_mid<ROWS, TX, SP>, SHM, optin));
    const long long ntiles = (long long)Bc * ((H + ROWS - 1) / ROWS) * (W / TX);
    const unsigned grid = (unsigned)std::min<long long>(ntiles, (SP ? 1 : 2) * (long long)ncu);
    const ConvDev &c0 = m->conv[3], &c1 = m->conv[4];
    k_me_mid<ROWS, TX, SP><<<dim3(grid), dim3(512), SHM, st>>>(in.hi, in.lo, elems<SP>(out.hi), elems<SP>(out.lo), frags<SP>(c0.w, c0.w16), c0.bias,
                                                               c0.rbias, frags<SP>(c1.w, c1.w16), c1.bias, H, W, (int)ntiles);
    return hipGetLastError();
}
constexpr int kPoolNY = 24;                // output rows per thread: (NY + KH - 1) / NY of the minimum input traffic (3 ... 24: same time)
template <int KH, int KW, int SH, int SW, int PH, int PW, bool SP>
hipError_t launch_pool(hipStream_t st, const Planes<SP>& in, const Planes<SP>& out, int Bc, int H, int W, int C, int Ho, int Wo) {
    // (DC_ME_POOL_NY: diagnostic of the single-plane pools.  Rows per thread 6 / 12 / 24 / 48 / 96: the three pools together 719 / 730 / 682 / 805 / 1 116 us per 32 clips)
    static const int NY16 = getenv("DC_ME_POOL_NY") ? std::max(1, atoi(getenv("DC_ME_POOL_NY"))) : kPoolNY;
    const int NY = SP ? kPoolNY : NY16;
    const long long total = (long long)Bc * ((Ho + NY - 1) / NY) * Wo * (C / 8);
    k_me_pool<KH, KW, SH, SW, PH, PW, SP><<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st>>>(in.hi, in.lo, out.hi, out.lo, Bc, H, W, C / 8,
                                                                                                     Ho, Wo, NY);
    return hipGetLastError();
}

// One pass: Bc clips of Tm mel frames through the encoder in format SP, the activations ping-ponging between the plane pairs a and b
// (single plane: the hi buffers, half of each is used).  xp may be null.
template <bool SP>
hipError_t encode_pass(hipStream_t st, const dc_music* m, const float* mel, int Bc, int Tm, float* xo, float* xp) {
    using V8 = typename PL<SP>::v8;
    const int T = dc_music_frames(Tm);
    Planes<SP> a{reinterpret_cast<V8*>(m->a_hi), SP ? reinterpret_cast<V8*>(m->a_lo) : nullptr};
    Planes<SP> b{reinterpret_cast<V8*>(m->b_hi), SP ? reinterpret_cast<V8*>(m->b_lo) : nullptr};
    if (!(SP && getenv("DC_ME_NO_STEM"))) {
        ME_TRY(launch_stem<SP>(st, m, mel, a, Bc, Tm, 128));
    } else if constexpr (SP) {
        ME_TRY(launch_conv10(st, m->conv[0], mel, a, Bc, Tm, 128));
        ME_TRY((launch_conv_t<16, 16, 1, 8, 2, SP>(st, m->conv[1], a, b, Bc, Tm, 128)));
        ME_TRY((launch_conv_t<16, 16, 1, 8, 2, SP>(st, m->conv[2], b, a, Bc, Tm, 128)));
    }
    ME_TRY((launch_pool<5, 5, 1, 2, 2, 2, SP>(st, a, b, Bc, Tm, 128, 16, Tm, 64)));
    if (!(SP && getenv("DC_ME_NO_MID"))) {
        ME_TRY(launch_mid<SP>(st, m, b, a, Bc, Tm, 64));
    } else if constexpr (SP) {
        ME_TRY((launch_conv_t<16, 32, 2, 8, 2, SP>(st, m->conv[3], b, a, Bc, Tm, 64)));
        ME_TRY((launch_conv_t<32, 32, 1, 8, 1, SP>(st, m->conv[4], a, b, Bc, Tm, 64)));
        std::swap(a, b);        // two launches leave conv2.1's output where one leaves its input
    }
    ME_TRY((launch_pool<5, 5, 3, 2, 2, 2, SP>(st, a, b, Bc, Tm, 64, 32, T, 32)));
    ME_TRY((launch_conv_t<32, 32, 1, 8, 1, SP>(st, m->conv[5], b, a, Bc, T, 32)));
    ME_TRY((launch_conv_t<32, 32, 1, 8, 1, SP>(st, m->conv[6], a, b, Bc, T, 32)));
    ME_TRY((launch_pool<3, 3, 1, 2, 1, 1, SP>(st, b, a, Bc, T, 32, 32, T, 16)));
    const int M = Bc * T;
    const unsigned grid = (unsigned)((M + 127) / 128);
    k_me_head<SP><<<dim3(grid), dim3(256), 0, st>>>(a.hi, a.lo, frags<SP>(m->w4, m->w4_16), m->b4, xo, M);
    ME_TRY(hipGetLastError());
    if (xp) {
        k_me_proj<<<dim3(grid), dim3(256), 0, st>>>(xo, m->wp, m->bp, xp, M);
        ME_TRY(hipGetLastError());
    }
    return hipSuccess;
}

}  // namespace

// plane format of this encoder's next dc_music_encode calls: 0 = split bf16 planes (~6e-6), 1 = one fp16 plane (~4e-4, about half the
// time); DC_ME_PREC=f16 | split (read per call) overrides it
void dc_music_set_format(dc_music* m, int single_fp16) {
    if (m) m->format = single_fp16 ? 1 : 0;
}
void dc_music_pin_format(dc_music* m, int single_fp16) {
    if (!m) return;
    m->format = single_fp16 ? 1 : 0;
    m->pinned = true;
}
int dc_music_format(const dc_music* m) {
    if (m && m->pinned) return m->format;
    if (const char* e = getenv("DC_ME_PREC")) return (!strcmp(e, "f16") || !strcmp(e, "fp16")) ? 1 : 0;
    return m ? m->format : 0;
}

hipError_t dc_music_encode(dc_music* m, const float* d_mel, int B, int Tm, float* d_xf_proj, float* d_xf_out, hipStream_t st,
                           std::string* err) {
    const int T = dc_music_frames(Tm);
    if (d_xf_proj && !m->wp) {
        *err = "this music encoder was built without proj";
        return hipErrorInvalidValue;
    }
    // chunk of clips whose largest activation (16 channels x Tm x 128 bins, two bf16 planes) stays under ~1.4 GB per buffer (32 clips of 60 s in one pass: 4.5 ms; 16 per pass: 4.7 ms, 8: 5.0 ms)
    int chunk = std::max(1, std::min(B, 32 * 5400 / std::max(Tm, 1)));
    if (const char* e = getenv("DC_ME_CHUNK")) chunk = std::max(1, std::min(B, atoi(e)));
    if (chunk > m->cap || Tm > m->cap_tm) {
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        const int ncap = std::max(chunk, m->cap), ntm = std::max(Tm, m->cap_tm);
        const size_t plane = (size_t)ncap * ntm * 128 * 16 * 2;
        for (bf16x8** p : {&m->a_hi, &m->a_lo, &m->b_hi, &m->b_lo}) {
            if (*p) hipFree(*p);
            *p = nullptr;
            if ((e = hipMalloc((void**)p, plane)) != hipSuccess) {
                *err = "activation plane allocation failed";
                m->cap = m->cap_tm = 0;
                return e;
            }
        }
        m->ws_bytes += 4 * (long long)plane - 4LL * m->cap * m->cap_tm * 128 * 16 * 2;
        m->cap = ncap;
        m->cap_tm = ntm;
    }
    const auto pass = dc_music_format(m) ? encode_pass<false> : encode_pass<true>;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const size_t f0 = (size_t)b0 * T * 64;
        ME_TRY(pass(st, m, d_mel + (size_t)b0 * Tm * 128, std::min(chunk, B - b0), Tm, d_xf_out + f0, d_xf_proj ? d_xf_proj + f0 : nullptr));
    }
    return hipSuccess;
}
#undef ME_TRY
