// dc_mfma_f32.h - device helpers of the exact-fp32 kernels on v_mfma_f32_32x32x2_f32 (dc_stgcn.hip, dc_m2snet.hip, dc_m2sgan.hip, dc_rhythm.hip): one wave = 32
// frames of one clip on the lanes (lane l: frame l & 31, k half l >> 5), the weights as lane-major A fragments read from L2
// (dc_pack.h, head_pack_frags), an accumulator tile handed on as the next layer's B operand.  Every output is one k-ordered fmaf
// chain: no partial sums and no reduction across lanes, so a frame's result depends on that frame's inputs alone.
#pragma once
#include <hip/hip_runtime.h>

#include "dc_common.h"   // DEV, relu, nanmax

namespace dc_f32 {

DEV f32x16 mfma2(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

// the row (channel) of its 32-row tile that accumulator register r of lane half h holds (dc_pack.h's tile_row, on the device)
DEV int tile_channel(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// A lane's frame as a channel-contiguous row of 64 floats (16-byte aligned): 16 float4 loads, then channel 2 ks + h as the B
// operand of k-step ks.  ks must be a constant where this is called (a fully unrolled loop), or m[] goes to scratch.
DEV void load_row64(const float* row, f32x4 (&m)[16]) {
    const f32x4* p = reinterpret_cast<const f32x4*>(row);
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = p[i];
}
DEV float row_operand(const f32x4 (&m)[16], int ks, int h) { return h ? m[ks >> 1][2 * (ks & 1) + 1] : m[ks >> 1][2 * (ks & 1)]; }

// + bias (, ReLU) over a 64-channel activation held as two accumulator tiles (channels 0 .. 31 in lo, 32 .. 63 in hi)
template <bool RELU>
DEV void add_bias(f32x16& lo, f32x16& hi, const float* b, int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = tile_channel(r, h);
        lo[r] = RELU ? relu(lo[r] + b[o]) : lo[r] + b[o];
        hi[r] = RELU ? relu(hi[r] + b[o + 32]) : hi[r] + b[o + 32];
    }
}

// B operand of k-step S (channels 2 S and 2 S + 1) out of a 64-channel activation held as two accumulator tiles (channels
// 0 .. 31 in lo, 32 .. 63 in hi; register r of lane half h = channel (r & 3) + 8 (r >> 2) + 4 h).  Both channels sit in half HC
// of the wave; that half keeps its own and sends the other one across.
template <int S>
DEV float kstep_operand(const f32x16& lo, const f32x16& hi, int h) {
    constexpr int c = (2 * S) & 31, HC = (c >> 2) & 1, r0 = (c & 3) + 4 * (c >> 3), r1 = r0 + 1;
    const f32x16& t = S < 16 ? lo : hi;
    const float own = HC ? t[r1] : t[r0], send = HC ? t[r0] : t[r1];
    const float recv = __shfl_xor(send, 32);
    return h == HC ? own : recv;
}

template <int S0, int N>
struct Layer {
    // acc (+)= W[:, 2 S0 .. 2 (S0 + N)) x;  NMT output tiles, KS k-steps per tile in the fragment image `wf`
    template <int NMT, int KS>
    static DEV void run(const float* __restrict__ wf, int lane, int h, const f32x16& lo, const f32x16& hi, f32x16& acc0, f32x16& acc1) {
        const float x = kstep_operand<S0>(lo, hi, h);
        acc0 = mfma2(wf[S0 * 64 + lane], x, acc0);
        if (NMT == 2) acc1 = mfma2(wf[(KS + S0) * 64 + lane], x, acc1);
        Layer<S0 + 1, N - 1>::template run<NMT, KS>(wf, lane, h, lo, hi, acc0, acc1);
    }
};
template <int S0>
struct Layer<S0, 0> {
    template <int NMT, int KS>
    static DEV void run(const float*, int, int, const f32x16&, const f32x16&, f32x16&, f32x16&) {}
};

}  // namespace dc_f32
