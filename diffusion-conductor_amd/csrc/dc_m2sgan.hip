// dc_m2sgan.hip - the M2S-GAN generator, the baseline the diffusion denoiser is compared against, on gfx950 (MI355X).
//
// Reference (restated, not translated): Contrastive_Stage/models/Generator.py:52-77 in eval mode,
//   hx     = music_encoder(mel)                               [B, T, 64]    MusicEncoder.py:30-53 - dc_music.hip, split format, pinned
//   hnoise = noise_BN(noise_convTranspose(noise^T))^T         [B, T, 64]    four ConvTranspose1d + ReLU, Ln -> Ln -> 5 Ln -> 15 Ln -> 30 Ln
//   feat   = cat(hx, hnoise)                                  [B, T, 128]   Generator.features
//   pose   = fc(TCN.linear(six TemporalBlocks(feat)))         [B, T, 26]    models/TCN.py:19-86, Generator.py:34-49
// A TemporalBlock with dilation d = 2^i (TCN.py:19-52): two weight-normed Conv1d(kernel 5, dilation d, reflection padding 4 d)
// each followed by Chomp1d(4 d) (2 d frames off each end), BatchNorm and ReLU - net effect y[t] = b + sum_j W[:, :, j] x[rho(t + (j - 2) d)]
// with rho the reflection about the clip's ends -, then AvgPool1d(3, 1, 1) (zero padded, always / 3), + residual, ReLU.
//
// Kernels (all products of the blocks and the head on v_mfma_f32_32x32x2_f32: exact fp32, one k-ordered fmaf chain per output):
//   k_gan_conv<CIN, DOWN, false>  conv1 of a block: one wave = 32 frames of ONE clip x all 64 output channels (two accumulator
//                                 tiles).  K = 5 CIN, tap-major: per tap the lane loads the row of its source frame rho(t + (j - 2) d)
//                                 - computed from the frame's index inside its own clip, never from the tile - as float4s and picks
//                                 channel 2 ks + (l >> 5) per k-step; the folded weights come lane-major from L2, both tiles in one
//                                 8-byte load (dc_pack.h, gan_pack_frags2).  Epilogue: + bias, ReLU.  DOWN (block 0): the 1x1
//                                 downsample rides on the centre tap's rows into two more tiles -> the residual plane.
//   k_gan_conv<64, false, true>   conv2 of a block with the pool, the residual and the last ReLU: a wave computes 32 frames
//                                 t0 - 1 .. t0 + 30 and writes the inner 30 (a one-frame halo each side: the pool's neighbours come
//                                 from lanes l -+ 1; frames outside the clip count as the pool's zero padding).
//   k_gan_head                    TCN.linear and the three fc layers chained in registers, as k_m2s_head (dc_m2snet.hip), sigmoid.
//   k_gan_convt                   the noise branch on the vector ALU, one thread per output element; the last launch applies noise_BN
//                                 behind the ReLU and writes channels 64 .. 127 of feat while it copies hx into channels 0 .. 63.
// Launches per chunk of <= 32 clips: decode 13 (2 per block + head), features = the music encoder's + 4.  No atomics, no LDS, no
// reduction across lanes or clips: a clip's poses are bit-identical in any batch and on every rerun.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "dc_common.h"
#include "dc_handle.h"
#include "dc_mfma_f32.h"

namespace {

using namespace dc_f32;

constexpr int G_WAVES = 4;                 // waves (frame tiles of one clip) per workgroup
constexpr int G_CHUNK = 32;                // clips per pass (bounds the workspace: 32 x T x 448 floats + the noise branch's planes)
constexpr int G_MIN_T = 129;               // block 5 reflects 128 frames: PyTorch's reflection padding needs T > 128

// reflection about a clip's ends; one fold is enough for |offset| <= 64 < T
DEV int reflect(int p, int T) {
    p = p < 0 ? -p : p;
    return p >= T ? 2 * (T - 1) - p : p;
}

// x [clips][T][CIN] -> out [clips][T][64] (see the head of the file).  !POOL: out = relu(conv(x) + b); DOWN: res_out = Wd x + bd as
// well.  POOL: out = relu(avgpool3(relu(conv(x) + b)) + res), res [clips][T][64].
template <int CIN, bool DOWN, bool POOL>
__global__ __launch_bounds__(64 * G_WAVES) void k_gan_conv(const float* __restrict__ x, const float* __restrict__ W, const float* __restrict__ bias,
                                                          const float* __restrict__ Wd, const float* __restrict__ bd,
                                                          const float* __restrict__ res, float* __restrict__ out,
                                                          float* __restrict__ res_out, int T, int d) {
    constexpr int STEP = POOL ? 30 : 32, CH = CIN / 64;
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int first = (blockIdx.x * G_WAVES + (threadIdx.x >> 6)) * STEP;      // first frame this wave writes
    if (first >= T) return;              // wave-uniform; no barriers below
    const int t = first + j - (POOL ? 1 : 0);
    const bool inside = t >= 0 && t < T;
    const int tc = t < 0 ? 0 : (t < T ? t : T - 1);      // (frames outside the clip compute on an end frame and are dropped)
    const size_t clip = (size_t)blockIdx.y * T;
    const float* xb = x + clip * CIN;
    const float2* w2 = reinterpret_cast<const float2*>(W) + lane;
    const float2* wd2 = reinterpret_cast<const float2*>(Wd) + lane;
    f32x16 a0 = {}, a1 = {}, r0 = {}, r1 = {};
#pragma unroll 1
    for (int tap = 0; tap < 5; ++tap) {
        const float* row = xb + (size_t)reflect(tc + (tap - 2) * d, T) * CIN;
#pragma unroll 1
        for (int cc = 0; cc < CH; ++cc) {
            f32x4 m[16];
            load_row64(row + cc * 64, m);
            const float2* wq = w2 + (size_t)(tap * CH + cc) * 32 * 64;
#pragma unroll
            for (int ks = 0; ks < 32; ++ks) {
                const float v = row_operand(m, ks, h);      // channel 64 cc + 2 ks + h
                const float2 ww = wq[ks * 64];
                a0 = mfma2(ww.x, v, a0);
                a1 = mfma2(ww.y, v, a1);
            }
            if (DOWN && tap == 2) {      // the centre tap's rows are the block's input at the wave's own frames
                const float2* wq = wd2 + (size_t)cc * 32 * 64;
#pragma unroll
                for (int ks = 0; ks < 32; ++ks) {
                    const float v = row_operand(m, ks, h);
                    const float2 ww = wq[ks * 64];
                    r0 = mfma2(ww.x, v, r0);
                    r1 = mfma2(ww.y, v, r1);
                }
            }
        }
    }
    // accumulator register r of lane (j, h) = channel (r & 3) + 8 (r >> 2) + 4 h (+ 32 in the second tile): float4 groups of a row
    const size_t o = (clip + tc) * 64 + 4 * h;
    const bool keep = POOL ? (j >= 1 && j <= 30 && inside) : inside;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 y0, y1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = tile_channel(4 * q + e, h);
            y0[e] = relu(a0[4 * q + e] + bias[c]);
            y1[e] = relu(a1[4 * q + e] + bias[c + 32]);
        }
        if (POOL) {
            const f32x4 s0 = *reinterpret_cast<const f32x4*>(res + o + 8 * q), s1 = *reinterpret_cast<const f32x4*>(res + o + 8 * q + 32);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float c0 = inside ? y0[e] : 0.f, c1 = inside ? y1[e] : 0.f;      // AvgPool1d's zero padding (count_include_pad)
                const float p0 = (__shfl_up(c0, 1) + c0 + __shfl_down(c0, 1)) / 3.f;
                const float p1 = (__shfl_up(c1, 1) + c1 + __shfl_down(c1, 1)) / 3.f;
                y0[e] = relu(p0 + s0[e]);
                y1[e] = relu(p1 + s1[e]);
            }
        }
        if (keep) {
            *reinterpret_cast<f32x4*>(out + o + 8 * q) = y0;
            *reinterpret_cast<f32x4*>(out + o + 8 * q + 32) = y1;
        }
        if (DOWN && keep) {
            f32x4 d0, d1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = tile_channel(4 * q + e, h);
                d0[e] = r0[4 * q + e] + bd[c];
                d1[e] = r1[4 * q + e] + bd[c + 32];
            }
            *reinterpret_cast<f32x4*>(res_out + o + 8 * q) = d0;
            *reinterpret_cast<f32x4*>(res_out + o + 8 * q + 32) = d1;
        }
    }
}

// hidden [clips][T][64] -> pose [clips][T][26]: TCN.linear (no activation), fc.0 + ReLU, fc.2 + ReLU, fc.4 + sigmoid.  P: the
// generator's image, hw / hb its head offsets.  Frames >= T of a partial tile compute on frame T - 1 and are not written.
struct GanHead {
    unsigned w[4], b[4];
};
__global__ __launch_bounds__(64 * G_WAVES) void k_gan_head(const float* __restrict__ hid, const float* __restrict__ P, GanHead hd,
                                                          float* __restrict__ pose, int T) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int t0 = (blockIdx.x * G_WAVES + (threadIdx.x >> 6)) * 32;
    if (t0 >= T) return;                 // wave-uniform; no barriers below
    const int t = t0 + j;
    const bool inside = t < T;
    const size_t frame = (size_t)blockIdx.y * T + (inside ? t : T - 1);
    f32x4 m[16];
    load_row64(hid + frame * 64, m);
    const float* w0 = P + hd.w[0];
    f32x16 a0 = {}, a1 = {};
#pragma unroll
    for (int ks = 0; ks < 32; ++ks) {
        const float v = row_operand(m, ks, h);
        a0 = mfma2(w0[ks * 64 + lane], v, a0);
        a1 = mfma2(w0[(32 + ks) * 64 + lane], v, a1);
    }
    add_bias<false>(a0, a1, P + hd.b[0], h);
    f32x16 c0 = {}, c1 = {};
    Layer<0, 32>::run<2, 32>(P + hd.w[1], lane, h, a0, a1, c0, c1);
    add_bias<true>(c0, c1, P + hd.b[1], h);
    f32x16 e0 = {}, e1 = {};
    Layer<0, 32>::run<2, 32>(P + hd.w[2], lane, h, c0, c1, e0, e1);
    add_bias<true>(e0, e1, P + hd.b[2], h);
    f32x16 p0 = {}, p1 = {};
    Layer<0, 32>::run<1, 32>(P + hd.w[3], lane, h, e0, e1, p0, p1);      // 26 rows of one tile
    const float* b = P + hd.b[3];
    if (!inside) return;
    float* dst = pose + frame * 26;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = tile_channel(r, h);
        if (o < 26) dst[o] = 1.f / (1.f + expf(-(p0[r] + b[o])));
    }
}

// One ConvTranspose1d + ReLU of the noise branch, channel-last: x [clips][Lin][cin], w [cin][cout][k] -> y [clips][Lout][ystride]
// at channel yoff + co, Lout = (Lin - 1) stride - 2 pad + k.  y[to][co] = b[co] + sum over (tap, ci) with ti stride - pad + tap = to.
// scale != NULL: scale[co] relu(.) + shift[co] (noise_BN).  copy != NULL ([clips][Lout][64], cout = 64): y's channels 0 .. 63 <- copy.
__global__ __launch_bounds__(256) void k_gan_convt(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                  const float* __restrict__ copy, float* __restrict__ y, int Lin, int Lout, int cin, int cout,
                                                  int k, int stride, int pad, int ystride, int yoff) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= Lout * cout) return;
    const int to = e / cout, co = e - to * cout;
    const float* xb = x + (size_t)blockIdx.y * Lin * cin;
    float acc = bias[co];
    for (int tap = 0; tap < k; ++tap) {
        const int n = to + pad - tap;
        if (n < 0 || n % stride) continue;
        const int ti = n / stride;
        if (ti >= Lin) continue;
        for (int ci = 0; ci < cin; ++ci) acc = fmaf(xb[(size_t)ti * cin + ci], w[((size_t)ci * cout + co) * k + tap], acc);
    }
    acc = relu(acc);
    if (scale) acc = fmaf(acc, scale[co], shift[co]);
    const size_t rowi = (size_t)blockIdx.y * Lout + to;
    y[rowi * ystride + yoff + co] = acc;
    if (copy) y[rowi * ystride + co] = copy[rowi * 64 + co];
}

const char* const kWhat = "M2S-GAN";

// `net.N` of a TemporalBlock's nn.Sequential -> the attribute the same module is registered under first (TCN.py:22-38)
std::string unalias(const std::string& k) {
    static const char* const twin[4][2] = {{".net.0.", ".conv1."}, {".net.2.", ".bn1."}, {".net.5.", ".conv2."}, {".net.7.", ".bn2."}};
    if (!starts_with(k, "tcn.TCN.tcn.tcn.network.")) return k;
    for (const auto& t : twin) {
        const size_t p = k.find(t[0]);
        if (p != std::string::npos) return k.substr(0, p) + t[1] + k.substr(p + 7);
    }
    return k;
}

}  // namespace

struct dc_m2sgan {
    int device = 0;
    DcOwnedMusic music;                  // from the generator's own `music_encoder.*` entries
    DcParams params;
    GanImage image;                      // offsets (the floats themselves are dropped after the upload)
    float* d_img = nullptr;
    size_t img_bytes = 0;                // (the image's size follows the decoder choice)
    DcWorkspace ws;
    int decoder = DC_M2SGAN_DECODER_TCN; // dc_m2sgan_set_decoder: NONE = features only (the pose decoder is another handle's)
    bool finalized = false;
};

namespace {

// The one place where workgroup counts and plane sizes come from (B, T).
struct GanPlan {
    int chunk;                           // clips per pass
    unsigned gx32, gx30;                 // workgroups per clip: 32-frame tiles (conv1, head), 30-frame tiles (conv2 + pool)
    size_t plane, noise;                 // floats of one [chunk][T][64] plane; of the noise branch's three intermediate planes
    GanPlan(int B, int T) {
        chunk = B < G_CHUNK ? B : G_CHUNK;
        gx32 = (unsigned)(((T + 31) / 32 + G_WAVES - 1) / G_WAVES);
        gx30 = (unsigned)(((T + 29) / 30 + G_WAVES - 1) / G_WAVES);
        plane = (size_t)chunk * T * 64;
        noise = (size_t)chunk * (T / 30 + 1) * (16 + 5 * 16 + 15 * 32);
    }
    size_t floats() const { return 7 * plane + noise; }      // hx, feat (2 planes), x0, x1, h, res
};

// feat [nb][T][128] -> after n_blocks TemporalBlocks the residual stream [nb][T][64] at *hid (one of the workspace planes)
int blocks_run(dc_m2sgan* g, const GanPlan& pl, const float* feat, int nb, int T, int n_blocks, const float** hid, hipStream_t st) {
    float* xs[2] = {g->ws.p + 3 * pl.plane, g->ws.p + 4 * pl.plane};
    float *hp = g->ws.p + 5 * pl.plane, *rp = g->ws.p + 6 * pl.plane;
    const float* P = g->d_img;
    const GanImage& I = g->image;
    const dim3 g32(pl.gx32, nb), g30(pl.gx30, nb);
    const float* x = feat;
    for (int i = 0; i < n_blocks; ++i) {
        const GanImage::Block& bk = I.block[i];
        float* y = xs[i & 1];
        if (i == 0)
            k_gan_conv<128, true, false><<<g32, 64 * G_WAVES, 0, st>>>(x, P + bk.w1, P + bk.b1, P + I.wd, P + I.bd, nullptr, hp, rp, T, 1);
        else
            k_gan_conv<64, false, false><<<g32, 64 * G_WAVES, 0, st>>>(x, P + bk.w1, P + bk.b1, nullptr, nullptr, nullptr, hp, nullptr, T, 1 << i);
        k_gan_conv<64, false, true><<<g30, 64 * G_WAVES, 0, st>>>(hp, P + bk.w2, P + bk.b2, nullptr, nullptr, i == 0 ? rp : x, y, nullptr, T, 1 << i);
        x = y;
    }
    DC_HIP_TRY(hipGetLastError());
    *hid = x;
    return DC_OK;
}

int decode_run(dc_m2sgan* g, const GanPlan& pl, const float* feat, int nb, int T, float* pose, hipStream_t st) {
    const float* hid = nullptr;
    if (const int rc = blocks_run(g, pl, feat, nb, T, kGanBlocks, &hid, st)) return rc;
    GanHead hd;
    for (int i = 0; i < 4; ++i) hd.w[i] = (unsigned)g->image.hw[i], hd.b[i] = (unsigned)g->image.hb[i];
    k_gan_head<<<dim3(pl.gx32, nb), 64 * G_WAVES, 0, st>>>(hid, g->d_img, hd, pose, T);
    DC_HIP_TRY(hipGetLastError());
    return DC_OK;
}

// mel [nb][Tm][128], noise [nb][Ln][8] -> feat [nb][T][128]
int features_run(dc_m2sgan* g, const GanPlan& pl, const float* mel, int nb, int Tm, const float* noise, int Ln, int T, float* feat,
                 hipStream_t st) {
    float* hx = g->ws.p;
    if (const int rc = g->music.encode(kWhat, mel, nb, Tm, hx, st)) return rc;
    float* np = g->ws.p + 7 * pl.plane;
    float* planes[3] = {np, np + (size_t)nb * Ln * 16, np + (size_t)nb * Ln * (16 + 5 * 16)};
    const float* P = g->d_img;
    const GanImage& I = g->image;
    const float* x = noise;
    int L = Ln;
    for (int i = 0; i < 4; ++i) {
        const GanConvT& c = kGanNoise[i];
        const int Lout = (L - 1) * c.stride - 2 * c.pad + c.k;
        const bool last = i == 3;
        float* y = last ? feat : planes[i];
        k_gan_convt<<<dim3((unsigned)((Lout * c.cout + 255) / 256), nb), 256, 0, st>>>(
            x, P + I.nw[i], P + I.nb[i], last ? P + I.nscale : nullptr, last ? P + I.nshift : nullptr, last ? hx : nullptr, y, L, Lout, c.cin,
            c.cout, c.k, c.stride, c.pad, last ? 128 : c.cout, last ? 64 : 0);
        x = y;
        L = Lout;
    }
    DC_HIP_TRY(hipGetLastError());
    return DC_OK;
}

// the shape rules every entry point shares; Tm < 0: no mel (decode), Ln < 0: no latent.  A features-only handle has no decoder
// to call and no temporal block whose reflection bounds T.
int check_shapes(const char* fn, const dc_m2sgan* g, int B, int Tm, int Ln, int T) {
    const std::string f(fn);
    if (!g->finalized) return dc_set_error(DC_ERR_INVALID, (f + " before dc_m2sgan_finalize").c_str());
    const bool tcn = g->decoder == DC_M2SGAN_DECODER_TCN;
    if (!tcn && f != "dc_m2sgan_features")
        return dc_set_error(DC_ERR_INVALID, (f + ": this generator was finalized without a decoder (dc_m2sgan_set_decoder); it computes features only").c_str());
    if (B < 1) return dc_set_error(DC_ERR_INVALID, (f + ": B must be >= 1").c_str());
    if (Tm >= 0 && Tm < 4) return dc_set_error(DC_ERR_INVALID, (f + ": need at least 4 mel frames (the encoder's reflection padding)").c_str());
    if (Tm >= 0 && T != dc_music_frames(Tm))
        return dc_set_error(DC_ERR_INVALID, (f + ": " + std::to_string(Tm) + " mel frames make " + std::to_string(dc_music_frames(Tm)) +
                                             " frames, not " + std::to_string(T)).c_str());
    if (Ln >= 0 && (Ln < 1 || T != 30 * Ln))
        return dc_set_error(DC_ERR_INVALID, (f + ": a latent of " + std::to_string(Ln) + " steps makes " + std::to_string(30 * (long long)Ln) +
                                             " frames, the music has " + std::to_string(T)).c_str());
    if (tcn && T < G_MIN_T)
        return dc_set_error(DC_ERR_INVALID, (f + ": " + std::to_string(T) + " frames; the last temporal block reflects 128 frames and needs T > 128").c_str());
    return DC_OK;
}

}  // namespace

extern "C" {

int dc_m2sgan_create(int32_t device, dc_m2sgan** out) {
    if (!out) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_create: out is NULL");
    *out = nullptr;
    if (const int rc = dc_check_device("dc_m2sgan_create", device)) return rc;
    auto* g = new dc_m2sgan;
    g->device = device;
    *out = g;
    return DC_OK;
}

void dc_m2sgan_destroy(dc_m2sgan* g) {
    if (!g) return;
    const DcDeviceGuard on(g->device);
    g->music.release();
    if (g->d_img) (void)hipFree(g->d_img);
    g->ws.release();
    delete g;
}

int dc_m2sgan_set_param(dc_m2sgan* g, const char* name, const float* h_data, int64_t numel) {
    if (!g || !name || !h_data) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_set_param: NULL argument");
    const std::string given(name), k = unalias(given);
    bool changed = false;
    // a `net.N.*` alias (k != given) is the same tensor as its conv / bn twin, which is the parameter: checked and dropped
    const DcParamList used = g->decoder == DC_M2SGAN_DECODER_TCN ? gan_required() : gan_required_features();
    const int rc = starts_with(k, "music_encoder.") ? g->music.take(kWhat, kGanC, k, h_data, numel, &changed)
                                                    : dc_param_take(kWhat, used, {}, k, given, h_data, numel, k == given ? &g->params : nullptr, &changed);
    if (changed) g->finalized = false;
    return rc;
}

int dc_m2sgan_set_decoder(dc_m2sgan* g, int32_t decoder) {
    if (!g) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_set_decoder: NULL handle");
    if (decoder != DC_M2SGAN_DECODER_TCN && decoder != DC_M2SGAN_DECODER_NONE)
        return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_set_decoder: decoder must be DC_M2SGAN_DECODER_TCN or DC_M2SGAN_DECODER_NONE");
    if (decoder != g->decoder) g->finalized = false;
    g->decoder = decoder;
    return DC_OK;
}

int dc_m2sgan_finalize(dc_m2sgan* g) {
    if (!g) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_finalize: NULL handle");
    g->finalized = false;
    const bool tcn = g->decoder == DC_M2SGAN_DECODER_TCN;
    if (!tcn)
        for (const auto& e : g->params)
            if (starts_with(e.first, "tcn."))
                return dc_set_error(DC_ERR_PARAM, (std::string(kWhat) + " parameter " + e.first + " was set, but the generator has no decoder (dc_m2sgan_set_decoder)").c_str());
    if (const int rc = g->music.check(kWhat, kGanC)) return rc;
    if (const int rc = dc_param_complete(kWhat, tcn ? gan_required() : gan_required_features(), g->params)) return rc;
    DC_HIP_TRY(hipSetDevice(g->device));
    if (const int rc = g->music.rebuild(kWhat, kGanC)) return rc;
    g->image = gan_pack(g->params, tcn);
    const size_t bytes = g->image.img.size() * sizeof(float);
    if (g->d_img && g->img_bytes != bytes) {
        DC_HIP_TRY(hipDeviceSynchronize());     // (work of earlier calls may still read the old image)
        DC_HIP_TRY(hipFree(g->d_img));
        g->d_img = nullptr;
    }
    if (!g->d_img) DC_HIP_TRY(hipMalloc((void**)&g->d_img, bytes));
    g->img_bytes = bytes;
    DC_HIP_TRY(hipMemcpy(g->d_img, g->image.img.data(), bytes, hipMemcpyHostToDevice));
    g->image.img = std::vector<float>();
    g->finalized = true;
    return DC_OK;
}

int dc_m2sgan_features(dc_m2sgan* g, const float* d_mel, int32_t B, int32_t Tm, const float* d_noise, int32_t Ln, float* d_feat,
                       void* stream) {
    if (!g || !d_mel || !d_noise || !d_feat) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_features: NULL argument");
    const int T = Tm >= 4 ? dc_music_frames(Tm) : 0;
    if (const int rc = check_shapes("dc_m2sgan_features", g, B, Tm, Ln, T)) return rc;
    DC_HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    const GanPlan pl(B, T);
    if (const int rc = g->ws.reserve(pl.floats(), st)) return rc;
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        return features_run(g, pl, d_mel + (size_t)b0 * Tm * 128, nb, Tm, d_noise + (size_t)b0 * Ln * kGanLatent, Ln, T, d_feat + (size_t)b0 * T * 128, st);
    });
}

int dc_m2sgan_decode(dc_m2sgan* g, const float* d_feat, int32_t B, int32_t T, float* d_pose, void* stream) {
    if (!g || !d_feat || !d_pose) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_decode: NULL argument");
    if (const int rc = check_shapes("dc_m2sgan_decode", g, B, -1, -1, T)) return rc;
    if ((uintptr_t)d_feat & 15) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_decode: the features must be 16-byte aligned");
    DC_HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    const GanPlan pl(B, T);
    if (const int rc = g->ws.reserve(pl.floats(), st)) return rc;
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        return decode_run(g, pl, d_feat + (size_t)b0 * T * 128, nb, T, d_pose + (size_t)b0 * T * kGanPose, st);
    });
}

int dc_m2sgan_generate(dc_m2sgan* g, const float* d_mel, int32_t B, int32_t Tm, const float* d_noise, int32_t Ln, float* d_pose,
                       void* stream) {
    if (!g || !d_mel || !d_noise || !d_pose) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_generate: NULL argument");
    const int T = Tm >= 4 ? dc_music_frames(Tm) : 0;
    if (const int rc = check_shapes("dc_m2sgan_generate", g, B, Tm, Ln, T)) return rc;
    DC_HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    const GanPlan pl(B, T);
    if (const int rc = g->ws.reserve(pl.floats(), st)) return rc;
    float* feat = g->ws.p + pl.plane;
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        if (const int rc = features_run(g, pl, d_mel + (size_t)b0 * Tm * 128, nb, Tm, d_noise + (size_t)b0 * Ln * kGanLatent, Ln, T, feat, st))
            return rc;
        return decode_run(g, pl, feat, nb, T, d_pose + (size_t)b0 * T * kGanPose, st);
    });
}

int dc_m2sgan_debug_blocks(dc_m2sgan* g, const float* d_feat, int32_t B, int32_t T, int32_t n_blocks, float* d_h, void* stream) {
    if (!g || !d_feat || !d_h) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_debug_blocks: NULL argument");
    if (const int rc = check_shapes("dc_m2sgan_debug_blocks", g, B, -1, -1, T)) return rc;
    if (n_blocks < 1 || n_blocks > kGanBlocks) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_debug_blocks: n_blocks must be 1 .. 6");
    if ((uintptr_t)d_feat & 15) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_debug_blocks: the features must be 16-byte aligned");
    DC_HIP_TRY(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)stream;
    const GanPlan pl(B, T);
    if (const int rc = g->ws.reserve(pl.floats(), st)) return rc;
    return dc_chunks(B, pl.chunk, [&](int b0, int nb) -> int {
        const float* hid = nullptr;
        if (const int rc = blocks_run(g, pl, d_feat + (size_t)b0 * T * 128, nb, T, n_blocks, &hid, st)) return rc;
        DC_HIP_TRY(hipMemcpyAsync(d_h + (size_t)b0 * T * 64, hid, (size_t)nb * T * 64 * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DC_OK;
    });
}

int dc_m2sgan_fold_conv(const float* weight_g, const float* weight_v, const float* conv_bias, const float* bn_weight, const float* bn_bias,
                        const float* bn_mean, const float* bn_var, int32_t cout, int32_t cin, int32_t k, float* h_w, float* h_b) {
    if (!weight_g || !weight_v || !conv_bias || !bn_weight || !bn_bias || !bn_mean || !bn_var || !h_w || !h_b)
        return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_fold_conv: NULL argument");
    if (cout < 1 || cin < 1 || k < 1) return dc_set_error(DC_ERR_INVALID, "dc_m2sgan_fold_conv: cout, cin and k must be >= 1");
    gan_fold_conv(weight_g, weight_v, conv_bias, bn_weight, bn_bias, bn_mean, bn_var, cout, cin, k, h_w, h_b);
    return DC_OK;
}

}  // extern "C"
