// dc_pack.h - host-only half of the weight preparation (no kernels, no HIP call): 16-bit conversions, the MFMA fragment
// packers, the 256-byte-aligned host arena, the MusicEncoder's folded image, M2SNet's fuse head, the M2S-GAN generator's image, the
// ST-GCN motion encoder's, the M2S-GAN critic's, the Welch table and the mel front end's tables.  Included by dc_api.hip (denoiser
// image, dc_pack_weight), dc_music.hip, dc_m2snet.hip, dc_m2sgan.hip, dc_stgcn.hip, dc_rhythm.hip and dc_mel.hip; the single copy of
// every rounding routine they must agree on bit for bit.
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

// ---- 16-bit conversions (round to nearest even; inputs are finite weights) --------------------------------------------
inline uint16_t f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
inline uint16_t f2h(float f) {   // fp32 -> fp16 bits, round to nearest even (compiler's conversion)
    const _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}
inline float h2f(uint16_t u) {
    _Float16 h;
    memcpy(&h, &u, 2);
    return (float)h;
}
inline uint16_t to16(float v, bool f16) { return f16 ? f2h(v) : f2bf(v); }

inline int tile_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// ---- fragment packers ---------------------------------------------------------------------------------------------
// One MFMA operand fragment - 64 lanes x 8 elements, lane-major (1 KiB per half) - of w [n_out][k_in] (row-major, 0 outside):
// element (l, j) = w[row][col] with (row, col) = at(l, j), split into v ~ hi + lo in the 16-bit format (fp16 or bf16):
// hi = round(v), lo = round(v - hi).  A null `lo` keeps the hi halves only.  Every packer below goes through here.
template <class At>
inline void pack_frag(const float* w, int n_out, int k_in, bool f16, uint16_t* hi, uint16_t* lo, At at) {
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 8; ++j) {
            const std::pair<int, int> rc = at(l, j);
            const float v = (rc.first < n_out && rc.second < k_in) ? w[(size_t)rc.first * k_in + rc.second] : 0.f;
            const uint16_t h = hi[l * 8 + j] = to16(v, f16);
            if (lo) lo[l * 8 + j] = to16(v - (f16 ? h2f(h) : bf2f(h)), f16);
        }
}

// Weight image of v_mfma_f32_32x32x16 operands, lane (i = l&31, hh = l>>5).  "chained" k order: frag (ot, kt, s), element j
//   = W[32ot + i][32kt + 16s + 8(j>>2) + 4hh + (j&3)]
// i.e. the k order in which an accumulator tile, converted in registers, presents its rows; frags [kt][ot][s] (k-outer sweeps).
// "natural" k order: frag (ot, ks): element j = W[32ot + i][16ks + 8hh + j]; frags [ot][ks] (streamed per tile).
inline void pack_weight(const float* w, int n_out, int k_in, bool chained, uint16_t* hi, uint16_t* lo, bool f16 = false) {
    const int OT = cdiv(n_out, 32), KT = cdiv(k_in, 32);
    for (int ot = 0; ot < OT; ++ot)
        for (int kt = 0; kt < KT; ++kt)
            for (int s = 0; s < 2; ++s) {
                const size_t o = 512 * ((chained ? (size_t)kt * OT + ot : (size_t)ot * KT + kt) * 2 + s);
                pack_frag(w, n_out, k_in, f16, hi + o, lo + o, [&](int l, int j) {
                    const int hh = l >> 5, k = chained ? 8 * (j >> 2) + 4 * hh + (j & 3) : 8 * hh + j;
                    return std::make_pair(32 * ot + (l & 31), 32 * kt + 16 * s + k);
                });
            }
}
inline size_t packed_elems(int n_out, int k_in) { return (size_t)cdiv(n_out, 32) * cdiv(k_in, 32) * 2 * 64 * 8; }
// v_mfma_f32_16x16x32 operand image of the 16-token layer kernel (DcLayer16 in dc_common.h): [m][rb][64][8]
inline void pack_weight16(const float* w, int n_out, int k_in, uint16_t* hi, uint16_t* lo, bool f16) {
    const int RB = cdiv(n_out, 16), KM = cdiv(k_in, 32);
    for (int m = 0; m < KM; ++m)
        for (int rb = 0; rb < RB; ++rb) {
            const size_t o = 512 * ((size_t)m * RB + rb);
            pack_frag(w, n_out, k_in, f16, hi + o, lo + o, [&](int l, int j) {
                return std::make_pair(16 * rb + (l & 15), 32 * m + 16 * (j >> 2) + 4 * (l >> 4) + (j & 3));
            });
        }
}
inline size_t packed_elems16(int n_out, int k_in) { return (size_t)cdiv(n_out, 16) * cdiv(k_in, 32) * 64 * 8; }

// The MusicEncoder's natural-k A fragments of Wm [n_out][k_in]: [hi: ot][ks], then [lo: ot][ks] when `with_lo`.  The element
// order is pack_weight's natural one, but the image is sized by k-steps of 16: an odd KS (K = 16, 144) has no padding
// half-tile, so this stays its own function.
inline std::vector<uint16_t> pack_nat(const std::vector<float>& Wm, int n_out, int k_in, int OT, int KS, bool f16, bool with_lo) {
    const size_t ne = (size_t)OT * KS * 512;
    std::vector<uint16_t> out((with_lo ? 2 : 1) * ne, 0);
    for (int ot = 0; ot < OT; ++ot)
        for (int ks = 0; ks < KS; ++ks) {
            uint16_t* hi = out.data() + 512 * ((size_t)ot * KS + ks);
            pack_frag(Wm.data(), n_out, k_in, f16, hi, with_lo ? hi + ne : nullptr,
                      [&](int l, int j) { return std::make_pair(32 * ot + (l & 31), 16 * ks + 8 * (l >> 5) + j); });
        }
    return out;
}

// per-feature vector in FT register order: out[(t*2+hh)*16 + r] = v[32t + tile_row(r,hh)]
inline std::vector<float> ftvec(const float* v, int n, int NT) {
    std::vector<float> out((size_t)NT * 32);
    for (int t = 0; t < NT; ++t)
        for (int hh = 0; hh < 2; ++hh)
            for (int r = 0; r < 16; ++r) {
                const int f = 32 * t + tile_row(r, hh);
                out[(t * 2 + hh) * 16 + r] = f < n ? v[f] : 0.f;
            }
    return out;
}

// FiLM GEMM operands in v_mfma_f32_16x16x32 order (DcModel::film_w16 in dc_common.h): w [32 NT][k] row-major -> [tile][ks32][fb][64][8],
// lane l = row 16 fb + pi(l & 15), element j = column 32 ks32 + 8 (l >> 4) + j; hi halves only
constexpr int kFilmPi[16] = {0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15};
inline std::vector<uint16_t> pack_film16(const std::vector<float>& w, int NT, int k, bool f16) {
    std::vector<uint16_t> out((size_t)NT * 32 * k);
    for (int ot = 0; ot < NT; ++ot)
        for (int ks = 0; ks < k / 32; ++ks)
            for (int fb = 0; fb < 2; ++fb)
                pack_frag(w.data(), NT * 32, k, f16, out.data() + 512 * (((size_t)ot * (k / 32) + ks) * 2 + fb), nullptr, [&](int l, int j) {
                    return std::make_pair(32 * ot + 16 * fb + kFilmPi[l & 15], 32 * ks + 8 * (l >> 4) + j);
                });
    return out;
}
// ... and their constants in the same row order: [tile][fb][16]
inline std::vector<float> permute_film_bias16(const std::vector<float>& b, int NT) {
    std::vector<float> out((size_t)NT * 32);
    for (int ot = 0; ot < NT; ++ot)
        for (int fb = 0; fb < 2; ++fb)
            for (int r = 0; r < 16; ++r) out[((size_t)ot * 2 + fb) * 16 + r] = b[(size_t)32 * ot + 16 * fb + kFilmPi[r]];
    return out;
}

// ---- host arena ---------------------------------------------------------------------------------------------------
// Everything a model keeps on the device, appended at 256-byte alignment.  Pointers into it are known only after the upload:
// point() notes a destination and the arena offset it will hold, resolve() fills every destination in for a base address.
struct Arena {
    std::vector<uint8_t> host;
    std::vector<std::pair<const void**, size_t>> fix;
    size_t add(const void* p, size_t bytes) {
        const size_t off = (host.size() + 255) & ~(size_t)255;
        host.resize(off + bytes);
        memcpy(host.data() + off, p, bytes);
        return off;
    }
    template <class T>
    size_t add(const std::vector<T>& v) { return add(v.data(), v.size() * sizeof(T)); }
    template <class T>
    void point(const T** dst, size_t off) { fix.push_back({(const void**)dst, off}); }
    void resolve(const uint8_t* base) const {
        for (const auto& f : fix) *f.first = base + f.second;
    }
};

using DcParams = std::map<std::string, std::vector<float>>;
using DcParamList = std::vector<std::pair<std::string, size_t>>;      // (name, numel) of state_dict entries

// ---- MusicEncoder image (kernels: dc_music.hip) -------------------------------------------------------------------
struct MusicConvSpec {
    const char* name;
    int cin, cout;
    bool res_conv;
};
constexpr MusicConvSpec kMusicConvs[7] = {{"conv1.0", 1, 16, false},  {"conv1.1", 16, 16, false}, {"conv1.2", 16, 16, false},
                                          {"conv2.0", 16, 32, true},  {"conv2.1", 32, 32, false}, {"conv3.0", 32, 32, false},
                                          {"conv3.1", 32, 32, false}};
constexpr float kBnEps = 1e-5f;   // nn.BatchNorm default

// the folded weights as one arena plus the offsets of its entries (kNone: the layer has no such entry)
struct MusicImage {
    static constexpr size_t kNone = (size_t)-1;
    Arena arena;
    struct Conv {
        size_t w, w16, bias, rbias;       // bf16 hi + lo fragments, fp16 fragments, folded bias, residual branch's bias
    } conv[7];
    size_t w4, w4_16, b4;                 // conv4: bf16 hi + lo, fp16 hi + lo, bias
    size_t stem_w, stem_w16, stem_b, stem_wa;
    size_t wp, bp;                        // proj (kNone when the image was packed without it)
};

// v_mfma_f32_16x16x32 A fragments of the fused conv1 kernel (k_me_stem) for one of its three layers, Wm [16][K]: lane (co = l & 15,
// q4 = l >> 4), element j; bf16 hi and lo, and for the 16-channel layers the fp16 fragments appended to `f16` ([layer][ks][lane][j])
inline void music_pack_stem(const std::vector<float>& Wm, int K, int cin, std::vector<uint16_t>& hi, std::vector<uint16_t>& lo,
                            std::vector<uint16_t>& f16) {
    const int nks = cin == 1 ? 1 : 5;
    hi.assign((size_t)nks * 512, 0);
    lo.assign((size_t)nks * 512, 0);
    for (int ks = 0; ks < nks; ++ks) {
        const auto at = [&](int l, int j) {      // conv1.0: k = tap (9 of 16); else tap-major, 16 channels per tap (tap 9 of k-step 4: past K)
            const int q4 = l >> 4;
            return std::make_pair(l & 15, cin == 1 ? 8 * q4 + j : (2 * ks + (q4 >> 1)) * 16 + 8 * (q4 & 1) + j);
        };
        pack_frag(Wm.data(), 16, K, false, &hi[(size_t)ks * 512], &lo[(size_t)ks * 512], at);
        if (cin == 1) continue;
        f16.resize(f16.size() + 512);
        pack_frag(Wm.data(), 16, K, true, &f16[f16.size() - 512], nullptr, at);
    }
}

// Folds and packs the reference state_dict entries `music_encoder.*` / `proj.*` (all present, with the sizes of
// dc_music_required: dc_music_check).  with_proj = false: the `music_encoder.*` entries alone (M2SNet's encoder has no proj); the
// image is the same up to where proj would be appended.
inline MusicImage music_pack(const DcParams& params, bool with_proj = true) {
    const auto P = [&](const std::string& n) -> const std::vector<float>& { return params.find(n)->second; };
    // eval-mode BatchNorm `bn` folded into the convolution in front of it (bias cb): s = gamma / sqrt(var + eps)
    const auto bn_fold = [&](const std::string& bn, const std::vector<float>& cb, std::vector<float>& scale, std::vector<float>& bias) {
        const auto &g = P(bn + ".weight"), &be = P(bn + ".bias"), &mu = P(bn + ".running_mean"), &var = P(bn + ".running_var");
        scale.resize(g.size());
        bias.resize(g.size());
        for (size_t c = 0; c < g.size(); ++c) {
            scale[c] = g[c] / std::sqrt(var[c] + kBnEps);
            bias[c] = (cb[c] - mu[c]) * scale[c] + be[c];
        }
    };
    MusicImage I;
    Arena& A = I.arena;
    std::vector<uint16_t> stem_hi[3], stem_lo[3], stem_16;
    std::vector<float> stem_bias, stem_wa32;
    const std::string me = "music_encoder.";
    for (int i = 0; i < 7; ++i) {
        const MusicConvSpec& c = kMusicConvs[i];
        const std::string p = me + c.name;
        std::vector<float> sc, bi;
        bn_fold(p + ".conv2d_layer.1", P(p + ".conv2d_layer.0.bias"), sc, bi);
        const auto& w = P(p + ".conv2d_layer.0.weight");                 // [cout][cin][3][3]
        const int K = c.cin >= 16 ? 9 * c.cin : 16, KS = K / 16;
        std::vector<float> Wm((size_t)c.cout * K, 0.f);
        for (int co = 0; co < c.cout; ++co)
            for (int ci = 0; ci < c.cin; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    Wm[(size_t)co * K + tap * c.cin + ci] = w[((size_t)co * c.cin + ci) * 9 + tap] * sc[co];
        std::vector<uint16_t> frags = pack_nat(Wm, c.cout, K, 1, KS, false, true);
        std::vector<uint16_t> frags16 = pack_nat(Wm, c.cout, K, 1, KS, true, false);
        if (i == 0) {                                                    // conv1.0 runs on the vector ALU: [16][9] fp32
            stem_wa32.resize(16 * 9);
            for (int co = 0; co < 16; ++co)
                for (int tap = 0; tap < 9; ++tap) stem_wa32[co * 9 + tap] = Wm[(size_t)co * K + tap];
        }
        if (i < 3) {
            music_pack_stem(Wm, K, c.cin, stem_hi[i], stem_lo[i], stem_16);
            stem_bias.insert(stem_bias.end(), bi.begin(), bi.end());
        }
        std::vector<float> rb;
        if (c.res_conv) {
            std::vector<float> rs;
            bn_fold(p + ".residual.1", P(p + ".residual.0.bias"), rs, rb);
            const auto& rw = P(p + ".residual.0.weight");                // [cout][cin][1][1]
            std::vector<float> Rm((size_t)c.cout * c.cin);
            for (int co = 0; co < c.cout; ++co)
                for (int ci = 0; ci < c.cin; ++ci) Rm[(size_t)co * c.cin + ci] = rw[(size_t)co * c.cin + ci] * rs[co];
            const std::vector<uint16_t> rf = pack_nat(Rm, c.cout, c.cin, 1, c.cin / 16, false, true);
            frags.insert(frags.end(), rf.begin(), rf.end());
            const std::vector<uint16_t> rf16 = pack_nat(Rm, c.cout, c.cin, 1, c.cin / 16, true, false);
            frags16.insert(frags16.end(), rf16.begin(), rf16.end());
        }
        I.conv[i].w = A.add(frags);
        I.conv[i].w16 = A.add(frags16);
        I.conv[i].bias = A.add(ftvec(bi.data(), (int)bi.size(), 1));
        I.conv[i].rbias = c.res_conv ? A.add(ftvec(rb.data(), (int)rb.size(), 1)) : MusicImage::kNone;
    }
    // conv4 + BatchNorm1d; reference feature index c*16 + bin  ->  plane order bin*32 + c
    std::vector<float> s4, b4;
    bn_fold(me + "conv4.1", P(me + "conv4.0.bias"), s4, b4);
    const auto& w4 = P(me + "conv4.0.weight");
    std::vector<float> W4((size_t)64 * 512);
    for (int o = 0; o < 64; ++o)
        for (int c = 0; c < 32; ++c)
            for (int bin = 0; bin < 16; ++bin) W4[(size_t)o * 512 + bin * 32 + c] = w4[(size_t)o * 512 + c * 16 + bin] * s4[o];
    I.w4 = A.add(pack_nat(W4, 64, 512, 2, 32, false, true));
    I.w4_16 = A.add(pack_nat(W4, 64, 512, 2, 32, true, true));
    I.b4 = A.add(ftvec(b4.data(), (int)b4.size(), 2));
    std::vector<uint16_t> stem_frags;
    for (int i = 0; i < 3; ++i) {
        stem_frags.insert(stem_frags.end(), stem_hi[i].begin(), stem_hi[i].end());
        stem_frags.insert(stem_frags.end(), stem_lo[i].begin(), stem_lo[i].end());
    }
    I.stem_w = A.add(stem_frags);
    I.stem_w16 = A.add(stem_16);
    I.stem_b = A.add(stem_bias);
    I.stem_wa = A.add(stem_wa32);
    I.wp = I.bp = MusicImage::kNone;
    if (with_proj) {
        const auto& bp = P("proj.bias");
        I.wp = A.add(pack_nat(P("proj.weight"), 64, 64, 2, 4, false, true));
        I.bp = A.add(ftvec(bp.data(), (int)bp.size(), 2));
    }
    return I;
}

// ---- M2SNet fuse head image (kernel: dc_m2snet.hip) ---------------------------------------------------------------
// fuse_layer of Contrastive_Stage/models/M2SNet.py:14-18: Conv1d(128 -> 64, k = 1), ReLU, Conv1d(64 -> 64, k = 1), ReLU,
// Conv1d(64 -> 1, k = 1), Sigmoid.  The weights are copied unchanged (nothing to fold) into v_mfma_f32_32x32x2_f32 A fragments,
// lane-major, one float per lane and k-step: lane l of fragment (mt, ks) = W[32 mt + (l & 31)][2 ks + (l >> 5)].  The last conv
// has one output row: its fragments carry w2 in row 0 (lanes 0 and 32) and zeros elsewhere.
constexpr int kHeadIn = 128, kHeadHid = 64;
constexpr int kHeadW0 = 0;                                         // [2 mt][64 ks][64 lanes]
constexpr int kHeadB0 = kHeadW0 + 2 * (kHeadIn / 2) * 64;           // [64]
constexpr int kHeadW1 = kHeadB0 + kHeadHid;                         // [2 mt][32 ks][64 lanes]
constexpr int kHeadB1 = kHeadW1 + 2 * (kHeadHid / 2) * 64;          // [64]
constexpr int kHeadW2 = kHeadB1 + kHeadHid;                         // [32 ks][64 lanes]
constexpr int kHeadB2 = kHeadW2 + (kHeadHid / 2) * 64;              // [1] (+ padding)
constexpr int kHeadFloats = kHeadB2 + 64;

inline void head_pack_frags(const float* W, int n_out, int k_in, float* dst) {
    for (int mt = 0; mt < cdiv(n_out, 32); ++mt)
        for (int ks = 0; ks < k_in / 2; ++ks)
            for (int l = 0; l < 64; ++l) {
                const int o = 32 * mt + (l & 31), k = 2 * ks + (l >> 5);
                dst[((size_t)mt * (k_in / 2) + ks) * 64 + l] = o < n_out ? W[(size_t)o * k_in + k] : 0.f;
            }
}

// params: `fuse_layer.{0,2,4}.{weight,bias}` (all present, sizes 64*128, 64, 64*64, 64, 64, 1)
inline std::vector<float> m2s_head_pack(const DcParams& params) {
    const auto P = [&](const char* n) -> const std::vector<float>& { return params.find(n)->second; };
    std::vector<float> img(kHeadFloats, 0.f);
    head_pack_frags(P("fuse_layer.0.weight").data(), kHeadHid, kHeadIn, img.data() + kHeadW0);
    head_pack_frags(P("fuse_layer.2.weight").data(), kHeadHid, kHeadHid, img.data() + kHeadW1);
    head_pack_frags(P("fuse_layer.4.weight").data(), 1, kHeadHid, img.data() + kHeadW2);
    memcpy(img.data() + kHeadB0, P("fuse_layer.0.bias").data(), kHeadHid * sizeof(float));
    memcpy(img.data() + kHeadB1, P("fuse_layer.2.bias").data(), kHeadHid * sizeof(float));
    img[kHeadB2] = P("fuse_layer.4.bias")[0];
    return img;
}

// ---- M2S-GAN generator image (kernels: dc_m2sgan.hip) -------------------------------------------------------------
// The decoder of Contrastive_Stage/models/Generator.py:52-77: six TemporalBlocks (models/TCN.py:19-52; Conv1d kernel 5, dilation
// 2^i, weight norm, eval-mode BatchNorm), TCN.linear, the fc head, and the noise branch's four ConvTranspose1d + noise_BN.
constexpr int kGanC = 64, kGanIn = 128, kGanTaps = 5, kGanBlocks = 6, kGanPose = 26, kGanLatent = 8;
struct GanConvT {
    int cin, cout, k, stride, pad;
};
constexpr GanConvT kGanNoise[4] = {{8, 16, 3, 1, 1}, {16, 16, 11, 5, 3}, {16, 32, 5, 3, 1}, {32, 64, 6, 2, 2}};
inline std::string gan_block(int i) { return "tcn.TCN.tcn.tcn.network." + std::to_string(i) + "."; }

// One weight-normed Conv1d with the eval-mode BatchNorm behind it as ONE weight and bias:
//   W[o][tap cin + ci] = s_o g_o v[o][ci][tap] / |v[o]|,   b[o] = (cb_o - mean_o) s_o + beta_o,   s_o = gamma_o / sqrt(var_o + eps)
// (|v[o]| over (ci, tap): torch's weight_norm with dim = 0).  v [cout][cin][k]; W [cout][k cin], tap-major - the k order of the
// convolution's GEMM.  Computed in fp64 and rounded once.
inline void gan_fold_conv(const float* g, const float* v, const float* cb, const float* gamma, const float* beta, const float* mean,
                          const float* var, int cout, int cin, int k, float* W, float* b) {
    for (int o = 0; o < cout; ++o) {
        double n2 = 0.0;
        for (int i = 0; i < cin * k; ++i) n2 += (double)v[(size_t)o * cin * k + i] * v[(size_t)o * cin * k + i];
        const double s = (double)gamma[o] / std::sqrt((double)var[o] + (double)kBnEps), a = s * g[o] / std::sqrt(n2);
        for (int ci = 0; ci < cin; ++ci)
            for (int tap = 0; tap < k; ++tap)
                W[(size_t)o * k * cin + (size_t)tap * cin + ci] = (float)(a * v[((size_t)o * cin + ci) * k + tap]);
        b[o] = (float)(((double)cb[o] - mean[o]) * s + beta[o]);
    }
}

// v_mfma_f32_32x32x2_f32 A fragments of a 64-row W [64][k_in] with both output tiles of a k-step side by side, so a lane reads
// them as one 8-byte load: dst[(ks 64 + l) 2 + mt] = W[32 mt + (l & 31)][2 ks + (l >> 5)]
inline void gan_pack_frags2(const float* W, int k_in, float* dst) {
    for (int ks = 0; ks < k_in / 2; ++ks)
        for (int l = 0; l < 64; ++l)
            for (int mt = 0; mt < 2; ++mt) dst[((size_t)ks * 64 + l) * 2 + mt] = W[(size_t)(32 * mt + (l & 31)) * k_in + 2 * ks + (l >> 5)];
}

struct GanImage {
    std::vector<float> img;      // every entry at a multiple of 64 floats
    struct Block {
        size_t w1, b1, w2, b2;   // gan_pack_frags2 images (K = 5 cin) and plain [64] biases
    } block[kGanBlocks];
    size_t wd, bd;               // block 0's 1x1 downsample: gan_pack_frags2 (K = 128), plain bias
    size_t hw[4], hb[4];         // TCN.linear, fc.0, fc.2, fc.4: head_pack_frags images ([mt][ks][lane]), plain biases
    size_t nw[4], nb[4];         // noise branch: the ConvTranspose1d weights [cin][cout][k] and biases as they are
    size_t nscale, nshift;       // noise_BN behind the last ReLU: y = scale x + shift
    size_t add(const std::vector<float>& v) {
        const size_t off = (img.size() + 63) & ~(size_t)63;
        img.resize(off + v.size());
        memcpy(img.data() + off, v.data(), v.size() * sizeof(float));
        return off;
    }
};

// names and sizes of the state_dict entries the generator's decoder computes with (the `music_encoder.*` ones: dc_music_required)
inline DcParamList gan_required() {
    DcParamList r;
    for (int i = 0; i < kGanBlocks; ++i) {
        const std::string p = gan_block(i);
        for (int c = 1; c <= 2; ++c) {
            const std::string cv = p + "conv" + std::to_string(c), bn = p + "bn" + std::to_string(c);
            const size_t cin = (i == 0 && c == 1) ? kGanIn : kGanC;
            r.push_back({cv + ".bias", kGanC});
            r.push_back({cv + ".weight_g", kGanC});
            r.push_back({cv + ".weight_v", kGanC * cin * kGanTaps});
            for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) r.push_back({bn + s, kGanC});
        }
        if (i == 0) {
            r.push_back({p + "downsample.weight", (size_t)kGanC * kGanIn});
            r.push_back({p + "downsample.bias", kGanC});
        }
    }
    r.push_back({"tcn.TCN.tcn.linear.weight", (size_t)kGanC * kGanC});
    r.push_back({"tcn.TCN.tcn.linear.bias", kGanC});
    for (int i = 0; i < 3; ++i) {
        const size_t n = i == 2 ? kGanPose : kGanC;
        r.push_back({"tcn.fc." + std::to_string(2 * i) + ".weight", n * kGanC});
        r.push_back({"tcn.fc." + std::to_string(2 * i) + ".bias", n});
    }
    for (int i = 0; i < 4; ++i) {
        const GanConvT& c = kGanNoise[i];
        r.push_back({"noise_convTranspose." + std::to_string(2 * i) + ".weight", (size_t)c.cin * c.cout * c.k});
        r.push_back({"noise_convTranspose." + std::to_string(2 * i) + ".bias", (size_t)c.cout});
    }
    for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) r.push_back({std::string("noise_BN") + s, kGanC});
    return r;
}

// the entries of gan_required a features-only generator (decoder = none) computes with: everything but `tcn.*`
inline DcParamList gan_required_features() {
    DcParamList r;
    for (const auto& e : gan_required())
        if (e.first.rfind("tcn.", 0) != 0) r.push_back(e);
    return r;
}

// params: every entry of gan_required (with_tcn) or of gan_required_features (the `tcn.*` offsets are then left unset), with its size
inline GanImage gan_pack(const DcParams& params, bool with_tcn = true) {
    const auto P = [&](const std::string& n) -> const float* { return params.find(n)->second.data(); };
    GanImage I;
    const int n_blocks = with_tcn ? kGanBlocks : 0, n_head = with_tcn ? 4 : 0;
    const auto conv = [&](const std::string& cv, const std::string& bn, int cin, size_t& w, size_t& b) {
        std::vector<float> W((size_t)kGanC * kGanTaps * cin), bias(kGanC), frags(W.size());
        gan_fold_conv(P(cv + ".weight_g"), P(cv + ".weight_v"), P(cv + ".bias"), P(bn + ".weight"), P(bn + ".bias"), P(bn + ".running_mean"),
                      P(bn + ".running_var"), kGanC, cin, kGanTaps, W.data(), bias.data());
        gan_pack_frags2(W.data(), kGanTaps * cin, frags.data());
        w = I.add(frags);
        b = I.add(bias);
    };
    for (int i = 0; i < n_blocks; ++i) {
        const std::string p = gan_block(i);
        conv(p + "conv1", p + "bn1", i == 0 ? kGanIn : kGanC, I.block[i].w1, I.block[i].b1);
        conv(p + "conv2", p + "bn2", kGanC, I.block[i].w2, I.block[i].b2);
    }
    if (with_tcn) {
        std::vector<float> fd((size_t)kGanC * kGanIn);
        gan_pack_frags2(P(gan_block(0) + "downsample.weight"), kGanIn, fd.data());
        I.wd = I.add(fd);
        I.bd = I.add(params.find(gan_block(0) + "downsample.bias")->second);
    }
    const std::string head[4] = {"tcn.TCN.tcn.linear", "tcn.fc.0", "tcn.fc.2", "tcn.fc.4"};
    for (int i = 0; i < n_head; ++i) {
        const int n = i == 3 ? kGanPose : kGanC;
        std::vector<float> f((size_t)cdiv(n, 32) * (kGanC / 2) * 64), b(kGanC, 0.f);
        head_pack_frags(P(head[i] + ".weight"), n, kGanC, f.data());
        memcpy(b.data(), P(head[i] + ".bias"), n * sizeof(float));
        I.hw[i] = I.add(f);
        I.hb[i] = I.add(b);
    }
    for (int i = 0; i < 4; ++i) {
        const std::string p = "noise_convTranspose." + std::to_string(2 * i);
        I.nw[i] = I.add(params.find(p + ".weight")->second);
        I.nb[i] = I.add(params.find(p + ".bias")->second);
    }
    std::vector<float> sc(kGanC), sh(kGanC);
    for (int c = 0; c < kGanC; ++c) {
        const double s = (double)P("noise_BN.weight")[c] / std::sqrt((double)P("noise_BN.running_var")[c] + (double)kBnEps);
        sc[c] = (float)s;
        sh[c] = (float)((double)P("noise_BN.bias")[c] - (double)P("noise_BN.running_mean")[c] * s);
    }
    I.nscale = I.add(sc);
    I.nshift = I.add(sh);
    return I;
}

// ---- BiLSTM pose decoder image (kernels: dc_bilstm.hip) -----------------------------------------------------------
// PoseDecoderBiLSTM of Contrastive_Stage/models/Generator.py:7-31: nn.LSTM(In, 128, num_layers = 2, bidirectional) and the head
// `out` = Linear(256, 64), ReLU, Linear(64, 64), ReLU, Linear(64, 26), Sigmoid.  Gate rows in torch's order i, f, g, o.
constexpr int kLstmH = 128, kLstmGates = 4 * kLstmH, kLstmRows = 2 * kLstmGates, kLstmMaxIn = 128, kLstmPose = 26, kLstmHead = 64;
inline std::string lstm_name(const char* leaf, int layer, int dir) {
    return std::string("LSTM.") + leaf + "_l" + std::to_string(layer) + (dir ? "_reverse" : "");
}

// names and sizes of the decoder's state_dict entries for an input of `in` features, in the module's order
inline DcParamList lstm_required(int in) {
    DcParamList r;
    for (int l = 0; l < 2; ++l)
        for (int d = 0; d < 2; ++d) {
            r.push_back({lstm_name("weight_ih", l, d), (size_t)kLstmGates * (l ? 2 * kLstmH : in)});
            r.push_back({lstm_name("weight_hh", l, d), (size_t)kLstmGates * kLstmH});
            r.push_back({lstm_name("bias_ih", l, d), kLstmGates});
            r.push_back({lstm_name("bias_hh", l, d), kLstmGates});
        }
    const int n[3] = {kLstmHead, kLstmHead, kLstmPose}, k[3] = {2 * kLstmH, kLstmHead, kLstmHead};
    for (int i = 0; i < 3; ++i) {
        r.push_back({"out." + std::to_string(2 * i) + ".weight", (size_t)n[i] * k[i]});
        r.push_back({"out." + std::to_string(2 * i) + ".bias", (size_t)n[i]});
    }
    return r;
}

// A layer's input projection for both directions as ONE 1024-row matrix (row 512 d + r = W_ih[d][r]) in sixteen 64-row groups,
// each a gan_pack_frags2 image over k_pad columns (k_in, rounded up to even, the pad a zero weight): dst [16][k_pad / 2][64][2]
inline void lstm_pack_proj(const float* w_fwd, const float* w_bwd, int k_in, int k_pad, float* dst) {
    std::vector<float> W((size_t)64 * k_pad);
    for (int rg = 0; rg < kLstmRows / 64; ++rg) {
        const float* src = (rg < 8 ? w_fwd : w_bwd) + (size_t)(rg & 7) * 64 * k_in;
        for (int r = 0; r < 64; ++r)
            for (int k = 0; k < k_pad; ++k) W[(size_t)r * k_pad + k] = k < k_in ? src[(size_t)r * k_in + k] : 0.f;
        gan_pack_frags2(W.data(), k_pad, dst + (size_t)rg * 64 * k_pad);
    }
}
// b_ih + b_hh of both directions [1024], summed in fp64 and rounded once
inline void lstm_fold_bias(const float* bih_f, const float* bhh_f, const float* bih_b, const float* bhh_b, float* dst) {
    for (int r = 0; r < kLstmGates; ++r) {
        dst[r] = (float)((double)bih_f[r] + (double)bhh_f[r]);
        dst[kLstmGates + r] = (float)((double)bih_b[r] + (double)bhh_b[r]);
    }
}

struct LstmImage {
    std::vector<float> img;      // every entry at a multiple of 64 floats
    int in = 0, k_pad[2] = {0, 2 * kLstmH};
    size_t wih[2], bias[2];      // per layer: lstm_pack_proj image, lstm_fold_bias [1024]
    size_t whh[2];               // per layer: W_hh of both directions as they are, [2][512][128]
    size_t hw[3], hb[3];         // out.0, out.2, out.4: head_pack_frags images ([mt][ks][lane]), plain biases (padded to 64)
    size_t add(const std::vector<float>& v) {
        const size_t off = (img.size() + 63) & ~(size_t)63;
        img.resize(off + v.size());
        memcpy(img.data() + off, v.data(), v.size() * sizeof(float));
        return off;
    }
};

// params: every entry of lstm_required(in), with its size
inline LstmImage lstm_pack(const DcParams& params, int in) {
    const auto P = [&](const std::string& n) -> const float* { return params.find(n)->second.data(); };
    LstmImage I;
    I.in = in;
    I.k_pad[0] = (in + 1) & ~1;
    for (int l = 0; l < 2; ++l) {
        const int k_in = l ? 2 * kLstmH : in;
        std::vector<float> f((size_t)kLstmRows * I.k_pad[l]), b(kLstmRows), hh((size_t)2 * kLstmGates * kLstmH);
        lstm_pack_proj(P(lstm_name("weight_ih", l, 0)), P(lstm_name("weight_ih", l, 1)), k_in, I.k_pad[l], f.data());
        lstm_fold_bias(P(lstm_name("bias_ih", l, 0)), P(lstm_name("bias_hh", l, 0)), P(lstm_name("bias_ih", l, 1)), P(lstm_name("bias_hh", l, 1)),
                       b.data());
        for (int d = 0; d < 2; ++d) memcpy(hh.data() + (size_t)d * kLstmGates * kLstmH, P(lstm_name("weight_hh", l, d)), sizeof(float) * kLstmGates * kLstmH);
        I.wih[l] = I.add(f);
        I.bias[l] = I.add(b);
        I.whh[l] = I.add(hh);
    }
    const int n[3] = {kLstmHead, kLstmHead, kLstmPose}, k[3] = {2 * kLstmH, kLstmHead, kLstmHead};
    for (int i = 0; i < 3; ++i) {
        const std::string p = "out." + std::to_string(2 * i);
        std::vector<float> f((size_t)cdiv(n[i], 32) * (k[i] / 2) * 64), b(kLstmHead, 0.f);
        head_pack_frags(P(p + ".weight"), n[i], k[i], f.data());
        memcpy(b.data(), P(p + ".bias"), n[i] * sizeof(float));
        I.hw[i] = I.add(f);
        I.hb[i] = I.add(b);
    }
    return I;
}

// ---- ST-GCN motion encoder image (kernels: dc_stgcn.hip) ----------------------------------------------------------
// MotionEncoder_STGCN in eval mode; the network and the folding formulas are at the head of dc_stgcn.hip.  Everything is computed
// in fp64 and rounded once, except Ahat = A * edge_importance, the reference's own fp32 product.
constexpr int kStgcnV = 13, kStgcnC = 32, kStgcnL = 10, kStgcnOut = 64, kStgcnK = kStgcnC * kStgcnV;   // joints, channels, blocks, latent, fc K
// device parameter image (floats).  Per block: W1 fragments [16 kk][64 lanes] (lane l = W1'[l & 31][2 kk + (l >> 5)]; block 0
// uses kk = 0 only), W2 fragments [3 tap][16 kk][64], b1' [13 w][32 c], b2' [32], Ahat [13 w][13 v] (+ pad).
constexpr int kStgcnW1 = 0, kStgcnW2 = kStgcnW1 + 16 * 64, kStgcnB1 = kStgcnW2 + 3 * 16 * 64, kStgcnB2 = kStgcnB1 + kStgcnV * kStgcnC,
              kStgcnAhat = kStgcnB2 + kStgcnC, kStgcnBlockFloats = kStgcnAhat + 176;
constexpr int kStgcnDbn = kStgcnL * kStgcnBlockFloats;           // data_bn scale [26] at +0, shift [26] at +32
constexpr int kStgcnFcW = kStgcnDbn + 64;                        // fc fragments [2 mt][208 ks][64]: lane l = W'[32 mt + (l & 31)][2 ks + (l >> 5)]
constexpr int kStgcnFcB = kStgcnFcW + 2 * (kStgcnK / 2) * 64;    // fc bias' [64]
constexpr int kStgcnFloats = kStgcnFcB + kStgcnOut;
// This fold has always added BatchNorm's epsilon as the double 1e-5; kBnEps widened is 2.5e-13 smaller, enough to move a folded
// weight by an ulp where running_var is small.  Kept, so that the image stays what it was bit for bit.
constexpr double kStgcnBnEps = 1e-5;
inline std::string stgcn_block(int l) { return "st_gcn.st_gcn_networks." + std::to_string(l) + "."; }

// names and sizes of the state_dict entries the encoder computes with ...
inline DcParamList stgcn_required() {
    DcParamList r;
    const auto bn = [&](const std::string& p, size_t n) {
        for (const char* s : {"weight", "bias", "running_mean", "running_var"}) r.push_back({p + s, n});
    };
    r.push_back({"st_gcn.A", kStgcnV * kStgcnV});
    bn("st_gcn.data_bn.", 2 * kStgcnV);
    for (int l = 0; l < kStgcnL; ++l) {
        const std::string p = stgcn_block(l);
        r.push_back({p + "gcn.conv.weight", (size_t)kStgcnC * (l == 0 ? 2 : kStgcnC)});
        r.push_back({p + "gcn.conv.bias", kStgcnC});
        bn(p + "tcn.0.", kStgcnC);
        r.push_back({p + "tcn.2.weight", kStgcnC * kStgcnC * 3});
        r.push_back({p + "tcn.2.bias", kStgcnC});
        bn(p + "tcn.3.", kStgcnC);
        r.push_back({"st_gcn.edge_importance." + std::to_string(l), kStgcnV * kStgcnV});
    }
    r.push_back({"fc.0.weight", (size_t)kStgcnOut * kStgcnK});
    r.push_back({"fc.0.bias", kStgcnOut});
    bn("fc.1.", kStgcnOut);
    return r;
}
// ... and of those it never applies: ST_GCN's classification head (the BatchNorm counters go by the rule of dc_handle.h)
inline DcParamList stgcn_ignored() { return {{"st_gcn.fcn.weight", 32 * 256}, {"st_gcn.fcn.bias", 32}}; }

// params: every entry of stgcn_required, with its size
inline std::vector<float> stgcn_pack(const DcParams& params) {
    const auto P = [&](const std::string& n) -> const std::vector<float>& { return params.find(n)->second; };
    // eval-mode BatchNorm as y = s x + h
    const auto bn_affine = [&](const std::string& p, size_t n, std::vector<double>& s, std::vector<double>& h) {
        const auto &g = P(p + "weight"), &be = P(p + "bias"), &rm = P(p + "running_mean"), &rv = P(p + "running_var");
        s.resize(n);
        h.resize(n);
        for (size_t i = 0; i < n; ++i) {
            s[i] = (double)g[i] / std::sqrt((double)rv[i] + kStgcnBnEps);
            h[i] = (double)be[i] - (double)rm[i] * s[i];
        }
    };
    std::vector<float> img(kStgcnFloats, 0.f);
    const auto& A = P("st_gcn.A");
    std::vector<double> s0, h0, s3, h3;
    for (int l = 0; l < kStgcnL; ++l) {
        const std::string p = stgcn_block(l);
        const int cin = l == 0 ? 2 : kStgcnC;
        float* blk = img.data() + (size_t)l * kStgcnBlockFloats;
        const auto& E = P("st_gcn.edge_importance." + std::to_string(l));
        const auto &W1 = P(p + "gcn.conv.weight"), &bb1 = P(p + "gcn.conv.bias");
        const auto &W2 = P(p + "tcn.2.weight"), &bb2 = P(p + "tcn.2.bias");
        bn_affine(p + "tcn.0.", kStgcnC, s0, h0);
        bn_affine(p + "tcn.3.", kStgcnC, s3, h3);
        double colsum[kStgcnV];
        for (int w = 0; w < kStgcnV; ++w) {
            colsum[w] = 0.0;
            for (int v = 0; v < kStgcnV; ++v) {
                const float a = A[v * kStgcnV + w] * E[v * kStgcnV + w];      // the reference's A * importance, in fp32
                blk[kStgcnAhat + w * kStgcnV + v] = a;
                colsum[w] += a;
            }
        }
        for (int lane = 0; lane < 64; ++lane) {
            const int c = lane & 31, hh = lane >> 5;
            for (int kk = 0; kk < (l == 0 ? 1 : 16); ++kk) {
                const int ci = 2 * kk + hh;
                blk[kStgcnW1 + kk * 64 + lane] = (float)(s0[c] * W1[c * cin + ci]);
            }
            for (int k = 0; k < 3; ++k)
                for (int kk = 0; kk < 16; ++kk) {
                    const int ci = 2 * kk + hh;     // tcn.2.weight [c][ci][k][0]
                    blk[kStgcnW2 + (k * 16 + kk) * 64 + lane] = (float)(s3[c] * W2[(c * kStgcnC + ci) * 3 + k]);
                }
        }
        for (int w = 0; w < kStgcnV; ++w)
            for (int c = 0; c < kStgcnC; ++c) blk[kStgcnB1 + w * kStgcnC + c] = (float)(s0[c] * bb1[c] * colsum[w] + h0[c]);
        for (int c = 0; c < kStgcnC; ++c) blk[kStgcnB2 + c] = (float)(s3[c] * bb2[c] + h3[c]);
    }
    std::vector<double> sd, hd, sf, hf;
    bn_affine("st_gcn.data_bn.", 2 * kStgcnV, sd, hd);
    for (int i = 0; i < 2 * kStgcnV; ++i) {
        img[kStgcnDbn + i] = (float)sd[i];
        img[kStgcnDbn + 32 + i] = (float)hd[i];
    }
    bn_affine("fc.1.", kStgcnOut, sf, hf);
    const auto &Wf = P("fc.0.weight"), &bf = P("fc.0.bias");
    for (int mt = 0; mt < 2; ++mt)
        for (int ks = 0; ks < kStgcnK / 2; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int o = 32 * mt + (lane & 31), k = 2 * ks + (lane >> 5);
                img[kStgcnFcW + ((size_t)mt * (kStgcnK / 2) + ks) * 64 + lane] = (float)(sf[o] * Wf[(size_t)o * kStgcnK + k]);
            }
    for (int o = 0; o < kStgcnOut; ++o) img[kStgcnFcB + o] = (float)(sf[o] * bf[o] + hf[o]);
    return img;
}

// ---- M2S-GAN critic image (kernels: dc_rhythm.hip) ----------------------------------------------------------------
// Discriminator_1DCNN of Contrastive_Stage/models/Discriminator.py:5-27: three Conv1d(kernel 5, zero padding 2) + ReLU +
// MaxPool1d(5, stride 3 / 2 / 2) on 26 -> 64 -> 64 -> 64 channels, then fc 64 -> 32 -> 32 -> 1 per pooled frame.  Nothing to fold:
// the weights are permuted into the k order of the convolution's GEMM (column tap cin + ci) and packed as A fragments.
constexpr int kDiscC = 64, kDiscIn = 26, kDiscTaps = 5, kDiscHid = 32, kDiscStages = 3;
constexpr int kDiscStride[kDiscStages] = {3, 2, 2};      // MaxPool1d(5, stride)
constexpr int kDiscMinT = 41;                            // the shortest clip with one pooled frame behind the third stage
inline int disc_pooled(int L, int stride) { return L < kDiscTaps ? 0 : (L - kDiscTaps) / stride + 1; }

struct DiscImage {
    std::vector<float> img;      // every entry at a multiple of 64 floats
    size_t w[kDiscStages], b[kDiscStages];      // gan_pack_frags2 images (K = 5 cin, tap-major) and plain [64] biases
    size_t fw[3], fb[3];                        // fc.0, fc.2, fc.4: head_pack_frags images ([ks][lane], one output tile), biases padded to 64
    size_t add(const std::vector<float>& v) {
        const size_t off = (img.size() + 63) & ~(size_t)63;
        img.resize(off + v.size());
        memcpy(img.data() + off, v.data(), v.size() * sizeof(float));
        return off;
    }
};

// names and sizes of the critic's 12 state_dict entries, in the reference module's order
inline DcParamList disc_required() {
    DcParamList r;
    for (int i = 0; i < kDiscStages; ++i) {
        const std::string p = "motion_encoder." + std::to_string(3 * i);
        r.push_back({p + ".weight", (size_t)kDiscC * (i == 0 ? kDiscIn : kDiscC) * kDiscTaps});
        r.push_back({p + ".bias", kDiscC});
    }
    const size_t fin[3] = {kDiscC, kDiscHid, kDiscHid}, fout[3] = {kDiscHid, kDiscHid, 1};
    for (int i = 0; i < 3; ++i) {
        r.push_back({"fc." + std::to_string(2 * i) + ".weight", fout[i] * fin[i]});
        r.push_back({"fc." + std::to_string(2 * i) + ".bias", fout[i]});
    }
    return r;
}

// params: every entry of disc_required, with its size
inline DiscImage disc_pack(const DcParams& params) {
    const auto P = [&](const std::string& n) -> const std::vector<float>& { return params.find(n)->second; };
    DiscImage I;
    for (int i = 0; i < kDiscStages; ++i) {
        const std::string p = "motion_encoder." + std::to_string(3 * i);
        const int cin = i == 0 ? kDiscIn : kDiscC, K = kDiscTaps * cin;
        const std::vector<float>& w = P(p + ".weight");      // [64][cin][5]
        std::vector<float> W((size_t)kDiscC * K), frags(W.size());
        for (int o = 0; o < kDiscC; ++o)
            for (int ci = 0; ci < cin; ++ci)
                for (int tap = 0; tap < kDiscTaps; ++tap) W[(size_t)o * K + tap * cin + ci] = w[((size_t)o * cin + ci) * kDiscTaps + tap];
        gan_pack_frags2(W.data(), K, frags.data());
        I.w[i] = I.add(frags);
        I.b[i] = I.add(P(p + ".bias"));
    }
    const int fin[3] = {kDiscC, kDiscHid, kDiscHid}, fout[3] = {kDiscHid, kDiscHid, 1};
    for (int i = 0; i < 3; ++i) {
        const std::string p = "fc." + std::to_string(2 * i);
        std::vector<float> f((size_t)(fin[i] / 2) * 64), b(64, 0.f);
        head_pack_frags(P(p + ".weight").data(), fout[i], fin[i], f.data());
        memcpy(b.data(), P(p + ".bias").data(), fout[i] * sizeof(float));
        I.fw[i] = I.add(f);
        I.fb[i] = I.add(b);
    }
    return I;
}

// ---- Welch window-and-twiddle table (kernel: dc_rhythm.hip) -------------------------------------------------------
// scipy.signal.welch(x, fs = 30) with its defaults as ONE matrix on the detrended segment: nperseg = 256, periodic Hann window w,
// `density` scaling 1 / (fs sum w^2), one-sided doubling of every bin but 0.  Row k (bins 0 .. 31) holds g_k w[n] cos(2 pi k n / 256),
// row 32 + k holds g_k w[n] sin(2 pi k n / 256), g_k = sqrt((k ? 2 : 1) / (30 sum w^2)): |row_k . x|^2 + |row_{32+k} . x|^2 is the
// segment's PSD at bin k.  Computed in fp64, rounded once.  [64][256] row-major.
constexpr int kWelchSeg = 256, kWelchHop = 128, kWelchBins = 32;
constexpr double kWelchFs = 30.0;
inline std::vector<float> welch_table() {
    const double pi = 3.14159265358979323846;
    std::vector<double> w(kWelchSeg);
    double s2 = 0.0;
    for (int n = 0; n < kWelchSeg; ++n) {
        w[n] = 0.5 - 0.5 * std::cos(2.0 * pi * n / kWelchSeg);
        s2 += w[n] * w[n];
    }
    std::vector<float> tab((size_t)2 * kWelchBins * kWelchSeg);
    for (int k = 0; k < kWelchBins; ++k) {
        const double g = std::sqrt((k ? 2.0 : 1.0) / (kWelchFs * s2));
        for (int n = 0; n < kWelchSeg; ++n) {
            const double a = 2.0 * pi * ((k * n) % kWelchSeg) / kWelchSeg;      // (the argument reduced exactly)
            tab[(size_t)k * kWelchSeg + n] = (float)(g * w[n] * std::cos(a));
            tab[(size_t)(kWelchBins + k) * kWelchSeg + n] = (float)(g * w[n] * std::sin(a));
        }
    }
    return tab;
}

// ---- mel front end: window, twiddles, sparse Slaney filterbank (kernel: dc_mel.hip) ---------------------------------
// librosa.feature.melspectrogram(y, sr, n_mels = 128, hop_length = 256) with its defaults: n_fft = 2048, the periodic Hann window,
// librosa.filters.mel(sr, 2048, 128) - Slaney's scale (linear below 1 kHz at 200 / 3 Hz per mel, logarithmic above with step
// ln(6.4) / 27), n_mels + 2 edge frequencies linspace'd in mel from 0 to sr / 2, triangles max(0, min(lower, upper)) scaled by
// 2 / (f[i + 2] - f[i]).  Everything in fp64, rounded once.  A filter is stored as its run of non-zero bins: at 22050 Hz 4 .. 53 of
// the 1025, 2018 weights in all where the dense matrix has 131 200.
constexpr int kMelFft = 2048, kMelHop = 256, kMelBands = 128, kMelBins = kMelFft / 2 + 1;
inline double mel_to_hz(double m) { return m >= 15.0 ? 1000.0 * std::exp((std::log(6.4) / 27.0) * (m - 15.0)) : (200.0 / 3.0) * m; }
inline double hz_to_mel(double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) / (std::log(6.4) / 27.0) : f / (200.0 / 3.0); }
struct MelTables {
    std::vector<float> window;                   // [2048]  0.5 - 0.5 cos(2 pi n / 2048)
    std::vector<float> twiddle;                  // [2048][2]  cos, -sin of 2 pi j / 2048
    std::vector<int32_t> first, count, offset;   // [128]  filter m covers bins first .. first + count - 1, its weights at `offset`
    std::vector<float> weights;                  // the filters' non-zero runs, one after the other
};
inline MelTables mel_tables(int sr) {
    const double pi = 3.14159265358979323846;
    MelTables t;
    t.window.resize(kMelFft);
    t.twiddle.resize((size_t)2 * kMelFft);
    for (int n = 0; n < kMelFft; ++n) {
        const double a = 2.0 * pi * n / kMelFft;
        t.window[n] = (float)(0.5 - 0.5 * std::cos(a));
        t.twiddle[2 * n] = (float)std::cos(a);
        t.twiddle[2 * n + 1] = (float)-std::sin(a);
    }
    // numpy.linspace(0, hz_to_mel(sr / 2), 130): i * step + start, the last element the stop itself
    const double top = hz_to_mel(0.5 * sr), step = top / (kMelBands + 1);
    std::vector<double> f(kMelBands + 2);
    for (int i = 0; i < kMelBands + 2; ++i) f[i] = mel_to_hz(i == kMelBands + 1 ? top : i * step);
    t.first.resize(kMelBands);
    t.count.resize(kMelBands);
    t.offset.resize(kMelBands);
    std::vector<double> row(kMelBins);
    for (int m = 0; m < kMelBands; ++m) {
        const double d0 = f[m + 1] - f[m], d1 = f[m + 2] - f[m + 1], norm = 2.0 / (f[m + 2] - f[m]);
        int lo = kMelBins, hi = -1;
        for (int k = 0; k < kMelBins; ++k) {
            const double fk = k * ((double)sr / kMelFft);
            const double lower = -(f[m] - fk) / d0, upper = (f[m + 2] - fk) / d1;
            const double w = std::fmax(0.0, std::fmin(lower, upper)) * norm;
            row[k] = w;
            if ((float)w != 0.f) {
                if (k < lo) lo = k;
                hi = k;
            }
        }
        t.first[m] = hi < 0 ? 0 : lo;
        t.count[m] = hi < 0 ? 0 : hi - lo + 1;
        t.offset[m] = (int32_t)t.weights.size();
        for (int k = t.first[m]; k < t.first[m] + t.count[m]; ++k) t.weights.push_back((float)row[k]);
    }
    return t;
}

// The reference's int(len(y) / sr * 90) (Diffusion_Stage/tools/visualization.py:160): a double division, a double product, truncation.
// (n * 90 / sr in integers disagrees for some n; the one copy the library and its bindings use.)
inline int32_t mel_out_frames(int64_t n, int32_t sr) { return (int32_t)((double)n / (double)sr * 90.0); }
