// dc_launch.h - host-callable launchers implemented in dc_kernels.hip.  fmt: 0 = bf16 operands, 1 = f16.
#pragma once
#include <hip/hip_runtime.h>
#include "dc_common.h"

// Kernels that use more than 64 KiB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize, and the attribute is
// per DEVICE: `done` is a per-kernel bit mask of the devices that already have it (a process may hold samplers on several GPUs).
inline hipError_t dc_lds_optin(const void* fn, int bytes, unsigned long long& done) {
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    if (dev < 64 && ((done >> dev) & 1ull)) return hipSuccess;
    if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes)) return e;
    if (dev < 64) done |= 1ull << dev;
    return hipSuccess;
}
// CUs of the current device (asked once per device)
inline hipError_t dc_cu_count(int* ncu) {
    static int n[64] = {0};
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return e;
    int& slot = n[dev & 63];
    if (!slot)
        if (hipError_t e = hipDeviceGetAttribute(&slot, hipDeviceAttributeMultiprocessorCount, dev)) return e;
    *ncu = slot;
    return hipSuccess;
}

hipError_t dc_launch_begin_step(hipStream_t st, int* iter, const int* t_of_iter, const float* coef_of_iter,
                                const int* snap_of_iter, int* t_clip, float* coef_cur, int* snap_cur, int B);
hipError_t dc_launch_temb_table(hipStream_t st, const float* freqs, const float* w0t, const float* b0,
                                const float* w2t, const float* b2, float* temb, int nt);
// `self.linear` of one conditioning tensor [M][64] into a fragment-major operand image: mode 0 = fp32 image of emb's
// step-invariant term (out_f32), mode 1 = text_norm'ed bf16 hi / lo images (out_hi, out_lo) for the cross-attention pre-pass
hipError_t dc_launch_cond_embed(hipStream_t st, int mode, const float* xf, const float* wt, const float* b, float* out_f32,
                                void* out_hi, void* out_lo, int M, int G, int T /* clip stride of the images */,
                                int Tx /* frames per clip of xf (<= T; the rest of a clip's stride is padding) */);
hipError_t dc_launch_ca_partials(hipStream_t st, const DcModel* dm, const void* nh_hi, const void* nh_lo,
                                 float* recs, int M, int T, int G, int L, int Tx /* frames per clip (<= the clip stride T) */);
// MODE 0 of dc_launch_cond_embed (the fp32 image of linear(xf_proj)) on split-bf16 MFMAs
hipError_t dc_launch_cond_pp64(hipStream_t st, const float* xf /*[B][Tx][64]*/, const void* wpack, const float* b, float* out_f32, int M, int G, int T, int Tx);
// the same records from the 64 music features (K = rstd (A x + d) + b'): k_cond_rstd -> rstd [G * 32], then k_cond_ca_partials64
hipError_t dc_launch_ca_partials64(hipStream_t st, const DcModel* dm, const float* xf /*[B][Tx][64]*/, const float* gram, float* rstd, float* recs,
                                   int M, int T, int G, int L, int Tx);
hipError_t dc_launch_attn_combine(hipStream_t st, int fmt, const float* recs, void* afrag, int T, int NU, int B, int nset,
                                  int gran);
hipError_t dc_launch_silu_emb(hipStream_t st, int fmt, bool split, const float* pp, const float* temb, const int* t_clip,
                              void* s_hi, void* s_lo, int G, int T, int B,
                              const int* iter_base = nullptr /* captured loop: t_clip = &t_of_iter[step], indexed by *iter_base */);
// pp != nullptr (non-split formats): the FiLM GEMM builds its operand SiLU(temb[t_clip] + pp) itself and s_hi is not read
struct DcFilmArgs {
    const void* W;
    const float* bias_ft;
    const void *s_hi, *s_lo;
    void* E;
    int G, NT, round0, nround;
    const float *pp, *temb;
    const int* t_clip;
    int T, B;
    unsigned long long* clk;     // diagnostic clock stamps or nullptr
    const float* rate_in;        // per-workgroup speeds of the previous / this launch (num_cu floats) or nullptr
    float* rate_out;
    const int* iter_base;        // captured loop: t_clip = &t_of_iter[step], indexed by *iter_base; else nullptr
    const void* W16;             // operands of the 16x16x32-MFMA form (used with pp, non-split)
    const float* bias16;
    const DcEmbedArgs* embed;    // S-stationary form only: fuse k_embed_front into this launch; an error if the launch cannot carry it
    int* status;                 // device status word: DC_STATUS_F16_SAT is OR-ed in when a tile leaves the fp16 range, or nullptr
};
hipError_t dc_launch_film_gemm(hipStream_t st, int fmt, bool split, const DcFilmArgs& a);
// The form of one step's k_embed_front / k_layer launches, as step_form decided it (dc_form.h).  The launchers pick the kernel
// instantiation from a table of the forms that exist; any other combination is hipErrorInvalidValue.
struct DcLayerForm {
    int fmt;
    bool split;
    bool wgr;            // workgroup-level partial records, combined by the consuming layer kernel itself (T >= 256 only; no
                         // dc_launch_attn_combine between the layers then).  Split formats: on clip-aligned units only (upc > 0)
    bool narrow;         // wgr, non-split, no stop stage, no stamps: 4-wave workgroups = 128-token units (small batches)
    bool g1;             // the FiLM scale tiles hold G' (film_affine in dc_dev.h; plain-operand production forms of k_layer only)
    int upc;             // wgr: workgroups per clip (clip-aligned units, WgMap in dc_dev.h), grid = B * upc; else 0
    size_t rec_stride;   // floats between the two alternating unit-record buffers, in units of the form (0 = single buffer, non-wgr)
    bool idle_path;      // k_layer, wide plain production form (wgr, non-split, 8 waves, no stop stage, no stamps): the padding waves of a
                         // clip's last workgroup pass the launch on the barrier-only path (layer_idle_wave); every other form ignores it
};
hipError_t dc_launch_embed_front(hipStream_t st, const DcLayerForm& f, const DcModel* dm, const float* x, float* hbuf, float* recs,
                                 const int* length, int M, int T, int G, int B,
                                 unsigned long long* clk /* diagnostic stamps (8 slots) or nullptr */,
                                 int Tx /* frames per clip of x (<= the clip stride T) */);
// test hook: front half of layer l0 from the residual stream as it stands in hbuf (per-group records)
hipError_t dc_launch_front_from_h(hipStream_t st, int fmt, bool split, const DcModel* dm, float* hbuf, float* recs, const int* length,
                                  int M, int T, int G, int B, int l0);
// What the layer launches of one step share (dc_launch_layer, dc_launch_layer16, dc_launch_layer_full)
struct DcLayerArgs {
    const DcModel* dm;
    float* hbuf;
    const void* E;
    int NT;
    float* recs;
    const int* length;
    const float* xin;
    float* xout;
    int out_mode;
    const float* coef_cur;       // captured loop: coef_cur / snap_cur = this step's slots of the per-iteration tables, indexed by
    const int* snap_cur;         // *iter_base; else iter_base = nullptr (scalars prepared by k_begin_step)
    float* snaps;
    const int* iter_base;
    int M, T, G, B;
    int Tx;                      // frames per clip of xin / xout / snaps
    int e_groups;                // groups of FiLM tiles behind E (film_share, dc_form.h): token group g reads the tiles of group
    int e_period, e_wrap;        // g < e_wrap ? g % e_period : e_groups - 1 (film_tile_group).  Nothing shared: all three G.  Guided, one
                                 // shared null column: e_period = e_wrap = the conditional half's groups, e_groups one more.  Takes:
                                 // e_period = one take's groups, e_wrap = the groups of all conditional clips
    unsigned e_magic;            // film_magic(e_period, e_wrap): the reciprocal the kernels take g / e_period from (0 where e_period == e_wrap)
    DcUpdate upd;                // options of the fused DDIM update + the status word (dc_common.h)
    // what film_tile_group relies on (checked by every layer launcher): the mapping stays inside the e_groups groups the GEMM wrote
    bool tiles_ok() const { return e_period >= 1 && e_wrap >= e_period && e_groups >= 1 && e_period <= e_groups && (e_magic != 0) == (e_period < e_wrap); }
};
hipError_t dc_launch_layer(hipStream_t st, const DcLayerForm& f, const DcLayerArgs& a, int l, const void* a_sa, const void* a_ca,
                           int dbg /* stop stage of this layer (test hook), 0 = the whole layer */,
                           unsigned long long* stamps /* diagnostic stage stamps or nullptr */);
// The same layer for SMALL batches on 16-token waves (dc_layer16.hip): non-split formats, clip-aligned 64-token units (grid = B * upc,
// upc = ceil(T / 64), T = clip stride, a multiple of 32), one unit record per workgroup.  a_ca16 = the cross-attention fragments in
// that kernel's form (dc_launch_cond_af16, once per conditioning).  nu_in / stride_in: unit records per clip and floats per unit of
// the records this layer combines (layer 0: k_embed_front's narrow 128-token units, 2 * DC_REC_FLOATS apart; later layers: upc
// units DC_REC_FLOATS apart).  At most dc_layer16_max_units() records per clip.
hipError_t dc_launch_layer16(hipStream_t st, int fmt, const DcLayerArgs& a, int l, const void* a_ca16, int upc, size_t rec_stride, int nu_in,
                             size_t stride_in,
                             unsigned long long* gran /* [B][1024] granules: the clip's workgroups share the combine inside the launch (nullptr: each alone) */,
                             unsigned tag_base /* the launch's tag = tag_base + 16 * (*iter_base) + l + 1: must differ between consecutive launches */,
                             bool g1 /* the FiLM scale tiles hold G' */);
hipError_t dc_launch_cond_af16(hipStream_t st, int fmt, const void* a_ca, void* a_ca16, int n_matrices);
int dc_layer16_max_units(void);
hipError_t dc_launch_advance_iter(hipStream_t st, int* iter, int k);
hipError_t dc_launch_set_ptr(hipStream_t st, const float** slot /* 24 bytes: base, seed, first element */, const float* p, unsigned long long seed,
                             unsigned long long first);
// known values (dc_sampler_set_known): the tensors' bases into the 24-byte slot DcUpdate::kslot names; x[known] = ca val + cb noise over n elements
hipError_t dc_launch_set_known(hipStream_t st, const float** slot, const float* val, const float* mask, const float* noise);
hipError_t dc_launch_known_blend(hipStream_t st, float* x, const float* val, const float* mask, const float* noise, float ca, float cb, size_t n);
// Classifier-free guidance (dc_sampler_set_conditioning_guided).  dc_launch_fill_rows64: `rows` rows of dst [rows][64] = v (the null pair
// broadcast over the unconditional clips' frames).  dc_launch_set_scale: the guidance scale into its device slot.
// dc_launch_guided_update: raw = the last layer's model output [2][n] (conditional half, unconditional half; n = B * Tx * P of the
// caller's B clips), x = [2][n]:  x_{t-1} = known_replace(ddim_update(c + (w - 1)(c - u), x_t)) into BOTH halves of x and the due snapshot.
// The step's scalars as the layer epilogue reads them (coef_cur / snap_cur / iter_base / upd: DcLayerArgs).
hipError_t dc_launch_fill_rows64(hipStream_t st, float* dst, size_t rows, const DcNull64& v);
hipError_t dc_launch_set_scale(hipStream_t st, float* slot, float w);
hipError_t dc_launch_guided_update(hipStream_t st, const float* raw, float* x, size_t n, const float* coef_cur, const int* snap_cur, float* snaps,
                                   const int* iter_base, const float* wslot, const DcUpdate& upd);
// Windows of a long piece (dc_sampler_set_conditioning_windows).  xw, raw = the internal x and the last layer's raw output
// [halves][W][Bp][T][P] (halves = 2: the guided shadows behind the conditional clips), xp = the loop's state in piece space [Bp][L][P].
// dc_launch_set_windows: the tables' addresses into the slot.  dc_launch_windows_gather: xw = every window's rows of xp.
// dc_launch_windows_update: blend raw over the covering windows, combine the halves (wslot: the guidance scale), update xp as
// dc_launch_guided_update updates x - noise, known values, x0_prev and snapshots in piece space - and write x_{t-1} to xp and xw.
hipError_t dc_launch_set_windows(hipStream_t st, DcWindows* slot, const int* start, const float* weight);
hipError_t dc_launch_windows_gather(hipStream_t st, const float* xp, float* xw, int halves, int Bp, int W, int T, int L, int P, const DcWindows* slot);
hipError_t dc_launch_windows_update(hipStream_t st, const float* raw, float* xw, float* xp, int halves, int Bp, int W, int T, int L, int P,
                                    const DcWindows* slot, const float* coef_cur, const int* snap_cur, float* snaps, const int* iter_base,
                                    const float* wslot, const DcUpdate& upd);
// N(0, 1) draws of one DDIM iteration (Philox keyed by *seed_slot when given, else seed; iteration = step + *iter_base, else snap_cur[1],
// else step) into z[0..n); z[0] is element `first` (seed_slot[1] when a slot is given) of the whole batch's draw
hipError_t dc_launch_step_noise(hipStream_t st, float* z, size_t n, unsigned long long seed, const unsigned long long* seed_slot, const int* iter_base,
                                int step, const int* snap_cur, unsigned long long first);
// diagnosis: OR DC_STATUS_F16_SAT into *status when the fp16 buffer e holds an inf / nan
hipError_t dc_launch_scan_f16(hipStream_t st, const void* e, size_t bytes, int* status);

// ---- no_eff variant (full T x T attention).  KT = key tiles per clip array.  split: the 128-wide GEMMs on split operands (`dm` is then
// the model record with the split stage images); the attention's own operands stay plain 16-bit.
hipError_t dc_launch_ca_kv(hipStream_t st, int fmt, const DcModel* dm, const void* nh_hi, const void* nh_lo, void* kv_ca,
                           int M, int T, int G, int B, int KT, int L);
hipError_t dc_launch_embed_front_full(hipStream_t st, int fmt, bool split, const DcModel* dm, const float* x, float* hbuf, void* kv_next,
                                      int M, int T, int B, int KT);
hipError_t dc_launch_layer_full(hipStream_t st, int fmt, bool split, const DcLayerArgs& a, int l, const void* kv_cur, void* kv_next,
                                const void* kv_ca, int KT, int stop_after);

// diagnostic builds (-DDC_DIAG_FULL_MOVES): visits / moves of the no_eff key loop's reference point; hipErrorNotSupported otherwise
hipError_t dc_full_moves_read(unsigned long long* out /* [2] */, bool reset);

// Savitzky-Golay smoothing along time of [B][T][P] fp32 (coef: hat matrix [win][win]); y != x
hipError_t dc_launch_savgol(hipStream_t st, const float* x, float* y, const float* coef, int B, int T, int P, int win);
