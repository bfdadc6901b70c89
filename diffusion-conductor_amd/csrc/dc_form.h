// dc_form.h - host-only: which form a denoiser evaluation takes (no kernels, no HIP call, no side effect).  step_form decides the
// launch form of one evaluation from the geometry, the sampler's settings, the environment switches and the step's options;
// clip_stride, steps_per_graph and loop_tail decide the workspace stride, the graph size and the precise tail of a loop; loop_plan
// decides a whole loop - eager or captured, its graphs, their keys and replays - and loop_step the options of each of its steps.
// dc_api.hip launches what they say; tests/form_probe.cpp checks the rules on the CPU (tests/test_host_form.py, _known, _guided, _takes),
// tests/form_probe_windows.cpp those of the windows option (tests/test_host_windows.py).
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "dc_common.h"

// dc_precision of include/dc_ddim.h (dc_api.hip asserts that the two agree)
constexpr int DCF_BF16 = 0, DCF_MIXED = 1, DCF_BF16X3 = 2, DCF_FP16 = 3;

// operand formats (0 = bf16, 1 = f16) and split flags of the 128-wide GEMMs and of the FiLM GEMM
struct Formats {
    int small_fmt = 0, film_fmt = 0;
    bool split_small = false, split_film = false;
    void set_precision(int precision) {
        split_small = precision == DCF_MIXED || precision == DCF_BF16X3;
        split_film = precision == DCF_BF16X3;
        small_fmt = precision == DCF_FP16 ? 1 : 0;
        film_fmt = (precision == DCF_FP16 || precision == DCF_MIXED) ? 1 : 0;
    }
};

// The environment switches that select a launch form or a stride.  One list: the fields, read() and bits() are made from it, so a
// switch step_form can see is in the graph key (loop_plan) by construction.  read() is called once per API call that
// enqueues or sizes the workspace and is never cached: one process can A/B the switches between calls (a change re-captures).
#define DC_FORM_SWITCHES(X)                                                                                                            \
    X(no_wgrec, "DC_NO_WGREC") X(no_narrow, "DC_NO_NARROW") X(no_align, "DC_NO_ALIGN") X(align, "DC_ALIGN")                          \
    X(no_fuse_embed, "DC_NO_FUSE_EMBED") X(film_static, "DC_FILM_STATIC") X(begin_step, "DC_BEGIN_STEP") X(no_pad, "DC_NO_PAD")      \
    X(no_layer16, "DC_NO_LAYER16") X(l16_own_combine, "DC_L16_OWN_COMBINE") X(l16_test_drop_slice, "DC_L16_TEST_DROP_SLICE")         \
    X(tail_film_bf16, "DC_TAIL_FILM_BF16") X(flat_units, "DC_FLAT_UNITS") X(no_embed_next, "DC_NO_EMBED_NEXT")                  \
    X(guide_full_film, "DC_GUIDE_FULL_FILM") X(takes_full_film, "DC_TAKES_FULL_FILM")
struct Switches {
#define X(field, name) bool field = false;
    DC_FORM_SWITCHES(X)
#undef X
    static Switches read() {
        Switches w;
#define X(field, name) w.field = getenv(name) != nullptr;
        DC_FORM_SWITCHES(X)
#undef X
        return w;
    }
    unsigned long long bits() const {      // one bit per switch, in the list's order (<= 16 bits)
        unsigned long long k = 0;
        int i = 0;
#define X(field, name) k |= (field ? 1ull : 0ull) << i++;
        DC_FORM_SWITCHES(X)
#undef X
        return k;
    }
};

// unit records (floats) the workspace holds for `g` token groups: per-group form 2 slots per group; workgroup-record forms two
// alternating buffers of 2 slots per workgroup, i.e. 4 * nwg records with nwg <= ceil(g / 4) (narrow flat units) or B * ceil(T / 128)
// (clip-aligned): both <= g for the T >= 256 those forms need - sized for the larger of the two explicitly, and checked against the
// launch form in step_form
inline size_t rec_capacity(size_t g) { return std::max(g * 2, 4 * ((g + 3) / 4) + 8) * DC_REC_FLOATS; }

struct Geometry {
    int B = 0, T = 0, Tx = 0, G = 0;      // clips, clip stride (clip_stride), the caller's frames per clip, 32-token groups
    int num_cu = 0;
    size_t cap_rec_floats = 0;            // rec_capacity of the workspace
};

// what a guided loop adds to the key of its captured graph (loop_plan; bits 27 and 28): the guided bit - another store in the
// last layer, k_guided_update behind it - and the shared-column bit - the FiLM GEMM's group count and the mapping of the tile reads
inline unsigned long long guided_key_bits(bool guided, bool shared_film) {
    return (guided ? 1ull << 27 : 0ull) | ((guided && shared_film) ? 1ull << 28 : 0ull);
}

// Overlapping windows of a long piece in one loop (dc_sampler_set_conditioning_windows; include/dc_ddim.h states the semantics): the
// geometry's B clips are W windows of Bp pieces each, window-major (twice that under guidance), and the loop's state is one tensor in
// piece space [Bp][L][P].  What such a loop adds to the key of its captured graph (loop_plan): bit 30 - another store in the last
// layer, k_windows_update behind it -, the window count in bits 47 .. 62 and the piece length in the key's last element (the takes'
// wrap period otherwise; windows refuse takes, so the two never meet).  Starts and weights are NOT in the key: the kernels read them
// from device tables, so another plan of the same (Bp, W, T, L) replays the graph.
constexpr int DC_WINDOWS_MAX = 65535;      // windows per piece: what the key's 16 bits hold
constexpr int DC_WINDOWS_COVER = 4;        // windows over one frame, at most
inline unsigned long long windows_key_bits(int W) { return W > 0 ? (1ull << 30 | (unsigned long long)(W & 0xffff) << 47) : 0ull; }

// The plan of such a loop, checked on the host before anything is enqueued: "" or why dc_sampler_set_conditioning_windows refuses it.
// starts[W] ascending from 0 to L - T without a gap (s_{k+1} <= s_k + T), at most DC_WINDOWS_COVER windows over a frame; weight[W][T]
// finite, >= 0, and summing to 1 over the covering windows of every frame within 4 ulp of fp32 (summed in fp64, ascending k).
inline std::string windows_plan_error(const int* start, const float* weight, int W, int T, int L) {
    char buf[200];
    const auto say = [&](const char* fmt, auto... a) { snprintf(buf, sizeof buf, fmt, a...); return std::string(buf); };
    if (!start || !weight) return "windows: the starts h_start[W] or the weights h_weight[W][T] are NULL";
    if (W < 1 || W > DC_WINDOWS_MAX || T < 1 || L < T) return say("windows: need 1 <= W <= %d and L >= T >= 1 (W=%d, T=%d, L=%d)", DC_WINDOWS_MAX, W, T, L);
    if (start[0] != 0) return say("windows: the first window starts at frame %d, not 0", start[0]);
    if (start[W - 1] != L - T) return say("windows: the last window starts at frame %d, not L - T = %d", start[W - 1], L - T);
    for (int k = 1; k < W; ++k) {
        if (start[k] <= start[k - 1]) return say("windows: starts must ascend (window %d starts at %d, window %d at %d)", k - 1, start[k - 1], k, start[k]);
        if (start[k] > start[k - 1] + T) return say("windows: frames [%d, %d) lie in no window", start[k - 1] + T, start[k]);
        if (k >= DC_WINDOWS_COVER && start[k - DC_WINDOWS_COVER] + T > start[k])
            return say("windows: frame %d lies in more than %d windows", start[k], DC_WINDOWS_COVER);
    }
    for (size_t i = 0; i < (size_t)W * T; ++i)
        if (!(weight[i] >= 0.f && weight[i] <= 3.0e38f)) return say("windows: weight[%d][%d] is negative or not finite", (int)(i / T), (int)(i % T));
    int lo = 0;      // the first window that reaches frame f
    for (int f = 0; f < L; ++f) {
        while (start[lo] + T <= f) ++lo;
        double sum = 0.0;
        for (int k = lo; k < W && start[k] <= f; ++k) sum += (double)weight[(size_t)k * T + (f - start[k])];
        if (!(sum >= 1.0 - 4 * 0x1p-23 && sum <= 1.0 + 4 * 0x1p-23)) return say("windows: the weights over frame %d sum to %.9g, not 1 (4 ulp)", f, sum);
    }
    return "";
}

// what the rule reads of a sampler
struct Settings {
    int precision = DCF_FP16;
    Formats fmt;
    bool no_eff = false;
    int clip_aligned = -1;                // dc_sampler_set_clip_aligned
    bool l16_own = false;                 // dc_sampler_set_combine_exchange(s, 0), or latched after a timeout
    int num_layers = 0;
    bool split_model = false;             // the model record with the split stage images exists (fp16 / bf16 precision, on a device)
    bool film_w16 = false, film_w16_tail = false;      // DcModel::film_w16 / film_w16_tail exist
    int l16_max_units = 0;                // dc_layer16_max_units()
    bool idle_wave_path = true;           // dc_sampler_set_idle_wave_path: padding waves of the wide plain layer kernel pass it barrier-only
};

// Test hooks of one evaluation (dc_sampler_debug_denoise, dc_sampler_debug_layer); the defaults run the production evaluation
struct Hooks {
    int layers = -1, stage = 0;   // run the first `layers` layers, the last of them up to `stage` (| (first stage - 1) << 16)
    int first = -1;               // start at this layer from the residual stream in d_h
    bool production() const { return layers < 0 && stage == 0 && first < 0; }
};

// The part of one enqueue_step call that decides its form (dc_api.hip's Step adds the tensors)
struct StepOpts {
    bool loop_mode = false;       // a loop's step: the last layer applies the DDIM update to x_src
    int graph_step = -1;          // >= 0: step number inside a graph being captured
    bool split = false;           // this evaluation's 128-wide GEMMs on split operands (the fp16 images' hi + lo halves)
    bool g1_loop = false;         // a loop with a precise tail: its plain-operand evaluations read G' scale tiles
    bool next_plain = false;      // loops: another step follows in this enqueue sequence (same graph) and it is a plain-operand evaluation
    bool embedded = false;        // the previous step's last layer has embedded x and run layer 0's front half for this step
    bool profile = false;         // events around every launch
    bool known = false;           // loops: known values are set (dc_sampler_set_known): the update replaces them (DC_UPD_KNOWN); no form is given up
    int takes = 1;                // loops: takes per music (dc_sampler_set_conditioning_takes): the conditional clips are `takes` runs of the same
                                  // musics, take-major, and share their FiLM tiles (film_share)
    bool guided = false;          // loops: classifier-free guidance (dc_sampler_set_conditioning_guided): the geometry's B clips are B / 2 conditional
                                  // clips followed by their B / 2 unconditional shadows; the last layer stores the raw model output and
                                  // k_guided_update combines the halves and updates x (no embed_next: x_{t-1} is not in the last layer's registers)
    bool windows = false;         // loops: the clips are overlapping windows of longer pieces (dc_sampler_set_conditioning_windows): the last layer
                                  // stores the raw model output and k_windows_update blends the windows, combines the guided halves when there
                                  // are any, and updates x in piece space (no embed_next, as for `guided`; no takes)
    Hooks dbg;
};

struct StepForm {
    std::string error;            // not empty: the step is refused (DC_ERR_INVALID) and nothing below `rec_stride` is decided
    bool ss = false;              // the 128-wide GEMMs run on split operands (a split format, or a split evaluation of the precise tail)
    bool film_tail = false;       // bf16 precision, split evaluations: the f16 FiLM image - the step is then exactly a "mixed" evaluation
    int fs = 0, ff = 0;           // operand formats of the 128-wide GEMMs and of the FiLM GEMM
    bool fuse_silu = false;       // the FiLM GEMM produces its own operand from pp + temb (no k_silu_emb pass)
    bool folded = false;          // the step's kernels look their timestep up through *d_iter (no k_begin_step launch)
    bool adapt = false;           // adaptive work shares of the persistent FiLM GEMM
    bool wgr = false, narrow = false, aligned = false, layer16 = false, l16_shared = false;
    int upc = 0, upc16 = 0, upc_narrow = 0, nwg = 0;
    size_t rec_stride = 0;        // floats between the two alternating unit-record buffers (0 = single buffer, per-group records)
    bool mixed_form = false, embed_next = false, fuse_embed = false, fuse_extra = false, g1_tiles = false;
    int upd_flags = 0;            // DC_UPD_* bits the form adds to the loop's (TEST_DROP_SLICE, EMBED_NEXT, KNOWN)
    int nl_run = 0, stop_stage = 0;      // layers to run; the stop stage handed to the last of them (0 = the whole layer)
    bool guided = false;          // the last layer writes the raw output of all clips; k_guided_update follows it
    bool windows = false;         // ... k_windows_update follows it (guided or not)
    bool shared_film = false;     // the FiLM GEMM covers film_groups < G groups (film_share): takes wrap, the guided shadow half reads group film_groups - 1
    int film_groups = 0;          // groups the FiLM GEMM computes = the e_groups of the layer kernels' tile reads (nothing shared: G)
    int film_period = 0, film_wrap = 0;      // token group g reads the tiles of group g < film_wrap ? g % film_period : film_groups - 1 (nothing shared: G, G)
    bool idle_path = false;       // wide plain production layer launches: the padding waves of a clip's last workgroup (WgMap, !active) issue
                                  // their shares of the image copies and pass the barriers, nothing else (k_layer, layer_idle_wave)
};

// The token groups the FiLM GEMM has to compute, and which of them a token group reads.  A loop's step has one timestep, so a FiLM tile
// column depends on its token's conditioning alone (emb = SiLU(temb[t] + linear(xf_proj))), never on x: tokens with equal conditioning
// at equal lanes share their tiles bit for bit.
// Takes (dc_sampler_set_conditioning_takes): the conditional clips are `takes` runs of the same Bm musics, take-major.  When one run is a
// whole number Gc = Bm T / 32 of 32-token groups, token group g of take j holds the very tokens of group g - j Gc of take 0 - same
// musics, same frames, same padding rows, whatever the clip stride - and the GEMM runs over one take: group g reads group g % Gc.
// Guided loops: every frame of every unconditional shadow clip carries the same conditioning (the null pair), so every tile column is
// one vector for the whole shadow half.  When the conditional half is a whole number of 32-token groups, the first group of the token
// space's shadow half serves lane n of every shadow group with its lane n:
//   - clip stride == frames per clip (no padding): every lane of every shadow group is a frame of a shadow clip, all with null pp;
//   - clip stride 32 for clips shorter than 32 frames: one group per clip, lane n is frame n of its clip in every group (null pp below
//     the frame count, the padding rows' value above it - zeros from k_cond_pp64, linear(0) from k_cond_embed: by position alone either way);
//   - clip stride padded to whole groups (>= 256 frames): that group holds frames 0 .. 31 of shadow clip 0, all null pp; the padding lanes
//     of later groups then read the null column instead of the padding rows' own - rows that no record, no output and no other token reads.
// The GEMM then runs one more group behind the conditional ones - the null column - and every shadow group reads that last group.
// With `wrap` the groups of all conditional clips and `period` those the GEMM computes of them (Gc, or all of them):
//   tile group of token group g  =  g < wrap ? g % period : groups - 1          (film_tile_group, dc_dev.h; film_magic below)
// Needs the GEMM that builds its operand from pp + temb (non-split FiLM formats).  DC_GUIDE_FULL_FILM=1 keeps all groups of a guided loop,
// DC_TAKES_FULL_FILM=1 all groups of the conditional clips (period = wrap).  Nothing shared: period = wrap = groups = G.
struct FilmShare {
    int period = 0, wrap = 0, groups = 0;
};
inline FilmShare film_share(int B, int T, int G, bool guided, int takes, bool film_from_pp, const Switches& w) {
    const FilmShare full{G, G, G};
    const int Bc = guided ? B / 2 : B;      // conditional clips
    if ((guided && B % 2) || takes < 1 || Bc % takes || !film_from_pp || (guided && w.guide_full_film)) return full;
    const long long mc = (long long)(Bc / takes) * T;      // tokens of one take
    if (mc % 32 != 0) return full;
    const long long gc = mc / 32, wrap = gc * takes;
    if ((guided ? 2 * wrap : wrap) != G) return full;
    // (gc >= 2 and wrap * gc < 2^32: what the kernels' reciprocal needs to exist in 32 bits and to be exact, film_magic - a take of one
    // group is a single clip of at most 32 frames, 65536 groups are two million tokens)
    const int period = (int)((takes > 1 && !w.takes_full_film && gc >= 2 && wrap * gc < (1ll << 32)) ? gc : wrap), groups = period + (guided ? 1 : 0);
    return groups < G ? FilmShare{period, (int)wrap, groups} : full;
}
// The reciprocal the layer kernels take g / period from: with m = floor(2^32 / period) + 1, (g m) >> 32 == g / period for every g with
// g period < 2^32 (the error of g m / 2^32 against g / period is below g / 2^32 < 1 / period) - every g < wrap, by film_share's condition;
// period >= 2, so that m fits 32 bits.
// 0 where nothing wraps (period == wrap): the quotient is then 0 and the kernels read g itself.
inline unsigned film_magic(int period, int wrap) { return period < wrap ? (unsigned)((1ull << 32) / (unsigned)period) + 1u : 0u; }
// what takes add to the key of a captured graph (GraphKey, loop_plan): the period the tile reads wrap at, 0 where no take shares another's
// tiles - 2 takes x 2 musics and a plain 4-clip conditioning have one internal geometry and different launches
inline int takes_key_period(const FilmShare& f) { return f.period < f.wrap ? f.period : 0; }

// split-operand evaluations (the precise tail, dc_sampler_set_precise_forward) exist for: fp16 / bf16 precision, no test hooks
inline bool can_split_steps(const Settings& s, const Hooks& dbg) {
    return (s.precision == DCF_FP16 || s.precision == DCF_BF16) && dbg.production() && s.split_model;
}

// One denoiser evaluation (+ DDIM update when loop_mode).  `stamps`: the process collects clock stamps (DC_STAMPS).
// graph_step >= 0: step number inside a graph being captured.  On the default path (fused SiLU fill, per-layer launches) the
// step's kernels then look the timestep / DDIM scalars up themselves - this step's slot of the per-iteration tables, offset by
// the iteration at which the replay began (*d_iter, advanced once per replay) - and the per-step bookkeeping launch
// (k_begin_step, 5 us + a launch gap) is dropped: `folded`.
inline StepForm step_form(const Geometry& g, const Settings& s, const Switches& w, const StepOpts& o, bool stamps) {
    StepForm f;
    const int B = g.B, T = g.T, G = g.G;
    const Hooks& dbg = o.dbg;
    if (o.guided && !(o.loop_mode && B % 2 == 0 && dbg.production())) {
        f.error = "internal: a guided evaluation is a loop step over an even number of internal clips";
        return f;
    }
    const bool guided = f.guided = o.guided;
    if (o.windows && !(o.loop_mode && dbg.production())) {
        f.error = "internal: an evaluation over windows is a loop step";
        return f;
    }
    if (o.windows && o.takes != 1) {
        f.error = "windows do not combine with takes";
        return f;
    }
    f.windows = o.windows;
    // "no test hook, no stamps": what the production-only forms below ask for.  Conditions that name single hooks instead are meant
    // as they stand, and say why.
    const bool quiet = dbg.production() && !stamps;
    const bool ss = f.ss = s.fmt.split_small || o.split, sf = s.fmt.split_film;
    f.film_tail = o.split && !s.fmt.split_small && s.film_w16_tail && !w.tail_film_bf16;
    const int fs = f.fs = s.fmt.small_fmt, ff = f.ff = f.film_tail ? 1 : s.fmt.film_fmt;
    // non-split formats: the FiLM GEMM produces its own operand from pp + temb (no k_silu_emb pass); the separate pass
    // remains for the split formats, for the v1 kernel, and under the test hooks that read the operand image back
    // (`layers` alone: `stage` stops inside a layer, after the GEMM; `first` never comes without `layers`, dc_sampler_debug_layer)
    const bool fuse_silu = f.fuse_silu = !sf && dbg.layers < 0;
    // (`stage` beside fuse_silu's `layers`; `first` never comes without `layers`.  Captured steps are loop steps and carry no hook anyway)
    f.folded = o.loop_mode && o.graph_step >= 0 && fuse_silu && !s.no_eff && !w.begin_step && dbg.stage == 0;
    // adaptive work shares of the persistent FiLM GEMM (dc_kernels.hip, film_shares); DC_FILM_STATIC=1 keeps equal shares
    f.adapt = !w.film_static && g.num_cu <= 1024;
    if (o.takes < 1 || (guided ? B / 2 : B) % o.takes != 0) {
        f.error = "internal: the conditional clips are not a whole number of takes";
        return f;
    }
    const FilmShare share = film_share(B, T, G, guided, o.takes, fuse_silu, w);
    f.film_groups = share.groups, f.film_period = share.period, f.film_wrap = share.wrap;
    f.shared_film = f.film_groups < G;
    f.nl_run = (dbg.layers >= 0 && dbg.layers < s.num_layers) ? dbg.layers : s.num_layers;
    // (full attention: the last layer of a shortened run stops after its FFN block)
    f.stop_stage = s.no_eff ? (dbg.stage ? dbg.stage : (f.nl_run < s.num_layers ? 3 : 0)) : dbg.stage;
    // ---- form of the layer launches (linear attention) --------------------------------------------------------------------
    // workgroup-level records (no combine launches) whenever a workgroup's 256 tokens cannot touch more than two clips
    // (`first` alone: k_front_from_h, which starts a run at a later layer, writes per-group records only.  Split formats: on
    // clip-aligned units only - the doubled weight images leave LDS for ONE clip's attention fragments - and in the production build
    // only: the test hooks keep the per-group form)
    const bool wgr = f.wgr = T >= 256 && !w.no_wgrec && dbg.first < 0 && !s.no_eff && (!ss || (T % 32 == 0 && dbg.production() && !w.no_align));
    // Narrow workgroups (4 waves = 128-token units, one wave per SIMD) while every unit still gets a CU of its own: the layer
    // kernel is bound by instruction issue, so a wave alone on its SIMD runs a layer in about half the time (DESIGN.md
    // section 4).  T <= 3840: the narrow combine holds 32 units per clip.  DC_NO_NARROW=1 keeps the 8-wave form.
    // Clip-aligned units (WgMap in dc_dev.h; needs a clip stride of whole groups): upc workgroups per clip, no workgroup spans two
    // clips.  Default for the narrow (small-batch) form; with the chip full (bs=32 x 1800: 256 workgroups instead of 228 flat
    // units) it measured 1.2 % slower than flat units - DC_ALIGN=1 forces it there.
    const bool can_align = wgr && T % 32 == 0 && !w.no_align;
    const int upc_wide = (T + 255) / 256, upc_narrow = f.upc_narrow = (T + 127) / 128;
    const bool aligned_env = can_align && w.align;
    const int nwg_narrow = can_align ? B * upc_narrow : (G + 3) / 4;
    const bool narrow = f.narrow = wgr && !ss && nwg_narrow <= g.num_cu && T <= 3840 && quiet && !w.no_narrow;
    // ... and for the wide (chip-full) form whenever the clip-aligned launch needs no more rounds of workgroups over the chip than the flat
    // one (bs = 32 x 1800: 256 workgroups instead of 228, one round either way): a clip's result is then bit-identical whatever the
    // batch around it - the reference's semantics (transformer.py:111: the key softmax is per clip) - for +1.6 ... +2.1 % per loop
    // (profiles/r06_ab_align.txt) while the padding waves of a clip's last workgroup ran the whole layer, +0.1 % since they pass it
    // barrier-only (idle_path below; profiles/idle_waves_ab.txt).  Where it would cost a round (bs = 35 x 1800: 280 against 250 workgroups on 256 CUs) flat units stay -
    // a clip then depends on its neighbours at the rounding level (4e-4).  dc_sampler_set_clip_aligned: 1 forces
    // aligned units, 0 flat ones; DC_ALIGN=1 / DC_FLAT_UNITS=1 in the environment do the same per process.
    const int nwg_flat = (G + 7) / 8, ncu = g.num_cu > 0 ? g.num_cu : 256;
    const bool same_rounds = ((long long)B * upc_wide + ncu - 1) / ncu == ((long long)nwg_flat + ncu - 1) / ncu;
    const bool aligned_wide = s.clip_aligned > 0 || aligned_env || (s.clip_aligned < 0 && same_rounds && !w.flat_units);
    const bool aligned = f.aligned = can_align && (narrow || ss || aligned_wide);
    // 16-token waves (dc_layer16.hip) while every clip-aligned 64-token unit still gets a CU of its own (bs <= 8 at T = 1800): in that
    // regime the layer is bound by the LENGTH of one wave's dependency chain, and a 16-token wave's is about half as long.  The
    // embedding stays the narrow 32-token form (its 128-token unit records feed layer 0).  DC_NO_LAYER16=1 keeps the 32-token form.
    // (`first` is what k_layer16 itself cannot do - it has no stop stage either, but `narrow` has already excluded every hook)
    const int upc16 = f.upc16 = (T + 63) / 64;
    const bool layer16 = f.layer16 = narrow && aligned && (long long)B * upc16 <= g.num_cu && upc16 <= s.l16_max_units && dbg.first < 0 && !w.no_layer16;
    const int upc = f.upc = aligned ? (narrow ? upc_narrow : upc_wide) : 0;
    const int nwg = f.nwg = aligned ? B * upc : (narrow ? (G + 3) / 4 : (G + 7) / 8);
    // k_layer16: the clip's workgroups share the combine of the previous layer's unit records inside the launch (dc_layer16.hip;
    // DC_L16_OWN_COMBINE=1: every workgroup combines alone, round 4's form)
    f.l16_shared = layer16 && !s.l16_own && !w.l16_own_combine;
    f.rec_stride = wgr ? (size_t)nwg * 2 * DC_REC_FLOATS : 0;
    // (the kernels write records at recs + rec_stride + wg * 2 * DC_REC_FLOATS: both alternating buffers must lie inside d_recs)
    const size_t rec_floats = wgr ? 2 * f.rec_stride : (size_t)G * 2 * DC_REC_FLOATS;
    if (rec_floats > g.cap_rec_floats) {
        char buf[160];
        snprintf(buf, sizeof buf, "unit records of this launch form (%zu floats) exceed the workspace (%zu)", rec_floats, g.cap_rec_floats);
        f.error = buf;
        return f;
    }
    // k_embed_front rides in the FiLM GEMM's launch (wide flat units, non-split formats, no test hooks; DC_NO_FUSE_EMBED=1 and the
    // per-kernel profile pass keep the two launches): one kernel boundary less per step, -1.3 % per loop at bs=32
    // (flat units in the non-split formats; the "mixed" mode - f16 GEMM, split-bf16 embedding - on its clip-aligned units)
    const bool mixed_form = f.mixed_form = ss && !sf && ff == 1 && fs == 0;
    // The last layer of a plain wide step does the NEXT step's front work (embedding of x_{t-1} + layer 0's self-attention front half:
    // k_layer, DC_UPD_EMBED_NEXT) when that step is a plain wide step of the same enqueue sequence; its FiLM launch is then the bare GEMM
    // and it has no front launch.  DC_NO_EMBED_NEXT=1 keeps the front work in every step's own FiLM launch.
    const bool wide_plain = wgr && !narrow && !ss && fuse_silu && ff == fs && quiet && !s.no_eff;
    // (a guided step's update runs in k_guided_update, behind the last layer: there is no x_{t-1} in that layer's registers to embed)
    // (nor a step's over windows: its update runs in k_windows_update, in piece space)
    f.embed_next = !w.no_embed_next && o.loop_mode && o.next_plain && wide_plain && !guided && !o.windows;
    // The padding waves of that kernel (clip-aligned units at 1800 frames: 7 of the 8 waves of every clip's last workgroup, 11 % of the
    // launch's waves) do a workgroup member's duties only; dc_sampler_set_idle_wave_path(s, 0) has them run the whole layer as before
    // (results are bit-identical either way: nothing of theirs ever reached an output).  Only the instantiation without hooks and stamps
    // has the path; the others ignore the flag.
    f.idle_path = s.idle_wave_path && wgr && !narrow && !ss && quiet && !s.no_eff;
    if (o.embedded && !(o.loop_mode && wide_plain)) {
        f.error = "internal: a step whose front work was done by its predecessor changed its launch form";
        return f;
    }
    // (a FiLM launch that carries the embedding hands it its own group count: with the shadow half's shared column the GEMM covers
    // fewer groups than the embedding, and the two launches stay apart - the form the profile pass runs)
    f.fuse_embed = !o.embedded && wgr && !narrow && (ss ? (aligned && mixed_form) : ff == fs) && fuse_silu && quiet && nwg <= g.num_cu &&
                   !o.profile && !w.no_fuse_embed && !f.shared_film;
    // small batches (narrow clip-aligned units): the embedding's workgroups ride BEHIND the GEMM's in the FiLM launch
    // (film_extra_workgroups, dc_kernels.hip): one launch (15 us at one clip) and one kernel boundary less per step.  DC_NO_FUSE_EMBED=1 keeps the two launches.
    // (`first`: there is no embedding to fuse when the run starts from d_h; `narrow` has already excluded every hook)
    f.fuse_extra = narrow && aligned && !ss && ff == fs && fuse_silu && s.film_w16 && dbg.first < 0 && !o.profile && !w.no_fuse_embed &&
                   !f.shared_film;
    f.upd_flags = (w.l16_test_drop_slice ? DC_UPD_TEST_DROP_SLICE : 0) | (f.embed_next ? DC_UPD_EMBED_NEXT : 0) |
                  ((o.known && o.loop_mode) ? DC_UPD_KNOWN : 0);
    // scale tiles: G' for the plain-operand consumers of this step, G' - 1 for the split-operand ones (dc_dev.h, film_affine)
    // (the production forms of the plain-operand kernels only: test hooks, stamps and the per-group record form keep G' - 1)
#ifndef DC_NO_FILM_G1
    f.g1_tiles = o.g1_loop && !ss && wgr && !s.no_eff && quiet;
#endif
    return f;
}

// Clip stride of the internal token space.  Where the workgroup-record kernels can run (non-split formats, linear attention,
// Tx >= 256) a clip may be padded to whole 32-token groups, so that no group spans two clips (the padding frames behave like
// frames past `length`).  Measured (same box): bs=32 x 1800 (+1.3 % tokens) -1.6 % per loop; bs=128 x 900
// (+3.1 %) +0.2 %; small batches, which then also run clip-aligned units (step_form), -9 % at bs=4 x 1800.
inline int clip_stride(const Settings& s, const Switches& w, int B, int Tx, int num_cu) {
    // clips shorter than one 32-token group: one group per clip (a group's records name at most two clips)
    if (Tx < 32 && !s.no_eff && !w.no_pad) return 32;
    if (s.no_eff || Tx < 256 || Tx % 32 == 0 || w.no_pad) return Tx;
    const int Tp = (Tx + 31) / 32 * 32;
    if (s.fmt.split_small) return Tp;      // split formats: workgroup records exist on clip-aligned units only (one clip per workgroup)
    const bool small_batch = (long long)B * ((Tp + 127) / 128) <= num_cu;       // narrow, clip-aligned workgroups
    // ... unless the padding frames cost the layer launches a whole extra round of workgroups (256 tokens each, one per CU): 36 clips of
    // 1800 frames are 254 workgroups, of 1824 frames 257 - 38 vs 51 ms per loop (profiles/r05_big_batches.md)
    const auto rounds = [&](int T) { return (((long long)B * T + 255) / 256 + num_cu - 1) / num_cu; };
    if (!small_batch && rounds(Tp) > rounds(Tx)) return Tx;
    return (small_batch || (Tp - Tx) * 50 <= Tx) ? Tp : Tx;
}

// steps of a loop one captured graph holds: the whole loop up to 64 steps, else the largest divisor of S up to 64
inline int steps_per_graph(int S) {
    if (S <= 64) return S;
    for (int k = 64; k >= 1; --k)
        if (S % k == 0) return k;
    return 1;
}

#ifndef DC_BF16_TAIL_DEFAULT
#define DC_BF16_TAIL_DEFAULT 6
#endif
#ifndef DC_BF16_SHORT_CLIP
#define DC_BF16_SHORT_CLIP 100     // bf16 precision: loops over clips of fewer frames run every evaluation split (loop_tail)
#endif
inline int precise_tail_default(int precision) { return precision == DCF_FP16 ? 1 : precision == DCF_BF16 ? DC_BF16_TAIL_DEFAULT : 0; }

// Precise tail of a loop of S steps: its last `tail` model evaluations run on split operands (tail_split: dc_sampler_set_precise_tail,
// -1 = by precision; env_tail: DC_PRECISE_TAIL=k, which overrides it; flags: DC_UPD_*): fp16 / bf16 precision, no test hooks.
struct LoopTail {
    int tail;          // split evaluations at the end of the loop's last graph (0 ... steps_per_graph(S))
    bool tail_all;     // every evaluation of the loop is split (every replay's graph, then)
};
inline LoopTail loop_tail(const Settings& s, int tail_split, std::optional<int> env_tail, int flags, int Tx, int S) {
    int tail = tail_split >= 0 ? tail_split : precise_tail_default(s.precision);
    bool tail_asked = tail_split >= 0;
    if (env_tail) tail = *env_tail, tail_asked = true;
    // An EPSILON model's final sample is sqrt(1 / abar) x_t - sqrt(1 / abar - 1) eps, not the last evaluations' prediction: what the plain
    // 16-bit evaluations left in x_t stays (eta = 0: fp16 1.4 - 1.8e-3 whatever the tail, tools/fuzz_sampler.py).  Parity first: unless a
    // tail was asked for, such a loop runs EVERY evaluation on split operands (2.1e-4, at the split precisions' speed).
    if (!tail_asked && (flags & DC_UPD_EPS)) tail = S;
    // Clips of fewer than 100 frames in the bf16 precision: a clip's error is a norm over a few hundred numbers (26 per frame), and the worst of
    // a batch of dozens of such clips reached 1.27e-3 with the default tail (39 clips of 36 frames, lengths down to 1: tools/fuzz_shapes.py,
    // profiles/r06_fuzz_final.txt; 8.6e-4 at 39 frames, <= 7.2e-4 from 100 frames up).  Such loops are bound by launch latency, not by the
    // kernels: they run every evaluation in the split form (the `mixed` precision's evaluations, 9e-5) unless a tail was asked for.
    if (!tail_asked && s.precision == DCF_BF16 && Tx < DC_BF16_SHORT_CLIP) tail = S;
    // (clip strides that are not whole 32-frame groups - T = 900 x 128 unpadded - and short clips run the split evaluations in the
    // per-group record form with its combine launches: no measurable cost at one evaluation per loop, 70.6 vs 70.6 ms at bs = 128 x 900)
    if (!can_split_steps(s, Hooks{})) tail = 0;
    // (a tail of the whole loop splits every replay's graph; any shorter one lives in the last replay and is clipped to its steps)
    const bool tail_all = tail >= S;
    return {std::max(0, std::min(tail, std::min(S, steps_per_graph(S)))), tail_all};
}

// ---- the loop: which graphs it replays how often, and what each of their steps is (dc_api.hip's loop_common executes the plan) ----------
// What a captured graph bakes in: (B, T, Tx, steps, form bits, takes_key_period).  The form bits, built in loop_plan alone:
//   0 .. 15  the environment switches (Switches::bits: every switch step_form can see)
//   16 .. 23 the loop's DC_UPD_* flags (the noise / known tensors' addresses are not baked in: the kernels read them from their slots)
//   24       l16_own            25, 26  clip_aligned + 1            27, 28  guided_key_bits
//   29       the padding waves' barrier-only path is OFF (Settings::idle_wave_path; set when off, so the default's key is what it was)
//   30       the clips are windows of longer pieces (windows_key_bits; their count in bits 47 .. 62, the piece length in the last element)
//   39       the loop has a precise tail: its plain evaluations read G' scale tiles, those of a loop without one G' - 1 tiles
//   40 ..    the split evaluations at the end of this graph
using GraphKey = std::tuple<int, int, int, int, unsigned long long, int>;

struct LoopOpts {
    int S = 1;                    // iterations
    int flags = 0;                // DC_UPD_* of the loop, the internal NOISY / ZSTEP / MULTISTEP / KNOWN bits resolved
    bool guided = false;          // the conditioning (StepOpts::guided, ::takes)
    int takes = 1;
    int windows = 0, win_L = 0;   // windows per piece and frames per piece (dc_sampler_set_conditioning_windows); 0: none (StepOpts::windows)
    bool profile = false;         // events around every launch: an eager loop
    bool no_graph = false;        // DC_DISABLE_GRAPH: an eager loop
    int tail_split = -1;          // loop_tail's arguments
    std::optional<int> env_tail;
};
struct LoopPart {
    int steps = 0;                // steps of one enqueue sequence (captured: of the graph) ...
    int split_n = 0;              // ... the last split_n of them on split operands
    int launches = 1;             // replays of the graph
    GraphKey key{};               // captured parts
};
struct LoopPlan {
    bool g1_loop = false;         // the loop has a precise tail
    bool eager = false;           // one part, enqueued on the stream itself
    std::vector<LoopPart> parts;
};
inline LoopPlan loop_plan(const Geometry& g, const Settings& s, const Switches& w, const LoopOpts& o) {
    const LoopTail lt = loop_tail(s, o.tail_split, o.env_tail, o.flags, g.Tx, o.S);
    LoopPlan p;
    p.g1_loop = lt.tail > 0, p.eager = o.profile || o.no_graph;
    if (p.eager) {
        p.parts.push_back({o.S, lt.tail_all ? o.S : lt.tail, 1, GraphKey{}});
        return p;
    }
    const FilmShare share = film_share(g.B, g.T, g.G, o.guided, o.takes, !s.fmt.split_film, w);
    const unsigned long long bits = w.bits() | (unsigned long long)(o.flags & 0xff) << 16 | (s.l16_own ? 1ull : 0ull) << 24 |
                                    (unsigned long long)((s.clip_aligned + 1) & 3) << 25 | guided_key_bits(o.guided, share.groups < g.G) |
                                    (s.idle_wave_path ? 0ull : 1ull) << 29 | windows_key_bits(o.windows) | (p.g1_loop ? 1ull : 0ull) << 39;
    const int K = steps_per_graph(o.S), replays = o.S / K;
    const auto part = [&](int split_n, int launches) {
        p.parts.push_back({K, split_n, launches, GraphKey{g.B, g.T, g.Tx, K, bits | (unsigned long long)split_n << 40,
                                                                  o.windows > 0 ? o.win_L : takes_key_period(share)}});
    };
    // (with a precise tail and several replays per loop - S > 64 - the LAST replay runs a second graph whose final steps are split)
    if (lt.tail && replays > 1) {
        part(lt.tail_all ? K : 0, replays - 1);
        part(lt.tail, 1);
    } else {
        part(replays == 1 ? lt.tail : (lt.tail_all ? K : 0), replays);
    }
    return p;
}
// step i of a part (`embedded` is the executor's: StepDone::embedded_next of step i - 1)
inline StepOpts loop_step(const LoopPlan& p, const LoopPart& part, const LoopOpts& o, int i) {
    StepOpts c;
    c.loop_mode = true, c.graph_step = p.eager ? -1 : i, c.split = i >= part.steps - part.split_n, c.g1_loop = p.g1_loop;
    c.next_plain = i + 1 < part.steps - part.split_n, c.profile = o.profile, c.known = (o.flags & DC_UPD_KNOWN) != 0;
    c.guided = o.guided, c.takes = o.takes, c.windows = o.windows > 0;
    return c;
}
