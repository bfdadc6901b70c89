// dc_api.hip - host side of libdc_ddim.so: parameter packing, workspace, step enqueue,
// hipGraph capture/replay and the C ABI declared in include/dc_ddim.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/dc_ddim.h"
#include "dc_common.h"
#include "dc_form.h"
#include "dc_launch.h"
#include "dc_music.h"
#include "dc_pack.h"

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(DC_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

enum KernelId { K_BEGIN = 0, K_SILU, K_FILM, K_EMBED, K_COMBINE, K_LAYER, K_NOISE, K_GUIDE, K_WINDOWS, K_COUNT };
const char* kKernelNames[K_COUNT] = {"k_begin_step", "k_silu_emb", "k_film_gemm", "k_embed_front", "k_attn_combine", "k_layer", "k_step_noise",
                                     "k_guided_update", "k_windows_update"};

struct Prof {                       // per-kernel profile (dc_sampler_profile_loop): events around every launch
    std::vector<hipEvent_t> ev;     // pairs
    std::vector<int> ids;
};

}  // namespace

struct dc_sampler : Formats {     // (set_precision(cfg.precision))
    dc_config cfg{};
    std::map<std::string, std::vector<float>> params;
    bool finalized = false;

    uint8_t* d_arena = nullptr;
    size_t arena_bytes = 0;
    DcModel* d_model = nullptr;
    DcModel h_model{};
    int NT = 0;   // FiLM feature tiles = 3 * L * 8

    hipStream_t stream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;

    // workspace (capacity-tracked)
    int B = 0, T = 0, M = 0, G = 0;          // T: clip stride of the token space (the caller's frames per clip, padded: below)
    int Tx = 0;                              // the caller's frames per clip: x, xf, snapshots are [B][Tx][..]
    size_t cap_G = 0, cap_B = 0, cap_MP = 0, cap_steps = 0, cap_snap = 0, cap_kv = 0;
    size_t cap_rec_floats = 0;      // floats behind d_recs
    std::vector<int> len_dev;       // the clip lengths d_length holds (dc_sampler_set_conditioning), valid while len_dev_ptr == d_length
    const int* len_dev_ptr = nullptr;
    int* d_length = nullptr;
    float* d_pp = nullptr;
    void *d_s_hi = nullptr, *d_s_lo = nullptr;
    void* d_E = nullptr;
    float* d_h = nullptr;
    float* d_recs = nullptr;
    void *d_a_sa = nullptr, *d_a_ca = nullptr;
    void* d_a_ca16 = nullptr;             // cross-attention fragments in the 16-token layer kernel's form (small batches)
    unsigned long long* d_gran = nullptr; // small batches: granules of the combine the clip's workgroups share inside a launch, [B][1024] (dc_layer16.hip)
    unsigned l16_seq = 0;                 // eager launches of k_layer16: tag sequence (tags must differ between consecutive launches)
    bool l16_own = false;                 // every workgroup of k_layer16 combines alone (no in-launch exchange): dc_sampler_set_combine_exchange(s, 0),
                                          // or latched by dc_sampler_status after a DC_STATUS_TIMEOUT (the GPU is shared: co-residency cannot be assumed)
    void *d_kv_sa[2] = {nullptr, nullptr}, *d_kv_ca = nullptr;   // no_eff: key-tile arrays (dc_kernels.hip, full attention)
    int KT = 0;                                                   // key tiles per clip array
    float* d_x = nullptr;
    float* d_snaps = nullptr;
    // conditioning temporaries
    float* d_recs_ca = nullptr;
    void *d_nh_hi = nullptr, *d_nh_lo = nullptr;
    // step state
    unsigned long long* d_stamps = nullptr;
    float* d_film_rate = nullptr;  // FiLM GEMM: per-workgroup speeds measured by the previous launches, two buffers of 1024 (ping-pong)
    int film_rate_parity = 0;
    int num_cu = 0;
    int *d_iter = nullptr, *d_t_clip = nullptr, *d_snap_cur = nullptr, *d_t_of_iter = nullptr, *d_snap_of_iter = nullptr;
    float *d_coef_cur = nullptr, *d_coef_of_iter = nullptr;   // the update's scalars: this step's row / every row, by ITERATION (only d_t_of_iter holds timesteps)
    bool cond_set = false;
    int64_t ws_bytes = 0;
    std::map<void*, size_t> alloc_bytes;   // live workspace allocations (ws_bytes = their sum)
    // host copies of the per-iteration tables currently on the device (tables_S == 0: none)
    int tables_S = 0;
    std::vector<int> tab_t, tab_snap;
    std::vector<float> tab_coef_iter;

    // graph cache, keyed by the GraphKey loop_plan (dc_form.h) builds for the captured launches: the current graph (the last entry) and
    // up to three parked ones for other batch shapes (a dataset's last, smaller batch; a service whose batch size varies): a shape
    // seen before replays its graph instead of paying a capture (tens of ms) every time the shape changes.  The workspace's
    // addresses are baked into every captured graph, so whatever re-allocates a buffer drops them all (drop_graph); find_or_capture
    // is the cache's only other entry.
    std::vector<std::pair<GraphKey, hipGraphExec_t>> graphs;
    // DDIM update options of the loop being enqueued (dc_sampler_ddim_loop_ex) and the device status word
    int upd_flags = 0;              // DC_UPD_* of the loop being enqueued (incl. the internal NOISY / ZSTEP bits)
    const float** d_zslot = nullptr;    // device slot holding the base address of the per-iteration noise (DcUpdate::zslot)
    float* d_zstep = nullptr;       // library-generated draws of one iteration [B][Tx][P] (dc_sampler_set_step_noise_seed)
    size_t cap_zstep = 0;
    unsigned long long noise_seed = 0, noise_first = 0;      // Philox key; index of this sampler's first element in the whole batch's draw
    bool noise_seed_set = false;                             // a seed is consumed by the loop that uses it
    int* d_status = nullptr;
    float* d_x0_prev = nullptr;     // DC_UPD_MULTISTEP: the previous step's predicted x0 [user_B][Tx][P], zeroed when such a loop starts
    size_t cap_x0_prev = 0;
    // known values (dc_sampler_set_known): the caller's three [B][Tx][P] tensors, valid for the conditioning they were set for; the kernels
    // read their addresses from d_kslot
    const float *known_val = nullptr, *known_mask = nullptr, *known_noise = nullptr;
    struct KnownFor {             // the CALLER's clips and frames, whether the conditioning was guided, and its takes per music (the same clips
        int user_B = 0, Tx = 0;   // in another take order are another geometry): a loop over any other conditioning clears the tensors
        bool guided = false;
        int takes = 1;
        int win_W = 0, win_L = 0; // windows: the caller's tensors are [pieces][L][P]
        bool operator==(const KnownFor& o) const {
            return user_B == o.user_B && Tx == o.Tx && guided == o.guided && takes == o.takes && win_W == o.win_W && win_L == o.win_L;
        }
    } known_set_for;
    KnownFor known_for() const { return {user_B(), Tx, guided, takes, win_W, win_L}; }      // ... of the current conditioning
    const float** d_kslot = nullptr;
    // Savitzky-Golay smoothing applied by the loop's final write (dc_sampler_set_smoothing; window 0 = off)
    int smooth_window = 0, smooth_order = 0, smooth_table_window = 0;     // (table_window: the hat matrix d_smooth_coef holds)
    float* d_smooth_coef = nullptr;
    // Classifier-free guidance (dc_sampler_set_conditioning_guided): B above is then the INTERNAL batch, the caller's B / 2 clips followed by
    // their unconditional shadows; the caller's tensors (noise, out, snapshots, step noise, known values) stay [B / 2][Tx][P]
    bool guided = false;
    float guide_w = 1.f;            // guidance scale; travels through d_wslot, so another scale replays the same graph
    float* d_wslot = nullptr;
    float* d_raw = nullptr;         // the last layer's raw model output of all internal clips [B][Tx][P]
    size_t cap_raw = 0;
    float *d_xf2_proj = nullptr, *d_xf2_out = nullptr;      // feature images [B][Tx][64] of the internal batch (second half: the null pair)
    size_t cap_xf2_proj = 0, cap_xf2_out = 0;
    int user_B() const { return (guided ? B / 2 : B) / (win_W > 0 ? win_W : 1); }       // clips of the caller's tensors (takes x the musics; windows: pieces)
    // Windows of longer pieces (dc_sampler_set_conditioning_windows): B is win_W windows x the caller's pieces, window-major (x 2 guided);
    // the caller's tensors and the loop's state d_xp are [pieces][win_L][P], d_x holds the windows' slots for the model to read.
    // d_win_start / d_win_weight: the plan's tables, d_winslot the slot that names them (k_windows_gather, k_windows_update)
    int win_W = 0, win_L = 0;
    int user_frames() const { return win_W > 0 ? win_L : Tx; }       // frames per clip of the caller's tensors
    size_t user_elems() const { return (size_t)user_B() * user_frames() * cfg.input_feats; }
    float* d_xp = nullptr;
    size_t cap_xp = 0;
    int* d_win_start = nullptr;
    float* d_win_weight = nullptr;
    size_t cap_win_start = 0, cap_win_weight = 0;
    DcWindows* d_winslot = nullptr;
    // Takes (dc_sampler_set_conditioning_takes): the conditional clips are `takes` runs of the same musics, take-major; the feature images of
    // the internal batch live in d_xf2_* as they do for guidance
    int takes = 1;
    // guided takes: the operand image of a FiLM GEMM over one take + the null column (film_share: Gc + 1 groups) - the first Gc groups of
    // d_pp, then its first shadow group.  (In d_pp itself group Gc is take 1's first group, and the GEMM reads its groups in order.)
    float* d_pp_share = nullptr;
    size_t cap_pp_share = 0;
    const float* pp_last = nullptr;      // the operand image the last enqueued step's FiLM GEMM read (dc_sampler_status re-runs it)
    int last_film_groups = 0;       // groups of d_E the last enqueued step's FiLM GEMM wrote (dc_sampler_status scans no others)

    DcModel h_model_split{};     // fp16 precision: the same model with the layer stage images in their split form ([hi][lo][consts]): the loop's precise tail
    DcModel* d_model_split = nullptr;
    dc_music* music = nullptr;   // MusicEncoder (built when its parameters were supplied)
    int me_format = -1;          // dc_sampler_set_encoder_format (-1: by precision)
    int clip_aligned = -1;         // dc_sampler_set_clip_aligned: 1 clip-aligned units in the wide form too, 0 flat units, -1 the library's rule
    bool idle_wave_path = true;    // dc_sampler_set_idle_wave_path: padding waves of the wide plain layer kernel pass it barrier-only (0: they run the whole layer)
    bool precise_forward = false;  // dc_sampler_set_precise_forward: dc_sampler_denoise on split operands (the precise tail's evaluation form)
    int tail_split = -1;         // dc_sampler_set_precise_tail: the loop's last evaluations with split operands (-1: by precision - fp16 1, bf16 DC_BF16_TAIL_DEFAULT = 6)
    bool host_only = false;      // -DDC_HOST_SANITIZE builds without a device: the host half only (tests/test_host_sanitize.py)

    Prof prof;
    bool diag_film_done = false;          // DC_DIAG_SKIP_FILM (diagnostic): the FiLM GEMM has been launched once on this sampler
};

namespace {

// (Re)allocates one workspace buffer.  The caller's capacity field is only raised after every buffer of its group was
// allocated (ensure_workspace resets it to 0 first), so a failed hipMalloc leaves "no capacity", never a stale one.
template <class P>
int dev_alloc(dc_sampler* s, P*& p, size_t bytes) {
    if (p) {
        auto it = s->alloc_bytes.find((void*)p);
        if (it != s->alloc_bytes.end()) {
            s->ws_bytes -= (int64_t)it->second;
            s->alloc_bytes.erase(it);
        }
        void* old = (void*)p;
        p = nullptr;
        HIP_TRY(hipFree(old));
    }
    void* q = nullptr;
    HIP_TRY(hipMalloc(&q, bytes));
    p = (P*)q;
    s->alloc_bytes[q] = bytes;
    s->ws_bytes += (int64_t)bytes;
    return DC_OK;
}

void drop_graph(dc_sampler* s) {
    for (auto& g : s->graphs) hipGraphExecDestroy(g.second);
    s->graphs.clear();
}

// Grows one buffer with a capacity of its own to `need` elements of `elem_bytes`.  in_graphs: the buffer's address is an argument of
// captured launches, so a new one drops the graphs.  The capacity follows dev_alloc's rule: reset first, raised last.
template <class P>
int grow(dc_sampler* s, P*& p, size_t& cap, size_t need, size_t elem_bytes, bool in_graphs) {
    if (need <= cap) return DC_OK;
    if (in_graphs) drop_graph(s);
    cap = 0;
    if (int rc = dev_alloc(s, p, need * elem_bytes)) return rc;
    cap = need;
    return DC_OK;
}

const std::vector<float>* find(dc_sampler* s, const std::string& n) {
    auto it = s->params.find(n);
    return it == s->params.end() ? nullptr : &it->second;
}

struct ParamReq {
    std::string name;
    size_t numel;
};

std::vector<ParamReq> required_params(const dc_config& c) {
    std::vector<ParamReq> r;
    const size_t D = c.latent_dim, E = 4 * D, L = 512, F = c.ff_size, P = c.input_feats;
    r.push_back({"sequence_embedding", (size_t)c.num_frames * D});
    r.push_back({"linear.weight", L * 64});
    r.push_back({"linear.bias", L});
    r.push_back({"joint_embed.weight", D * P});
    r.push_back({"joint_embed.bias", D});
    r.push_back({"time_embed.0.weight", E * D});
    r.push_back({"time_embed.0.bias", E});
    r.push_back({"time_embed.2.weight", E * E});
    r.push_back({"time_embed.2.bias", E});
    auto styl = [&](const std::string& p) {
        r.push_back({p + ".emb_layers.1.weight", 2 * D * E});
        r.push_back({p + ".emb_layers.1.bias", 2 * D});
        r.push_back({p + ".norm.weight", D});
        r.push_back({p + ".norm.bias", D});
        r.push_back({p + ".out_layers.2.weight", D * D});
        r.push_back({p + ".out_layers.2.bias", D});
    };
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = "temporal_decoder_blocks." + std::to_string(i);
        r.push_back({p + ".sa_block.norm.weight", D});
        r.push_back({p + ".sa_block.norm.bias", D});
        for (const char* n : {"query", "key", "value"}) {
            r.push_back({p + ".sa_block." + n + ".weight", D * D});
            r.push_back({p + ".sa_block." + n + ".bias", D});
        }
        styl(p + ".sa_block.proj_out");
        r.push_back({p + ".ca_block.norm.weight", D});
        r.push_back({p + ".ca_block.norm.bias", D});
        r.push_back({p + ".ca_block.text_norm.weight", L});
        r.push_back({p + ".ca_block.text_norm.bias", L});
        r.push_back({p + ".ca_block.query.weight", D * D});
        r.push_back({p + ".ca_block.query.bias", D});
        for (const char* n : {"key", "value"}) {
            r.push_back({p + ".ca_block." + n + ".weight", D * L});
            r.push_back({p + ".ca_block." + n + ".bias", D});
        }
        styl(p + ".ca_block.proj_out");
        r.push_back({p + ".ffn.linear1.weight", F * D});
        r.push_back({p + ".ffn.linear1.bias", F});
        r.push_back({p + ".ffn.linear2.weight", D * F});
        r.push_back({p + ".ffn.linear2.bias", D});
        styl(p + ".ffn.proj_out");
    }
    r.push_back({"out.weight", P * D});
    r.push_back({"out.bias", P});
    return r;
}

// MusicEncoder / proj entries are optional as a group: a sampler fed x_proj/x_out from elsewhere never needs them.
// Entries of the group the kernels do not consume (num_batches_tracked counters) are accepted and dropped.
bool music_param(const std::string& n) {
    return n.rfind("music_encoder.", 0) == 0 || n == "proj.weight" || n == "proj.bias";
}

// ---- the model image: everything the denoiser's kernels read, prepared on the host (no HIP call from here to upload_model) ----
// a pointer field of the model record and the same field of its split twin
template <class T>
struct Dst {
    const T **model, **split;
};

// What pack_model produces: the arena, and the two model records with their pointers still to be resolved (arena.resolve).
// `split` is the same model with the layer stage images in their split form where those are kept (dc_sampler::h_model_split).
struct ModelImage {
    Arena arena;
    DcModel model{}, split{};
    int NT = 0;                          // FiLM feature tiles = 3 * L * 8
    size_t freqs, w0t, b0, w2t, b2;      // arena offsets of the time-embedding operands (dc_launch_temb_table)
    ModelImage() = default;
    ModelImage(const ModelImage&) = delete;      // (the arena's fix-ups point into this object)
    template <class T>
    Dst<T> top(const T* DcModel::*f) { return {&(model.*f), &(split.*f)}; }
    template <class T>
    Dst<T> layer(int i, const T* DcLayer::*f) { return {&(model.layer[i].*f), &(split.layer[i].*f)}; }
    template <class T>
    Dst<T> l16(int i, const T* DcLayer16::*f) { return {&(model.l16[i].*f), &(split.l16[i].*f)}; }
};

// W' = W diag(g), c' = c + W b  (LayerNorm affine folded into the projection that consumes it)
// `scale` additionally multiplies the whole projection: log2(e) for the query / key projections, whose
// outputs only ever feed exp() (softmax), so the kernels can use the native exp2.
void fold_ln(const float* w, const float* c, const float* g, const float* b, int n_out, int k, std::vector<float>& wf,
             std::vector<float>& cf, double scale = 1.0) {
    wf.resize((size_t)n_out * k);
    cf.resize(n_out);
    for (int o = 0; o < n_out; ++o) {
        double acc = c[o];
        for (int i = 0; i < k; ++i) {
            wf[(size_t)o * k + i] = (float)((double)w[(size_t)o * k + i] * g[i] * scale);
            acc += (double)w[(size_t)o * k + i] * b[i];
        }
        cf[o] = (float)(acc * scale);
    }
}

// `linear` with the mean over its 512 outputs taken off (the LayerNorm in front of the cross-attention K / V projections sees
// linear(x) - mean = Wc x + bc), and that LayerNorm's variance as a quadratic form of the 64 inputs (DcModel::lin_gram).
// The inputs are shifted first: with u the least-squares solution of Wc u = bc, rounded to fp32, and r = bc - Wc u,
//   Wc x + bc = Wc (x + u) + r      exactly, for any u,
// and r is orthogonal to Wc's columns but for u's rounding.  The part of bc that lies in the column space of Wc - the part an x near
// -u cancels against, term by term, in every sum over the 64 features - is taken off in ONE fp32 addition per feature, exact where
// it cancels most (x_i within a factor 2 of -u_i); the sums then run over x + u and their constants come from r: d = W' r,
// gv = Wc^T r / 512 ~ 0, c = |r|^2 / 512, so that var = (x + u)^T Gc (x + u) + c is a sum of two non-negative terms.
struct LinearStats {
    std::vector<double> wc, bc;      // [512][64], [512] r = bc - Wc shift
    std::vector<float> gram;         // [64][64] Gc, gv[64], c, (3 unused), shift[64]: DC_GRAM_FLOATS
};
LinearStats centre_linear(const float* w /*[512][64]*/, const float* b) {
    LinearStats s{std::vector<double>((size_t)512 * 64), std::vector<double>(512), std::vector<float>(DC_GRAM_FLOATS, 0.f)};
    double bm = 0.0;
    for (int k = 0; k < 512; ++k) bm += b[k];
    bm /= 512.0;
    for (int k = 0; k < 512; ++k) s.bc[k] = (double)b[k] - bm;
    for (int i = 0; i < 64; ++i) {
        double wm = 0.0;
        for (int k = 0; k < 512; ++k) wm += w[(size_t)k * 64 + i];
        wm /= 512.0;
        for (int k = 0; k < 512; ++k) s.wc[(size_t)k * 64 + i] = (double)w[(size_t)k * 64 + i] - wm;
    }
    std::vector<double> n((size_t)64 * 64), rhs(64);      // normal equations Wc^T Wc u = Wc^T bc
    for (int i = 0; i < 64; ++i) {
        for (int j = 0; j < 64; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 512; ++k) acc += s.wc[(size_t)k * 64 + i] * s.wc[(size_t)k * 64 + j];
            n[i * 64 + j] = acc;
            s.gram[i * 64 + j] = (float)(acc / 512.0);
        }
        double acc = 0.0;
        for (int k = 0; k < 512; ++k) acc += s.wc[(size_t)k * 64 + i] * s.bc[k];
        rhs[i] = acc;
    }
    // Cholesky; a `linear.weight` without full column rank (to 1e-10 of its largest diagonal entry) keeps shift = 0, the unshifted form
    double dmax = 0.0;
    for (int i = 0; i < 64; ++i) dmax = std::max(dmax, n[i * 64 + i]);
    bool full_rank = dmax > 0.0;
    for (int j = 0; j < 64 && full_rank; ++j) {
        double d = n[j * 64 + j];
        for (int k = 0; k < j; ++k) d -= n[j * 64 + k] * n[j * 64 + k];
        if (!(d > 1e-10 * dmax)) {
            full_rank = false;
            break;
        }
        n[j * 64 + j] = std::sqrt(d);
        for (int i = j + 1; i < 64; ++i) {
            double v = n[i * 64 + j];
            for (int k = 0; k < j; ++k) v -= n[i * 64 + k] * n[j * 64 + k];
            n[i * 64 + j] = v / n[j * 64 + j];
        }
    }
    float* shift = s.gram.data() + DC_GRAM_SHIFT;
    if (full_rank) {
        for (int i = 0; i < 64; ++i) {                    // L z = rhs
            double v = rhs[i];
            for (int k = 0; k < i; ++k) v -= n[i * 64 + k] * rhs[k];
            rhs[i] = v / n[i * 64 + i];
        }
        for (int i = 63; i >= 0; --i) {                   // L^T u = z
            double v = rhs[i];
            for (int k = i + 1; k < 64; ++k) v -= n[k * 64 + i] * rhs[k];
            rhs[i] = v / n[i * 64 + i];
            shift[i] = (float)rhs[i];
        }
        for (int k = 0; k < 512; ++k)                     // r, from the shift as the device adds it
            for (int i = 0; i < 64; ++i) s.bc[k] -= s.wc[(size_t)k * 64 + i] * (double)shift[i];
    }
    for (int i = 0; i < 64; ++i) {
        double acc = 0.0;
        for (int k = 0; k < 512; ++k) acc += s.wc[(size_t)k * 64 + i] * s.bc[k];
        s.gram[64 * 64 + i] = (float)(acc / 512.0);
    }
    double cc = 0.0;
    for (int k = 0; k < 512; ++k) cc += s.bc[k] * s.bc[k];
    s.gram[64 * 64 + 64] = (float)(cc / 512.0);
    return s;
}

constexpr double LOG2E = 1.4426950408889634;

// The steps of pack_model and what they share.  Every add_* appends to the arena - the order of the calls IS the arena layout -
// and points the named field of both model records at the entry.
struct ModelPacker {
    const dc_config& c;
    const Formats& fmt;
    const DcParams& params;
    ModelImage& I;
    const bool sf16 = fmt.small_fmt == 1, ssp = fmt.split_small;
    const bool want_twins = (c.precision == DC_PREC_FP16 || c.precision == DC_PREC_BF16) && !ssp;
    // 16-token layer kernel (small batches; non-split formats, linear attention): up to two matrices + constants per stage image
    const bool want16 = !ssp && !c.no_eff;
    // softmax inputs: the linear-attention kernels use exp2 on log2(e)-scaled queries/keys; the full-attention
    // (no_eff) kernels keep keys unscaled and fold log2(e) / sqrt(head_dim) into the queries (scores arrive as exp2 exponents)
    const double QS = c.no_eff ? 0.25 * LOG2E : LOG2E, KS = c.no_eff ? 1.0 : LOG2E;
    // the FiLM stack, filled layer by layer (film_rows)
    std::vector<float> film_w = std::vector<float>((size_t)I.NT * 32 * DC_E), film_b = std::vector<float>((size_t)I.NT * 32), film_b_g1 = film_b;

    const float* P(const std::string& n) const { return params.find(n)->second.data(); }
    template <class T>
    void put(Dst<T> dst, size_t off) {
        I.arena.point(dst.model, off);
        I.arena.point(dst.split, off);
    }
    void add_vec(Dst<float> dst, const float* v, size_t n) { put(dst, I.arena.add(v, n * 4)); }
    void add_vec(Dst<float> dst, const std::vector<float>& v) { put(dst, I.arena.add(v)); }
    // natural-k fragments, [hi][lo]
    void add_natural(Dst<bf16x8> dst, const float* w, int n_out, int k_in, bool f16) {
        const size_t ne = packed_elems(n_out, k_in);
        std::vector<uint16_t> buf(2 * ne);
        pack_weight(w, n_out, k_in, false, buf.data(), buf.data() + ne, f16);
        put(dst, I.arena.add(buf));
    }
    // [hi frags][lo frags if `with_lo`][1 KiB of fp32 constants if `consts`]
    static std::vector<uint8_t> blob_of(const std::vector<uint16_t>& hi, const std::vector<uint16_t>& lo, bool with_lo, const float* consts,
                                        size_t n_consts) {
        const size_t half = hi.size() * 2;
        std::vector<uint8_t> blob(half * (with_lo ? 2 : 1) + (consts ? 1024 : 0), 0);
        memcpy(blob.data(), hi.data(), half);
        if (with_lo) memcpy(blob.data() + half, lo.data(), half);
        if (consts) memcpy(blob.data() + half * (with_lo ? 2 : 1), consts, n_consts * 4);
        return blob;
    }
    // stage image of k_layer (dc_common.h), chained k order; a plain one is followed by its split twin where the model keeps twins
    void add_image(Dst<bf16x8> dst, const float* w, int n_out, int k_in, bool with_lo, const float* consts, size_t n_consts) {
        const size_t ne = packed_elems(n_out, k_in);
        std::vector<uint16_t> hi(ne), lo(ne);
        pack_weight(w, n_out, k_in, true, hi.data(), lo.data(), sf16);
        const size_t off = I.arena.add(blob_of(hi, lo, with_lo, consts, n_consts));
        I.arena.point(dst.model, off);
        I.arena.point(dst.split, want_twins && !with_lo ? I.arena.add(blob_of(hi, lo, true, consts, n_consts)) : off);
    }
    // stage image of the 16-token layer kernel: one or two matrices, then the constants
    void add_image16(Dst<bf16x8> dst, const float* wa, int na_out, int ka, const float* wb, int nb_out, int kb, bool with_lo,
                     const std::vector<float>& consts) {
        if (!want16) return;
        const size_t ea = packed_elems16(na_out, ka), eb = wb ? packed_elems16(nb_out, kb) : 0;
        std::vector<uint16_t> hi(ea + eb), lo(ea + eb);
        pack_weight16(wa, na_out, ka, hi.data(), lo.data(), sf16);
        if (wb) pack_weight16(wb, nb_out, kb, hi.data() + ea, lo.data() + ea, sf16);
        put(dst, I.arena.add(blob_of(hi, lo, with_lo, consts.data(), consts.size())));
    }

    // a 128 x 128 projection with the LayerNorm `norm` in front of it folded in; its bias as an FT vector (queries) or plain
    void attn_proj(int i, const bf16x8* DcLayer::*img, const bf16x8* DcLayer16::*img16, const std::string& proj, const std::string& norm,
                   double scale, bool ft_bias) {
        std::vector<float> wf, cf;
        fold_ln(P(proj + ".weight"), P(proj + ".bias"), P(norm + ".weight"), P(norm + ".bias"), DC_D, DC_D, wf, cf, scale);
        const std::vector<float> cst = ft_bias ? ftvec(cf.data(), DC_D, 4) : cf;
        add_image(I.layer(i, img), wf.data(), DC_D, DC_D, ssp, cst.data(), cst.size());
        add_image16(I.l16(i, img16), wf.data(), DC_D, DC_D, nullptr, 0, 0, false, cf);
    }
    // a StylizationBlock's output projection
    void styl_out(int i, const bf16x8* DcLayer::*img, const bf16x8* DcLayer16::*img16, const std::string& p) {
        const float* b = P(p + ".out_layers.2.bias");
        const std::vector<float> bo = ftvec(b, DC_D, 4);
        // the kernels hand over log2(e) * SiLU(.) (silu_l2_pair in dc_kernels.hip): ln 2 goes into the weights
        const float* w = P(p + ".out_layers.2.weight");
        std::vector<float> ws((size_t)DC_D * DC_D);
        for (size_t k = 0; k < ws.size(); ++k) ws[k] = (float)((double)w[k] * 0.6931471805599453);
        add_image(I.layer(i, img), ws.data(), DC_D, DC_D, ssp, bo.data(), bo.size());
        add_image16(I.l16(i, img16), ws.data(), DC_D, DC_D, nullptr, 0, 0, false, std::vector<float>(b, b + DC_D));
    }
    // Cross-attention key (kv = 0) or value (1) projection of the conditioning pre-pass, text_norm's affine folded in
    // (transformer.py:149,153), always split-bf16 - and the same projection composed with `linear` (transformer.py:479-480;
    // 64 -> 512, shared by all layers): with y = W x + b, n-hat = (y - mean(y)) rstd = rstd (Wc x + bc), so
    //   W' n-hat + b' = rstd (A x + d) + b',   A = W' Wc [128][64],  d = W' bc;   on the shifted features (centre_linear):
    //                 = rstd (A (x + u) + d) + b' with d = W' r
    // - an eighth of the pre-pass GEMM's products (k_cond_ca_partials64), and no [tokens][512] image in between.
    void cross_kv(int i, int kv, const std::string& ca, const LinearStats& lin) {
        const std::string nm = ca + (kv ? ".value" : ".key");
        std::vector<float> wf, bf;
        fold_ln(P(nm + ".weight"), P(nm + ".bias"), P(ca + ".text_norm.weight"), P(ca + ".text_norm.bias"), DC_D, DC_E, wf, bf,
                kv ? 1.0 : KS);                        // keys feed exp2 in the partial records
        add_natural(I.layer(i, kv ? &DcLayer::ca_wv : &DcLayer::ca_wk), wf.data(), DC_D, DC_E, false);
        add_vec(I.layer(i, kv ? &DcLayer::ca_bv : &DcLayer::ca_bk), bf);
        std::vector<float> af((size_t)DC_D * 64), df(DC_D);
        for (int o = 0; o < DC_D; ++o) {
            double dacc = 0.0;
            for (int k = 0; k < DC_E; ++k) dacc += (double)wf[(size_t)o * DC_E + k] * lin.bc[k];
            df[o] = (float)dacc;
            for (int x = 0; x < 64; ++x) {
                double acc = 0.0;
                for (int k = 0; k < DC_E; ++k) acc += (double)wf[(size_t)o * DC_E + k] * lin.wc[(size_t)k * 64 + x];
                af[(size_t)o * 64 + x] = (float)acc;
            }
        }
        add_natural(I.layer(i, kv ? &DcLayer::ca_av : &DcLayer::ca_ak), af.data(), DC_D, 64, false);
        add_vec(I.layer(i, kv ? &DcLayer::ca_dv : &DcLayer::ca_dk), df);
    }
    void ffn(int i, const std::string& p) {
        const float *w1 = P(p + ".linear1.weight"), *b1 = P(p + ".linear1.bias"), *w2 = P(p + ".linear2.weight"), *b2 = P(p + ".linear2.bias");
        add_image(I.layer(i, &DcLayer::img_ffn_w1), w1, DC_F, DC_D, ssp, nullptr, 0);
        std::vector<float> cst = ftvec(b1, DC_F, 2);       // 64 floats, then b2
        const std::vector<float> c2 = ftvec(b2, DC_D, 4);
        cst.insert(cst.end(), c2.begin(), c2.end());
        add_image(I.layer(i, &DcLayer::img_ffn_w2), w2, DC_D, DC_F, ssp, cst.data(), cst.size());
        std::vector<float> plain(b1, b1 + DC_F);
        plain.insert(plain.end(), b2, b2 + DC_D);
        add_image16(I.l16(i, &DcLayer16::ffn_w), w1, DC_F, DC_D, w2, DC_D, DC_F, false, plain);
    }
    // Rows of the FiLM stack for StylizationBlock `blk` (0 .. 3L-1).  All blocks are stacked along the output axis -> one
    // [3L*256][512] GEMM operand; inside a block the 32-row tiles are interleaved (tile 2t = G' - 1 of features 32t.., tile
    // 2t+1 = H' of the same features) so one wave holds matching pairs.
    // y = LN(h) (1 + scale) + shift with LN = g n + beta (transformer.py:74-78) becomes  y = n G' + H',
    //   G' = g (1 + scale), H' = beta (1 + scale) + shift, both affine in S = SiLU(emb): fold g / beta into the rows.
    // The H' tiles additionally carry log2(e): the kernels evaluate SiLU on log2(e)-scaled arguments (silu_l2_pair)
    void film_rows(int blk, const std::string& p) {
        const size_t row0 = (size_t)blk * 256;
        const float* w = P(p + ".emb_layers.1.weight");   // rows 0..127 scale, 128..255 shift
        const float* bb = P(p + ".emb_layers.1.bias");
        const float* ng = P(p + ".norm.weight");
        const float* nb = P(p + ".norm.bias");
        for (int t = 0; t < 4; ++t)
            for (int f = 0; f < 32; ++f) {
                const int o = 32 * t + f;
                const size_t rg = row0 + (size_t)(2 * t) * 32 + f, rh = rg + 32;
                const float* ws = w + (size_t)o * DC_E;
                const float* wh = w + (size_t)(128 + o) * DC_E;
                float* dg = &film_w[rg * DC_E];
                float* dh = &film_w[rh * DC_E];
                for (int k = 0; k < DC_E; ++k) {
                    dg[k] = (float)((double)ng[o] * ws[k]);
                    dh[k] = (float)(((double)nb[o] * ws[k] + wh[k]) * LOG2E);
                }
                film_b[rg] = (float)((double)ng[o] * (1.0 + bb[o]) - 1.0);
                film_b[rh] = (float)(((double)nb[o] * (1.0 + bb[o]) + bb[128 + o]) * LOG2E);
                film_b_g1[rg] = (float)((double)ng[o] * (1.0 + bb[o]));          // (G' itself: film_stack)
                film_b_g1[rh] = film_b[rh];
            }
    }
    void decoder_layer(int i, const LinearStats& lin) {
        const std::string p = "temporal_decoder_blocks." + std::to_string(i);
        const std::string sa = p + ".sa_block", ca = p + ".ca_block";
        attn_proj(i, &DcLayer::img_sa_q, &DcLayer16::sa_q, sa + ".query", sa + ".norm", QS, true);
        attn_proj(i, &DcLayer::img_sa_k, &DcLayer16::sa_k, sa + ".key", sa + ".norm", KS, false);
        attn_proj(i, &DcLayer::img_sa_v, &DcLayer16::sa_v, sa + ".value", sa + ".norm", 1.0, false);
        styl_out(i, &DcLayer::img_sa_o, &DcLayer16::sa_o, sa + ".proj_out");
        attn_proj(i, &DcLayer::img_ca_q, &DcLayer16::ca_q, ca + ".query", ca + ".norm", QS, true);
        for (int kv = 0; kv < 2; ++kv) cross_kv(i, kv, ca, lin);
        styl_out(i, &DcLayer::img_ca_o, &DcLayer16::ca_o, ca + ".proj_out");
        ffn(i, p + ".ffn");
        styl_out(i, &DcLayer::img_ffn_o, &DcLayer16::ffn_o, p + ".ffn.proj_out");
        film_rows(3 * i + 0, sa + ".proj_out");
        film_rows(3 * i + 1, ca + ".proj_out");
        film_rows(3 * i + 2, p + ".ffn.proj_out");
    }
    void film_stack() {
        const int NT = I.NT;
        const bool f16 = fmt.film_fmt == 1;
        add_natural(I.top(&DcModel::film_w), film_w.data(), NT * 32, DC_E, f16);
        add_vec(I.top(&DcModel::film_b), ftvec(film_b.data(), NT * 32, NT));
        // ... and with the scale tiles holding G' itself: the plain-operand layer kernels then form n-hat G' + H' in ONE mixed-precision FMA
        // instead of two (-192 vector instructions per wave and layer).  fp16 keeps 11 bits of a number near 1 there instead of 11 bits of
        // its small part - affordable where the loop's last evaluations run on split operands and G' - 1 tiles (precise tail, dc_ddim.h)
        add_vec(I.top(&DcModel::film_b_g1), ftvec(film_b_g1.data(), NT * 32, NT));
        // 16x16x32 operand order (dc_common.h)
        put(I.top(&DcModel::film_w16), I.arena.add(pack_film16(film_w, NT, DC_E, f16)));
        add_vec(I.top(&DcModel::film_b16), permute_film_bias16(film_b, NT));
        // bf16 precision: the evaluations of the precise tail run the "mixed" form - split-bf16 128-wide GEMMs AND an f16 FiLM GEMM
        // (8 mantissa bits on the K = 512 operands were the tail's floor: 3.6 - 4.1e-4 with every evaluation split)
        if (want_twins && c.precision == DC_PREC_BF16) put(I.top(&DcModel::film_w16_tail), I.arena.add(pack_film16(film_w, NT, DC_E, true)));
        add_vec(I.top(&DcModel::film_b16_g1), permute_film_bias16(film_b_g1, NT));
    }
    void pose_projections() {   // the two pose projections always run split: [hi][lo][bias]
        const int P_ = c.input_feats;
        const std::vector<float> jb = ftvec(P("joint_embed.bias"), DC_D, 4);
        add_image(I.top(&DcModel::img_je), P("joint_embed.weight"), DC_D, P_, true, jb.data(), jb.size());
        const std::vector<float> ob = ftvec(P("out.bias"), P_, 1);
        add_image(I.top(&DcModel::img_out), P("out.weight"), P_, DC_D, true, ob.data(), ob.size());
        std::vector<float> ob16(32, 0.f);
        for (int k = 0; k < P_; ++k) ob16[k] = P("out.bias")[k];
        add_image16(I.top(&DcModel::out16), P("out.weight"), P_, DC_D, nullptr, 0, 0, true, ob16);
    }
    void conditioning_front(const LinearStats& lin) {
        const float* w = P("linear.weight");   // [512][64] -> transposed [64][512]
        std::vector<float> wt((size_t)64 * 512);
        for (int k = 0; k < 512; ++k)
            for (int x = 0; x < 64; ++x) wt[(size_t)x * 512 + k] = w[(size_t)k * 64 + x];
        add_vec(I.top(&DcModel::lin_wt), wt);
        add_vec(I.top(&DcModel::lin_b), P("linear.bias"), 512);
        add_vec(I.top(&DcModel::lin_gram), lin.gram);
        add_natural(I.top(&DcModel::lin_pack), w, 512, 64, false);
    }
    // timestep table storage (filled by dc_launch_temb_table after the upload) + the MLP's operands, transposed for coalesced reads
    void time_embedding() {
        add_vec(I.top(&DcModel::temb), std::vector<float>((size_t)c.max_timesteps * 512, 0.f));
        std::vector<float> fr(64);
        // transformer.py:18-20 in fp32: the fp32 argument, and the correctly rounded fp32 exp of it (through double, so that it does not
        // depend on the C library's expf; torch's own exp is one ulp off at k = 22 on some CPUs)
        for (int k = 0; k < 64; ++k) fr[k] = (float)std::exp((double)((float)(-std::log(10000.0)) * (float)k / 64.f));
        std::vector<float> w0t((size_t)128 * 512), w2t((size_t)512 * 512);
        const float* w0 = P("time_embed.0.weight");
        const float* w2 = P("time_embed.2.weight");
        for (int o = 0; o < 512; ++o) {
            for (int x = 0; x < 128; ++x) w0t[(size_t)x * 512 + o] = w0[(size_t)o * 128 + x];
            for (int x = 0; x < 512; ++x) w2t[(size_t)x * 512 + o] = w2[(size_t)o * 512 + x];
        }
        I.freqs = I.arena.add(fr);
        I.w0t = I.arena.add(w0t);
        I.b0 = I.arena.add(P("time_embed.0.bias"), 512 * 4);
        I.w2t = I.arena.add(w2t);
        I.b2 = I.arena.add(P("time_embed.2.bias"), 512 * 4);
    }
};

// Folds and packs the parameters (all of required_params present) into `I`.  Reads nothing but its arguments; runs on any host.
void pack_model(const dc_config& c, const Formats& fmt, const DcParams& params, ModelImage& I) {
    const int L = c.num_layers;
    I.NT = 3 * L * DC_FILM_TILES_PER_BLOCK;
    I.model.num_layers = L;
    I.model.input_feats = c.input_feats;
    I.model.num_frames = c.num_frames;
    I.model.max_timesteps = c.max_timesteps;
    I.split = I.model;
    ModelPacker k{c, fmt, params, I};
    const LinearStats lin = centre_linear(k.P("linear.weight"), k.P("linear.bias"));
    for (int i = 0; i < L; ++i) k.decoder_layer(i, lin);
    k.film_stack();
    k.pose_projections();
    k.add_vec(I.top(&DcModel::seq_emb), k.P("sequence_embedding"), (size_t)c.num_frames * DC_D);
    k.conditioning_front(lin);
    k.time_embedding();
}

// The impure half: the image goes to the device (host-only samplers: to malloc'ed memory), the pointers of both model records
// are resolved against its address, and the time-embedding table is computed in place.
int upload_model(dc_sampler* s, ModelImage& I) {
    const std::vector<uint8_t>& host = I.arena.host;
    s->NT = I.NT;
    s->arena_bytes = host.size();
    if (s->host_only) {
        free(s->d_arena);
        s->d_arena = (uint8_t*)malloc(host.size());
        memcpy(s->d_arena, host.data(), host.size());
    } else {
        if (s->d_arena) hipFree(s->d_arena);
        HIP_TRY(hipMalloc((void**)&s->d_arena, host.size()));
        HIP_TRY(hipMemcpy(s->d_arena, host.data(), host.size(), hipMemcpyHostToDevice));
    }
    I.arena.resolve(s->d_arena);
    s->h_model = I.model;
    s->h_model_split = I.split;
    if (s->host_only) return DC_OK;
    if (!s->d_model) HIP_TRY(hipMalloc((void**)&s->d_model, sizeof(DcModel)));
    HIP_TRY(hipMemcpy(s->d_model, &s->h_model, sizeof(DcModel), hipMemcpyHostToDevice));
    if (!s->d_model_split) HIP_TRY(hipMalloc((void**)&s->d_model_split, sizeof(DcModel)));
    HIP_TRY(hipMemcpy(s->d_model_split, &s->h_model_split, sizeof(DcModel), hipMemcpyHostToDevice));
    const auto op = [&](size_t off) { return (const float*)(s->d_arena + off); };
    HIP_TRY(dc_launch_temb_table(s->stream, op(I.freqs), op(I.w0t), op(I.b0), op(I.w2t), op(I.b2), (float*)s->h_model.temb, s->cfg.max_timesteps));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return DC_OK;
}

// what the launch rule (dc_form.h) reads of a sampler
Settings settings_of(const dc_sampler* s) {
    Settings r;
    r.precision = s->cfg.precision, r.fmt = *s, r.no_eff = s->cfg.no_eff != 0, r.clip_aligned = s->clip_aligned, r.l16_own = s->l16_own;
    r.num_layers = s->cfg.num_layers, r.split_model = s->d_model_split != nullptr, r.film_w16 = s->h_model.film_w16 != nullptr;
    r.film_w16_tail = s->h_model.film_w16_tail != nullptr, r.l16_max_units = dc_layer16_max_units(), r.idle_wave_path = s->idle_wave_path;
    return r;
}
int clip_stride(const dc_sampler* s, int B, int Tx) { return clip_stride(settings_of(s), Switches::read(), B, Tx, s->num_cu); }
int ensure_workspace(dc_sampler* s, int B, int Tx) {
    const int T = clip_stride(s, B, Tx);
    const int M = B * T, G = cdiv(M, 32), L = s->cfg.num_layers, P = s->cfg.input_feats;
    if ((size_t)G > s->cap_G) {
        drop_graph(s);
        const size_t g = (size_t)G;
        s->cap_G = 0;
        int rc;
        if ((rc = dev_alloc(s, s->d_pp, g * 32 * 64 * 8 * 4))) return rc;
        if ((rc = dev_alloc(s, s->d_s_hi, g * 32 * 64 * 16))) return rc;
        if ((rc = dev_alloc(s, s->d_s_lo, g * 32 * 64 * 16))) return rc;
        if ((rc = dev_alloc(s, s->d_E, g * s->NT * 64 * 32))) return rc;
        if ((rc = dev_alloc(s, s->d_h, g * 4 * 64 * 64))) return rc;
        HIP_TRY(hipMemset(s->d_h, 0, g * 4 * 64 * 64));     // rows past M are read (never written) by the full-attention front half
        s->cap_rec_floats = rec_capacity(g);      // unit records (dc_form.h)
        if ((rc = dev_alloc(s, s->d_recs, s->cap_rec_floats * 4))) return rc;
        if ((rc = dev_alloc(s, s->d_nh_hi, g * 32 * 64 * 16))) return rc;
        if ((rc = dev_alloc(s, s->d_nh_lo, g * 32 * 64 * 16))) return rc;
        if (!s->cfg.no_eff && (rc = dev_alloc(s, s->d_recs_ca, (size_t)L * g * 2 * DC_REC_FLOATS * 4))) return rc;
        s->cap_G = g;
    }
    if (s->cfg.no_eff) {     // key-tile arrays: [B][KT] tiles of 16 KiB; two for self-attention (layer parity), L for cross-attention
        const int KT = (T + 31) / 32 + 1;
        const size_t need = (size_t)B * KT;
        if (need > s->cap_kv) {
            drop_graph(s);
            s->cap_kv = 0;
            int rc;
            for (int i = 0; i < 2; ++i)
                if ((rc = dev_alloc(s, s->d_kv_sa[i], need * 16384))) return rc;
            if ((rc = dev_alloc(s, s->d_kv_ca, (size_t)L * need * 16384))) return rc;
            s->cap_kv = need;
        }
        s->KT = KT;
    }
    if ((size_t)B > s->cap_B) {
        drop_graph(s);
        s->cap_B = 0;
        int rc;
        if ((rc = dev_alloc(s, s->d_length, (size_t)B * 4))) return rc;
        if ((rc = dev_alloc(s, s->d_t_clip, (size_t)B * 4))) return rc;
        if ((rc = dev_alloc(s, s->d_a_sa, (size_t)B * 16 * 1024))) return rc;
        if ((rc = dev_alloc(s, s->d_a_ca, (size_t)L * B * 16 * 1024))) return rc;
        if ((rc = dev_alloc(s, s->d_a_ca16, (size_t)L * B * 8 * 1024))) return rc;
        if ((rc = dev_alloc(s, s->d_gran, (size_t)B * 1024 * 8))) return rc;
        HIP_TRY(hipMemset(s->d_gran, 0, (size_t)B * 1024 * 8));        // tag 0 is never a launch's
        s->cap_B = (size_t)B;
    }
    if ((size_t)M * P > s->cap_MP) {
        drop_graph(s);
        s->cap_MP = 0;
        int rc;
        if ((rc = dev_alloc(s, s->d_x, (size_t)M * P * 4))) return rc;
        s->cap_MP = (size_t)M * P;
    }
    if (!s->d_iter) {
        int rc;
        if ((rc = dev_alloc(s, s->d_stamps, (8 * 32 + 8 + 1024 + 1024 + 256 + 8 + 512) * 8))) return rc;
        if ((rc = dev_alloc(s, s->d_film_rate, 2 * 1024 * sizeof(float)))) return rc;
        HIP_TRY(hipMemset(s->d_film_rate, 0, 2 * 1024 * sizeof(float)));      // 0 = not measured yet: equal shares
        if ((rc = dev_alloc(s, s->d_status, 16))) return rc;
        HIP_TRY(hipMemset(s->d_status, 0, 16));
        if ((rc = dev_alloc(s, s->d_zslot, 32))) return rc;
        HIP_TRY(hipMemset(s->d_zslot, 0, 32));
        if ((rc = dev_alloc(s, s->d_kslot, 32))) return rc;
        HIP_TRY(hipMemset(s->d_kslot, 0, 32));
        if ((rc = dev_alloc(s, s->d_iter, 16))) return rc;
        if ((rc = dev_alloc(s, s->d_snap_cur, 16))) return rc;
        if ((rc = dev_alloc(s, s->d_coef_cur, DC_COEF * 4))) return rc;
    }
    if ((s->B != B || s->T != T) && s->d_gran)       // another geometry: no granule of the shared combine may carry a tag a launch could expect
        HIP_TRY(hipMemsetAsync(s->d_gran, 0, s->cap_B * 1024 * 8, s->stream));
    s->B = B;
    s->T = T;
    s->Tx = Tx;
    s->M = M;
    s->G = G;
    return DC_OK;
}

int ensure_steps(dc_sampler* s, int S) {
    if ((size_t)S > s->cap_steps) {
        drop_graph(s);
        s->cap_steps = 0;
        s->tables_S = 0;
        int rc;
        if ((rc = dev_alloc(s, s->d_t_of_iter, (size_t)S * 4))) return rc;
        if ((rc = dev_alloc(s, s->d_snap_of_iter, (size_t)S * 4))) return rc;
        if ((rc = dev_alloc(s, s->d_coef_of_iter, (size_t)S * DC_COEF * 4))) return rc;
        s->cap_steps = (size_t)S;
    }
    return DC_OK;
}

#define LAUNCH(id, expr)                                              \
    do {                                                              \
        if (c.profile) {                                              \
            hipEvent_t a_, b_;                                        \
            HIP_TRY(hipEventCreate(&a_));                             \
            HIP_TRY(hipEventCreate(&b_));                             \
            HIP_TRY(hipEventRecord(a_, st));                          \
            HIP_TRY(expr);                                            \
            HIP_TRY(hipEventRecord(b_, st));                          \
            s->prof.ev.push_back(a_);                                 \
            s->prof.ev.push_back(b_);                                 \
            s->prof.ids.push_back(id);                                \
        } else {                                                      \
            HIP_TRY(expr);                                            \
        }                                                             \
    } while (0)

// One enqueue_step call: the options that decide its form (dc_form.h) and its tensors ...
struct Step : StepOpts {
    const float* x_src = nullptr;
    float* x_dst = nullptr;
};
// ... and what it tells its caller
struct StepDone {
    bool embedded_next = false;   // the step also did the next step's front work (DC_UPD_EMBED_NEXT): Step::embedded of that step
    bool folded = false;          // the step's kernels look their timestep up through *d_iter (no k_begin_step launch)
};

// The FiLM GEMM over the current geometry (pp: the fp32 emb image of the non-split formats, nullptr for the split ones)
DcFilmArgs film_args(const dc_sampler* s, const float* pp, const int* t_clip) {
    DcFilmArgs f{};
    f.W = s->h_model.film_w, f.bias_ft = s->h_model.film_b, f.s_hi = s->d_s_hi, f.s_lo = s->d_s_lo, f.E = s->d_E, f.G = s->G, f.NT = s->NT;
    f.nround = s->NT / 16, f.pp = pp, f.temb = s->h_model.temb, f.t_clip = t_clip, f.T = s->T, f.B = s->B;
    f.W16 = s->h_model.film_w16, f.bias16 = s->h_model.film_b16, f.status = s->d_status;
    return f;
}

// One denoiser evaluation (+ DDIM update when loop_mode) enqueued on st, in the form step_form (dc_form.h) decides: this function
// fills the launch arguments and launches.  `w`: the caller's Switches::read() of this API call.
int enqueue_step(dc_sampler* s, hipStream_t st, const Step& c, const Switches& w, StepDone* done = nullptr) {
    static const bool want_stamps = getenv("DC_STAMPS") != nullptr;       // (the FiLM GEMM's clock stamps land in stamp slots 28..31 of wave 7)
    const int B = s->B, T = s->T, M = s->M, G = s->G, Tx = s->Tx;
    const StepForm f = step_form(Geometry{B, T, Tx, G, s->num_cu, s->cap_rec_floats}, settings_of(s), w, c, want_stamps);
    const bool folded = f.folded;
    const int fs = f.fs, ff = f.ff, graph_step = c.graph_step;
    const bool ss = f.ss, sf = s->split_film;
    // k_layer16's tags: captured steps 16 * (graph step + *d_iter) + layer + 1, eager launches from a sequence of their own above them -
    // consecutive launches never share a tag (the sequence advances on every step that is not folded, whichever kernel runs)
    const unsigned l16_tag = folded ? 16u * (unsigned)graph_step : (0x40000000u | (16u * (s->l16_seq++ & 0x3ffffffu)));
    if (!f.error.empty()) return fail(DC_ERR_INVALID, "%s", f.error.c_str());
    if (done) done->embedded_next = f.embed_next, done->folded = folded;
    const DcModel* dmod = (c.split && !s->split_small) ? s->d_model_split : s->d_model;      // (the precise tail's split stage images)
    const int* iter_base = folded ? s->d_iter : nullptr;
    const int* t_src = folded ? s->d_t_of_iter + graph_step : s->d_t_clip;
    const float* coef_src = folded ? s->d_coef_of_iter + DC_COEF * (size_t)graph_step : s->d_coef_cur;
    const int* snap_src = folded ? s->d_snap_of_iter + graph_step : s->d_snap_cur;
    if (c.loop_mode && !folded)
        LAUNCH(K_BEGIN, dc_launch_begin_step(st, s->d_iter, s->d_t_of_iter, s->d_coef_of_iter, s->d_snap_of_iter,
                                             s->d_t_clip, s->d_coef_cur, s->d_snap_cur, B));
    if (c.loop_mode && (s->upd_flags & DC_UPD_ZSTEP))       // this iteration's draws (eta > 0, library-generated): consumed by the last layer's epilogue
        LAUNCH(K_NOISE, dc_launch_step_noise(st, s->d_zstep, s->user_elems(), 0, reinterpret_cast<const unsigned long long*>(s->d_zslot) + 1,
                                             iter_base, folded ? graph_step : 0,
                                             folded ? nullptr : s->d_snap_cur, 0));
    if (!f.fuse_silu)
        LAUNCH(K_SILU, dc_launch_silu_emb(st, ff, sf, s->d_pp, s->h_model.temb, s->d_t_clip, s->d_s_hi, s->d_s_lo, G, T, B));
    DcEmbedArgs ea{};
    if (f.fuse_embed) ea = DcEmbedArgs{dmod, c.x_src, s->d_h, s->d_recs, s->d_length, M, Tx, f.nwg, f.upc, ss ? 1 : 0, 0};
    if (f.fuse_extra) ea = DcEmbedArgs{s->d_model, c.x_src, s->d_h, s->d_recs, s->d_length, M, Tx, f.nwg, f.upc, 0, 1};
    DcFilmArgs fa = film_args(s, f.fuse_silu ? s->d_pp : nullptr, t_src);
    if (f.g1_tiles) fa.bias_ft = s->h_model.film_b_g1, fa.bias16 = s->h_model.film_b16_g1;
    if (f.film_tail) fa.W16 = s->h_model.film_w16_tail;
    s->last_film_groups = f.film_groups;
    fa.G = f.film_groups;       // (film_share: one take's groups, + one for every shadow group of a guided step; nothing shared: G)
    if (f.guided && f.film_period < f.film_wrap) {      // guided takes: one take's groups, then the null column
        if (!s->d_pp_share || (size_t)f.film_groups > s->cap_pp_share) return fail(DC_ERR_INVALID, "internal: no operand image for the shared takes of a guided step");
        fa.pp = s->d_pp_share;
    }
    s->pp_last = fa.pp;
    fa.clk = want_stamps ? s->d_stamps + 252 : nullptr;
    if (f.adapt) fa.rate_in = s->d_film_rate + 1024 * s->film_rate_parity, fa.rate_out = s->d_film_rate + 1024 * (s->film_rate_parity ^ 1);
    fa.iter_base = iter_base;
    fa.embed = (f.fuse_embed || f.fuse_extra) ? &ea : nullptr;
    // DC_DIAG_SKIP_FILM=1 (diagnostic, eager passes only, results invalid): the FiLM GEMM is launched once and never again - the layers then
    // read stale tiles and run without the GEMM's 300 us of power-limited matrix work between them (what the chip's clock management
    // does to the layer launches that follow a GEMM: tools/diag_clock_coupling.py)
    const bool diag_skip_film = getenv("DC_DIAG_SKIP_FILM") && !f.fuse_embed && !f.fuse_extra && s->diag_film_done;
    s->diag_film_done = true;
    if (!diag_skip_film) LAUNCH(K_FILM, dc_launch_film_gemm(st, ff, sf, fa));
    s->film_rate_parity ^= 1;
    const int nl_run = f.nl_run;
    DcLayerArgs la{};
    la.dm = dmod, la.hbuf = s->d_h, la.E = s->d_E, la.NT = s->NT, la.recs = s->d_recs, la.length = s->d_length, la.xin = c.x_src, la.xout = c.x_dst;
    la.out_mode = (c.loop_mode && !f.guided && !f.windows) ? 1 : 0, la.coef_cur = coef_src, la.snap_cur = snap_src, la.snaps = s->d_snaps, la.iter_base = iter_base;
    la.M = M, la.T = T, la.G = G, la.B = B, la.Tx = Tx, la.e_groups = f.film_groups, la.e_period = f.film_period, la.e_wrap = f.film_wrap, la.e_magic = film_magic(f.film_period, f.film_wrap);
    if (f.guided) la.xout = s->d_raw;      // the raw output of all 2 B clips; k_guided_update (below) combines the halves and updates x
    if (f.windows) la.xout = s->d_raw;     // ... of all windows; k_windows_update (below) blends them and updates x in piece space
    la.upd = DcUpdate{s->d_zslot, s->d_status, (c.loop_mode ? s->upd_flags : 0) | f.upd_flags, folded ? graph_step : -1, nullptr, s->d_kslot, s->d_x0_prev};
    DcLayerArgs la_stamps = la;      // (stage stamps of layer 3 in diagnostic builds: DcUpdate::stamps carries the buffer)
    la_stamps.upd.stamps = s->d_stamps;
    // behind the last layer of a windows or guided step, which stored the raw output: the kernel that combines it and updates x
    const auto post_update = [&]() -> int {
        if (f.windows)
            LAUNCH(K_WINDOWS, dc_launch_windows_update(st, s->d_raw, c.x_dst, s->d_xp, f.guided ? 2 : 1, s->user_B(), s->win_W, Tx, s->win_L, s->cfg.input_feats,
                                                       s->d_winslot, coef_src, snap_src, s->d_snaps, iter_base, s->d_wslot, la.upd));
        else if (f.guided)
            LAUNCH(K_GUIDE, dc_launch_guided_update(st, s->d_raw, c.x_dst, (size_t)s->user_B() * Tx * s->cfg.input_feats, coef_src, snap_src,
                                                    s->d_snaps, iter_base, s->d_wslot, la.upd));
        return DC_OK;
    };
    if (s->cfg.no_eff) {
        LAUNCH(K_EMBED, dc_launch_embed_front_full(st, fs, ss, dmod, c.x_src, s->d_h, s->d_kv_sa[0], M, T, B, s->KT));
        for (int l = 0; l < nl_run; ++l)        // (stage stamps: tools/stage_stamps_full.py + a -DDC_FULL_STAMPS build)
            LAUNCH(K_LAYER, dc_launch_layer_full(st, fs, ss, (want_stamps && l == 3) ? la_stamps : la, l, s->d_kv_sa[l & 1], s->d_kv_sa[(l + 1) & 1],
                                                 s->d_kv_ca, s->KT, (l == nl_run - 1) ? f.stop_stage : 0));
        return post_update();
    }
    const DcLayerForm lf{fs, ss, f.wgr, f.narrow, f.g1_tiles, f.upc, f.rec_stride, f.idle_path};
    if (f.fuse_embed || f.fuse_extra || c.embedded) {
        // (embedded by the FiLM launch, or by the previous step's last layer)
    } else if (c.dbg.first >= 0)
        LAUNCH(K_EMBED, dc_launch_front_from_h(st, fs, ss, dmod, s->d_h, s->d_recs, s->d_length, M, T, G, B, c.dbg.first));
    else
        LAUNCH(K_EMBED, dc_launch_embed_front(st, lf, dmod, c.x_src, s->d_h, s->d_recs, s->d_length, M, T, G, B,
                                              want_stamps ? s->d_stamps + 256 : nullptr, Tx));
    for (int l = c.dbg.first >= 0 ? c.dbg.first : 0; l < nl_run; ++l) {
        if (f.layer16) {
            static const bool stamps16 = getenv("DC_L16_STAMPS") != nullptr;        // (-DDC_L16_STAMPS builds: tools/stage_stamps16.py)
            LAUNCH(K_LAYER, dc_launch_layer16(st, fs, (stamps16 && l == 3) ? la_stamps : la, l, s->d_a_ca16, f.upc16, f.rec_stride,
                                              l == 0 ? f.upc_narrow : f.upc16, l == 0 ? (size_t)2 * DC_REC_FLOATS : (size_t)DC_REC_FLOATS,
                                              f.l16_shared ? s->d_gran : nullptr, l16_tag, f.g1_tiles));
            continue;
        }
        if (!f.wgr) LAUNCH(K_COMBINE, dc_launch_attn_combine(st, fs, s->d_recs, s->d_a_sa, T, G, B, 1, 32));      // (per-group records)
        LAUNCH(K_LAYER, dc_launch_layer(st, lf, la, l, s->d_a_sa, s->d_a_ca, (l == nl_run - 1) ? f.stop_stage : 0,
                                        ((l == 3 || l == 4) && want_stamps) ? s->d_stamps : nullptr));
    }
    return post_update();
}

int sync_in(dc_sampler* s, hipStream_t user) {
    HIP_TRY(hipEventRecord(s->ev_in, user));
    HIP_TRY(hipStreamWaitEvent(s->stream, s->ev_in, 0));
    return DC_OK;
}
int sync_out(dc_sampler* s, hipStream_t user) {
    HIP_TRY(hipEventRecord(s->ev_out, s->stream));
    HIP_TRY(hipStreamWaitEvent(user, s->ev_out, 0));
    return DC_OK;
}

// What the five public loop entry points pass: run_loop validates the caller's half of it, loop_common runs it
struct LoopCall {
    const float* d_noise = nullptr;
    float* d_out = nullptr;
    int n = 0;                                // iterations
    bool listed = false;                      // the entry point takes a timestep list (dc_sampler_solver_loop): h_timesteps is required
    const int32_t* h_timesteps = nullptr;     // the timestep the model sees at each iteration ([n], strictly decreasing); nullptr = n-1 .. 0
    const float* h_rows = nullptr;            // [n][DC_COEF] scalars of the update PER ITERATION (dc_common.h)
    int flags = 0;                            // the caller's DC_UPD_CLIP | DC_UPD_EPS
    const float* d_step_noise = nullptr;      // [n][B][Tx][P] or nullptr
    const int32_t* h_snap_iters = nullptr;
    int n_snap = 0;
    float* d_snaps = nullptr;
    bool profile = false;                     // events around every launch of an eager loop, summed per kernel into h_ms / h_count [n_kernels]
    float* h_ms = nullptr;
    int32_t* h_count = nullptr;
    int n_kernels = 0;
    void* stream = nullptr;
};

// loop_common, step 1: what the sampler's state refuses.  flags: DC_UPD_*, the caller's + NOISY / MULTISTEP; gains KNOWN
int loop_validate(dc_sampler* s, const LoopCall& c, int& flags) {
    const int S = c.n;
    const float* h_coef = c.h_rows;
    const bool profile = c.profile;
    if (!s || !s->finalized) return fail(DC_ERR_INVALID, "sampler not finalized");
    if (!s->cond_set) return fail(DC_ERR_INVALID, "dc_sampler_set_conditioning must be called first");
    if (S < 1 || S > s->cfg.max_timesteps) return fail(DC_ERR_INVALID, "num_steps %d outside [1, max_timesteps=%d]", S, s->cfg.max_timesteps);
    if (!c.d_noise || !c.d_out || !h_coef) return fail(DC_ERR_INVALID, "null pointer argument");
    // EPSILON model x full attention x eta = 0: outside the 1e-3 bound on some loops even with every GEMM on split operands (scores, weights
    // and values of the attention stay plain fp16, and a deterministic EPSILON chain keeps every evaluation's error in x_t): 2.3e-4 ... 1.26e-3
    // over 14 randomized loops of tools/fuzz_sampler.py (profiles/r06_fuzz_final.txt).  Refused, not returned; with eta > 0 the fresh noise
    // damps it (<= 2e-4 on the same tool), and linear attention reads <= 2.8e-4 at eta = 0.
    if ((flags & DC_UPD_EPS) && s->cfg.no_eff && !(flags & DC_UPD_NOISY) && !getenv("DC_ALLOW_EPSILON_NO_EFF_ETA0"))
        return fail(DC_ERR_UNSUPPORTED, "EPSILON model with full attention (no_eff) at eta = 0 is outside the 1e-3 parity bound (up to 1.3e-3); "
                                        "use linear attention, or eta > 0");
    // known values (dc_sampler_set_known) serve the loops of the conditioning they were set for; any other clears them
    if (s->known_mask && !(s->known_set_for == s->known_for())) s->known_val = s->known_mask = s->known_noise = nullptr;
    const bool known = s->known_mask != nullptr;
    if (known && S > 1 && !(h_coef[5] > 0.f))      // (the first iteration's row: abar_prev < 1 there)
        return fail(DC_ERR_INVALID, "known values are set: the loop needs the [S][8] table of dc_ddim_coefficients_known (slot 5 = sqrt(1 - abar_prev))");
    if (known && profile) return fail(DC_ERR_UNSUPPORTED, "dc_sampler_profile_loop does not run with known values set");
    if (known) flags |= DC_UPD_KNOWN;
    if (s->smooth_window > 0 && s->user_frames() < s->smooth_window)       // (before anything is enqueued: a failed call leaves no work and no half-ordered streams)
        return fail(DC_ERR_INVALID, "smoothing window %d exceeds the %d frames of a clip", s->smooth_window, s->user_frames());
    return DC_OK;
}

// loop_common, step 2: the loop's buffers, its per-iteration tables and its starting state, enqueued behind the caller's stream.
// flags gains ZSTEP.  MP: elements of x and of one snapshot, in the caller's layout (guided: its B clips, half the internal batch)
int loop_prepare(dc_sampler* s, const LoopCall& c, int& flags, size_t MP) {
    const int S = c.n, n_snap = c.n_snap;
    const int32_t *h_t = c.h_timesteps, *h_snap_iters = c.h_snap_iters;
    const float* h_coef = c.h_rows;
    int rc;
    if ((rc = ensure_steps(s, S))) return rc;
    if ((rc = grow(s, s->d_snaps, s->cap_snap, (size_t)n_snap * MP, 4, true))) return rc;      // (in elements: the batch may have grown since the last call)
    // Per-iteration tables on the device: uploaded only when (S, coefficients, snapshot iterations) differ from the
    // previous call - a sampling service calls the loop with the same schedule every time, and the four small H2D
    // copies + the stream synchronisation they need cost as much as several kernels at bs=1.
    std::vector<int> snap_of_iter(S, -1);
    for (int k = 0; k < n_snap; ++k) {
        if (h_snap_iters[k] < 0 || h_snap_iters[k] >= S) return fail(DC_ERR_INVALID, "snapshot iteration %d outside [0,%d)", h_snap_iters[k], S);
        snap_of_iter[h_snap_iters[k]] = k;
    }
    std::vector<int> t_of_iter(S);
    for (int i = 0; i < S; ++i) t_of_iter[i] = h_t ? h_t[i] : S - 1 - i;            // indices = range(num_timesteps)[::-1] (gaussian_diffusion.py:943)
    const bool same_tables = s->tables_S == S && s->tab_snap == snap_of_iter && s->tab_t == t_of_iter &&
                             memcmp(s->tab_coef_iter.data(), h_coef, (size_t)S * DC_COEF * 4) == 0;
    // the history of the second-order update: one more [B][Tx][P] buffer, zeroed below
    if ((flags & DC_UPD_MULTISTEP) && (rc = grow(s, s->d_x0_prev, s->cap_x0_prev, MP, 4, true))) return rc;
    // eta > 0: the caller's [S][B][Tx][P] draws, or - none given, a seed set - one iteration's draws generated at the head of every step
    // (d_zstep is an argument of the captured k_step_noise launches)
    const float* zbase = (flags & DC_UPD_NOISY) ? c.d_step_noise : nullptr;
    if ((flags & DC_UPD_NOISY) && !zbase) {
        if ((rc = grow(s, s->d_zstep, s->cap_zstep, MP, 4, true))) return rc;
        zbase = s->d_zstep;
        flags |= DC_UPD_ZSTEP;
    }
    s->upd_flags = flags;
    if ((rc = sync_in(s, (hipStream_t)c.stream))) return rc;
    hipStream_t st = s->stream;
    // the status word reports on THIS loop: bits left by earlier work on the sampler (a dc_sampler_denoise, a loop nobody asked
    // about) must not fail it
    HIP_TRY(hipMemsetAsync(s->d_status, 0, 4, st));
    HIP_TRY(dc_launch_set_ptr(st, s->d_zslot, zbase, s->noise_seed, s->noise_first));
    if (flags & DC_UPD_ZSTEP) s->noise_seed_set = false;       // a seed serves ONE loop: a later loop without a new one must not replay its draws
    if (!same_tables) {
        HIP_TRY(hipStreamSynchronize(st));          // an earlier call's copies out of the member vectors are done
        s->tables_S = 0;
        s->tab_t = t_of_iter;
        s->tab_snap = snap_of_iter;
        s->tab_coef_iter.assign(h_coef, h_coef + (size_t)S * DC_COEF);
        HIP_TRY(hipMemcpyAsync(s->d_t_of_iter, s->tab_t.data(), S * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->d_snap_of_iter, s->tab_snap.data(), S * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(s->d_coef_of_iter, s->tab_coef_iter.data(), (size_t)S * DC_COEF * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));          // pageable sources: the copies have left the host vectors
        s->tables_S = S;
    }
    HIP_TRY(hipMemsetAsync(s->d_iter, 0, 16, st));
    if (flags & DC_UPD_MULTISTEP) HIP_TRY(hipMemsetAsync(s->d_x0_prev, 0, MP * 4, st));      // (kappa is 0 in the first step: the zeros are read, never used)
    float* x0 = s->win_W > 0 ? s->d_xp : s->d_x;      // the loop's state in the caller's layout (windows: piece space)
    HIP_TRY(hipMemcpyAsync(x0, c.d_noise, MP * 4, hipMemcpyDeviceToDevice, st));
    if (flags & DC_UPD_KNOWN) {      // x_T of the known elements at the loop's starting level (slots 6, 7 of the first step's row)
        const float* c0 = h_coef;
        HIP_TRY(dc_launch_set_known(st, s->d_kslot, s->known_val, s->known_mask, s->known_noise));
        HIP_TRY(dc_launch_known_blend(st, x0, s->known_val, s->known_mask, s->known_noise, c0[6], c0[7], MP));
    }
    if (s->win_W > 0)     // every window's slot of x (both halves of a guided loop) starts from its rows of the piece, behind the blend
        HIP_TRY(dc_launch_windows_gather(st, s->d_xp, s->d_x, s->guided ? 2 : 1, s->user_B(), s->win_W, s->Tx, s->win_L, s->cfg.input_feats, s->d_winslot));
    else if (s->guided)   // both halves of x start equal (behind the blend)
        HIP_TRY(hipMemcpyAsync(s->d_x + MP, s->d_x, MP * 4, hipMemcpyDeviceToDevice, st));
    if (s->guided) HIP_TRY(dc_launch_set_scale(st, s->d_wslot, s->guide_w));      // ... and the scale goes into its slot
    return DC_OK;
}

// The graph cache's lookup: makes the graph of `key` the current one (the last entry) - the current one already, a parked one, or a new
// capture of what `enqueue` puts on st - and returns it
template <class F>
int find_or_capture(dc_sampler* s, hipStream_t st, const GraphKey& key, hipGraphExec_t* out, F&& enqueue) {
    auto& gs = s->graphs;
    if (gs.empty() || gs.back().first != key) {
        if (gs.size() > 3) {        // the current graph is parked: the oldest parked one makes room
            hipGraphExecDestroy(gs.front().second);
            gs.erase(gs.begin());
        }
        auto it = std::find_if(gs.begin(), gs.end(), [&](const auto& g) { return g.first == key; });
        if (it != gs.end()) {
            std::rotate(it, it + 1, gs.end());      // captured before: it becomes the current graph
        } else {
            hipGraph_t g = nullptr;
            HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            if (int rc = enqueue()) {
                hipStreamEndCapture(st, &g);
                if (g) hipGraphDestroy(g);
                return rc;
            }
            HIP_TRY(hipStreamEndCapture(st, &g));
            hipGraphExec_t exec = nullptr;
            hipError_t e = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0);
            hipGraphDestroy(g);
            if (e != hipSuccess) return fail(DC_ERR_HIP, "hipGraphInstantiate: %s", hipGetErrorString(e));
            gs.push_back({key, exec});
        }
    }
    *out = gs.back().second;
    return DC_OK;
}

// One sampling loop: validate, prepare, plan (loop_plan, dc_form.h: eager or captured, which graphs, how often), then run the plan's
// parts and write the result.  flags: the caller's DC_UPD_* + NOISY / MULTISTEP as run_loop found them in the rows
int loop_common(dc_sampler* s, const LoopCall& c, int flags) {
    int rc;
    if ((rc = loop_validate(s, c, flags))) return rc;
    const size_t MP = s->user_elems();
    if ((rc = loop_prepare(s, c, flags, MP))) return rc;
    hipStream_t st = s->stream;
    const char* env_tail = getenv("DC_PRECISE_TAIL");      // (DC_PRECISE_TAIL=k overrides the sampler's precise tail: loop_tail)
    LoopOpts lo;
    lo.S = c.n, lo.flags = flags, lo.guided = s->guided, lo.takes = s->takes, lo.windows = s->win_W, lo.win_L = s->win_L, lo.profile = c.profile;
    lo.no_graph = getenv("DC_DISABLE_GRAPH") != nullptr, lo.tail_split = s->tail_split;
    if (env_tail) lo.env_tail = atoi(env_tail);
    const Switches sw = Switches::read();
    const LoopPlan plan = loop_plan(Geometry{s->B, s->T, s->Tx, s->G, s->num_cu, s->cap_rec_floats}, settings_of(s), sw, lo);
    for (const LoopPart& part : plan.parts) {
        auto enqueue_part = [&]() -> int {
            bool embedded = false;      // (a sequence's first step does its own front work, its last step nobody else's)
            StepDone d;
            for (int i = 0; i < part.steps; ++i) {
                Step step;
                static_cast<StepOpts&>(step) = loop_step(plan, part, lo, i);
                step.embedded = embedded, step.x_src = step.x_dst = s->d_x;
                if (int rc = enqueue_step(s, st, step, sw, &d)) return rc;
                embedded = d.embedded_next;
            }
            // captured steps that indexed the iteration tables themselves did not advance the counter (see enqueue_step)
            if (!plan.eager && d.folded)
                if (hipError_t ea = dc_launch_advance_iter(st, s->d_iter, part.steps)) return fail(DC_ERR_HIP, "k_advance_iter: %s", hipGetErrorString(ea));
            return DC_OK;
        };
        if (plan.eager) {
            if ((rc = enqueue_part())) return rc;
            continue;
        }
        hipGraphExec_t graph = nullptr;
        if ((rc = find_or_capture(s, st, part.key, &graph, enqueue_part))) return rc;
        for (int i = 0; i < part.launches; ++i) HIP_TRY(hipGraphLaunch(graph, st));
    }
    // the final write x0 -> the caller's tensor: a copy, or (dc_sampler_set_smoothing) the Savitzky-Golay filter along time
    // (tools/visualization.py:20-26,126) reading the loop's x0 and writing the caller's tensor directly - no pass of its own
    const float* x_end = s->win_W > 0 ? s->d_xp : s->d_x;      // (guided: the first half; windows: the piece)
    if (s->smooth_window > 0) {
        HIP_TRY(dc_launch_savgol(st, x_end, c.d_out, s->d_smooth_coef, s->user_B(), s->user_frames(), s->cfg.input_feats, s->smooth_window));
    } else {
        HIP_TRY(hipMemcpyAsync(c.d_out, x_end, MP * 4, hipMemcpyDeviceToDevice, st));
    }
    if (c.n_snap > 0 && c.d_snaps)
        HIP_TRY(hipMemcpyAsync(c.d_snaps, s->d_snaps, (size_t)c.n_snap * MP * 4, hipMemcpyDeviceToDevice, st));
    return sync_out(s, (hipStream_t)c.stream);
}

// A public per-TIMESTEP table [S][width] (width 4: dc_ddim_coefficients, sigma = 0; 8: dc_ddim_coefficients_ex / _known) as the rows
// PER ITERATION of the loop over t = S-1 .. 0, in the internal width (slots past `width` are 0: no history term)
std::vector<float> rows_of_table(const float* h_coef, int S, int width) {
    std::vector<float> rows((size_t)(S > 0 ? S : 0) * DC_COEF, 0.f);
    if (h_coef)
        for (int i = 0; i < S; ++i) memcpy(&rows[(size_t)DC_COEF * i], h_coef + (size_t)width * (S - 1 - i), (size_t)width * 4);
    return rows;
}

// One row of the update's scalars for a step from noise level abar = a64 to abar_next = an64 (`last`: to 1, the clean sample), slots 0..7
// as dc_ddim.h lists them: fp32 arithmetic on the fp32-rounded table entries, in the order ddim_sample evaluates them
// (gaussian_diffusion.py:812-826).  The one copy of these roundings: dc_ddim_coefficients_ex / _known call it with (abar_t, abar_{t-1}),
// dc_solver_table with the sub-schedule's pair.
void ddim_row8(double a64, bool last, double an64, float eta, float* c) {
    const float a = (float)a64, a_prev = last ? 1.0f : (float)an64;
    const float sigma = eta * sqrtf((1.0f - a_prev) / (1.0f - a)) * sqrtf(1.0f - a / a_prev);
    c[0] = (float)std::sqrt(1.0 / a64);
    c[1] = (float)std::sqrt(1.0 / a64 - 1.0);
    c[2] = sqrtf(a_prev);
    c[3] = sqrtf(1.0f - a_prev - sigma * sigma);
    c[4] = sigma;
    c[5] = sqrtf(1.0f - a_prev);      // (dc_ddim_coefficients' column 3: the same expression and rounding)
    c[6] = sqrtf(a);
    c[7] = sqrtf(1.0f - a);
}

// the per-kernel sums of a profiled loop's events (dc_sampler_profile_loop, dc_sampler_solver_profile_loop)
int collect_profile(dc_sampler* s, float* h_ms, int32_t* h_count, int n) {
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (int i = 0; i < n; ++i) {
        h_ms[i] = 0.f;
        h_count[i] = 0;
    }
    for (size_t i = 0; i < s->prof.ids.size(); ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s->prof.ev[2 * i], s->prof.ev[2 * i + 1]));
        const int id = s->prof.ids[i];
        if (id < n) {
            h_ms[id] += ms;
            h_count[id] += 1;
        }
    }
    for (hipEvent_t e : s->prof.ev) hipEventDestroy(e);
    s->prof.ev.clear();
    s->prof.ids.clear();
    return DC_OK;
}

// The one loop call behind the five public entry points: the checks of the caller's arguments, then loop_common (and, profiled, the sums)
int run_loop(dc_sampler* s, const LoopCall& c) {
    if (c.profile && (!s || !c.h_ms || !c.h_count)) return fail(DC_ERR_INVALID, "null argument");
    if (s) HIP_TRY(hipSetDevice(s->cfg.device));
    if (c.profile) s->prof.ev.clear(), s->prof.ids.clear();
    if (c.listed && !s) return fail(DC_ERR_INVALID, "null sampler");
    if (c.n_snap < 0 || (c.n_snap > 0 && (!c.h_snap_iters || !c.d_snaps))) return fail(DC_ERR_INVALID, "bad snapshot arguments");
    if (c.flags & ~(DC_UPD_CLIP | DC_UPD_EPS)) return fail(DC_ERR_INVALID, "unknown update flags 0x%x", c.flags);
    const int32_t* h_t = c.h_timesteps;
    if (c.listed) {
        if (!h_t || !c.h_rows) return fail(DC_ERR_INVALID, "null pointer argument");
        if (c.n < 1 || c.n > s->cfg.max_timesteps) return fail(DC_ERR_INVALID, "%d timesteps outside [1, max_timesteps=%d]", c.n, s->cfg.max_timesteps);
    }
    // (a table converted by rows_of_table has no slot 8: only a caller's rows can ask for the multistep update)
    bool noisy = false, multi = false;
    for (int i = 0; c.h_rows && i < c.n; ++i) {
        if (c.listed && (h_t[i] < 0 || h_t[i] >= s->cfg.max_timesteps || (i > 0 && h_t[i] >= h_t[i - 1])))
            return fail(DC_ERR_INVALID, "timesteps must be strictly decreasing inside [0, max_timesteps=%d): entry %d is %d", s->cfg.max_timesteps, i, h_t[i]);
        noisy = noisy || c.h_rows[(size_t)DC_COEF * i + 4] != 0.f;
        multi = multi || c.h_rows[(size_t)DC_COEF * i + 8] != 0.f;
    }
    if (multi && (c.h_rows[8] != 0.f || c.h_rows[(size_t)DC_COEF * (c.n - 1) + 8] != 0.f))
        return fail(DC_ERR_INVALID, "the history coefficient (slot 8) must be 0 in the first row (no history yet) and in the last (the final sample is the model's x0)");
    if (multi && noisy) return fail(DC_ERR_INVALID, "the second-order multistep update is deterministic: rows with a history coefficient need sigma = 0 (eta = 0)");
    if (noisy && !c.d_step_noise && !(s && s->noise_seed_set))
        return fail(DC_ERR_INVALID, "sigma != 0 (eta > 0) needs the per-iteration noise: the tensor d_step_noise [%s][B][T][P], or a seed "
                    "(dc_sampler_set_step_noise_seed) for draws generated step by step", c.listed ? "n" : "S");
    const int rc = loop_common(s, c, c.flags | (noisy ? DC_UPD_NOISY : 0) | (multi ? DC_UPD_MULTISTEP : 0));
    return (rc || !c.profile) ? rc : collect_profile(s, c.h_ms, c.h_count, c.n_kernels);
}

// dc_sampler_denoise; the debug entry points run it with their test hooks
int denoise(dc_sampler* s, const float* d_x, const int32_t* h_timesteps, float* d_out, void* stream, const Hooks& dbg) {
    if (!s || !s->finalized) return fail(DC_ERR_INVALID, "sampler not finalized");
    if (!s->cond_set) return fail(DC_ERR_INVALID, "dc_sampler_set_conditioning must be called first");
    if (!d_x || !h_timesteps || !d_out) return fail(DC_ERR_INVALID, "null pointer argument");
    if (s->guided)
        return fail(DC_ERR_INVALID, "the conditioning is guided (dc_sampler_set_conditioning_guided): single evaluations are not guided - per-clip "
                                    "timesteps break the unconditional half's shared FiLM column; call dc_sampler_set_conditioning and combine on your side");
    if (s->win_W > 0)
        return fail(DC_ERR_INVALID, "the conditioning holds the windows of longer pieces (dc_sampler_set_conditioning_windows): single evaluations "
                                    "have no piece to blend into; call dc_sampler_set_conditioning on the windows' features");
    if (s->takes > 1)
        return fail(DC_ERR_INVALID, "the conditioning holds %d takes per music (dc_sampler_set_conditioning_takes): single evaluations take per-clip "
                                    "timesteps, which break the takes' shared FiLM tiles; call dc_sampler_set_conditioning on tiled features", s->takes);
    for (int b = 0; b < s->B; ++b)
        if (h_timesteps[b] < 0 || h_timesteps[b] >= s->cfg.max_timesteps)
            return fail(DC_ERR_INVALID, "timestep %d outside [0,%d)", h_timesteps[b], s->cfg.max_timesteps);
    HIP_TRY(hipSetDevice(s->cfg.device));
    hipStream_t user = (hipStream_t)stream, st = s->stream;
    int rc;
    if ((rc = sync_in(s, user))) return rc;
    HIP_TRY(hipMemcpyAsync(s->d_t_clip, h_timesteps, (size_t)s->B * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    Step c;
    c.x_src = d_x, c.x_dst = d_out, c.split = s->precise_forward && can_split_steps(settings_of(s), dbg), c.dbg = dbg;
    if ((rc = enqueue_step(s, st, c, Switches::read()))) return rc;
    return sync_out(s, user);
}

}  // namespace

// the other translation units' way to set dc_last_error's message (dc_stgcn.hip); not exported
int dc_set_error(int code, const char* msg) { return fail(code, "%s", msg); }

// ======================================================================================
// C ABI
// ======================================================================================
extern "C" {

static_assert(DC_UPDATE_CLIP_DENOISED == DC_UPD_CLIP && DC_UPDATE_EPSILON == DC_UPD_EPS && DC_STATUS_F16_SATURATED == DC_STATUS_F16_SAT &&
                  DC_STATUS_TIMEOUT == DC_STATUS_SYNC_TIMEOUT,
              "include/dc_ddim.h and dc_common.h disagree");
static_assert(DC_SOLVER_ROW == DC_COEF, "include/dc_ddim.h and dc_common.h disagree on the row width");
static_assert(DC_PREC_BF16 == DCF_BF16 && DC_PREC_MIXED == DCF_MIXED && DC_PREC_BF16X3 == DCF_BF16X3 && DC_PREC_FP16 == DCF_FP16,
              "include/dc_ddim.h and dc_form.h disagree");

const char* dc_last_error(void) { return g_err.c_str(); }
const char* dc_version(void) { return "dc_ddim 0.1 (gfx950)"; }

int dc_linear_beta_schedule(int32_t n, double* betas, double* ac, double* ac_prev, double* sr, double* srm1) {
    if (n < 1 || !betas) return fail(DC_ERR_INVALID, "bad schedule arguments");
    const double scale = 1000.0 / n, b0 = scale * 0.0001, b1 = scale * 0.02;
    double cp = 1.0;
    for (int i = 0; i < n; ++i) {
        // np.linspace(start, stop, n): start + i*step with step=(stop-start)/(n-1); last point is `stop` exactly
        const double step = n > 1 ? (b1 - b0) / (n - 1) : 0.0;
        betas[i] = (i == n - 1 && n > 1) ? b1 : b0 + i * step;
        const double prev = cp;
        cp *= (1.0 - betas[i]);
        if (ac) ac[i] = cp;
        if (ac_prev) ac_prev[i] = prev;
        if (sr) sr[i] = std::sqrt(1.0 / cp);
        if (srm1) srm1[i] = std::sqrt(1.0 / cp - 1.0);
    }
    return DC_OK;
}

int dc_ddim_coefficients(int32_t n, const double* ac, float* coef) {
    if (n < 1 || !ac || !coef) return fail(DC_ERR_INVALID, "bad coefficient arguments");
    for (int t = 0; t < n; ++t) {
        const float a_prev = t == 0 ? 1.0f : (float)ac[t - 1];
        coef[4 * t + 0] = (float)std::sqrt(1.0 / ac[t]);
        coef[4 * t + 1] = (float)std::sqrt(1.0 / ac[t] - 1.0);
        coef[4 * t + 2] = sqrtf(a_prev);
        coef[4 * t + 3] = sqrtf(1.0f - a_prev);
    }
    return DC_OK;
}

int dc_ddim_coefficients_ex(int32_t n, const double* ac, float eta, float* coef8) {
    if (n < 1 || !ac || !coef8 || !(eta >= 0.f)) return fail(DC_ERR_INVALID, "bad coefficient arguments");
    for (int t = 0; t < n; ++t) {
        float* c = coef8 + (size_t)8 * t;
        ddim_row8(ac[t], t == 0, t == 0 ? 1.0 : ac[t - 1], eta, c);
        c[5] = c[6] = c[7] = 0.f;
    }
    return DC_OK;
}

int dc_ddim_coefficients_known(int32_t n, const double* ac, float eta, float* coef8, float* start2) {
    if (n < 1 || !ac || !coef8 || !(eta >= 0.f)) return fail(DC_ERR_INVALID, "bad coefficient arguments");
    for (int t = 0; t < n; ++t) ddim_row8(ac[t], t == 0, t == 0 ? 1.0 : ac[t - 1], eta, coef8 + (size_t)8 * t);
    if (start2) start2[0] = coef8[(size_t)8 * (n - 1) + 6], start2[1] = coef8[(size_t)8 * (n - 1) + 7];
    return DC_OK;
}

int dc_solver_table(int32_t n_train, const double* ac, const int32_t* ts, int32_t n, float eta, int32_t order, float* rows, float* start2) {
    if (n_train < 1 || !ac || !ts || !rows || !(eta >= 0.f)) return fail(DC_ERR_INVALID, "bad solver table arguments");
    if (n < 1) return fail(DC_ERR_INVALID, "a solver loop needs at least one timestep (n = %d)", n);
    if (order != 1 && order != 2) return fail(DC_ERR_INVALID, "solver order %d: 1 (DDIM) and 2 (multistep, DPM-Solver++ 2M) are built", order);
    if (order == 2 && eta != 0.f) return fail(DC_ERR_INVALID, "the second-order multistep update is deterministic: eta must be 0 (got %g)", (double)eta);
    for (int i = 0; i < n; ++i)
        if (ts[i] < 0 || ts[i] >= n_train || (i > 0 && ts[i] >= ts[i - 1]))
            return fail(DC_ERR_INVALID, "timesteps must be strictly decreasing inside [0, %d): entry %d is %d", n_train, i, ts[i]);
    // lambda = log(alpha / sigma) = 1/2 ln(abar / (1 - abar)), the half log-SNR the solver steps in
    const auto lam = [](double a) { return 0.5 * std::log(a / (1.0 - a)); };
    for (int i = 0; i < n; ++i) {
        float* c = rows + (size_t)DC_SOLVER_ROW * i;
        const bool last = i == n - 1;
        const double a = ac[ts[i]], an = last ? 1.0 : ac[ts[i + 1]];
        ddim_row8(a, last, an, eta, c);
        for (int k = 8; k < DC_SOLVER_ROW; ++k) c[k] = 0.f;
        if (order == 2 && i > 0 && !last) {
            const double la = lam(a), h = lam(an) - la, h_before = la - lam(ac[ts[i - 1]]), r = h_before / h;
            c[8] = (float)((std::sqrt(an) - std::sqrt(1.0 - an) * std::sqrt(a) / std::sqrt(1.0 - a)) / (2.0 * r));
        }
    }
    if (start2) start2[0] = rows[6], start2[1] = rows[7];      // the first iteration's level: the loop starts at abar[ts[0]]
    return DC_OK;
}

int dc_pack_weight(const float* w, int32_t n_out, int32_t k_in, int32_t chained, uint16_t* hi, uint16_t* lo) {
    if (!w || !hi || !lo || n_out < 1 || k_in < 1) return fail(DC_ERR_INVALID, "bad pack arguments");
    pack_weight(w, n_out, k_in, chained != 0, hi, lo);
    return DC_OK;
}

int dc_sampler_create(const dc_config* cfg, dc_sampler** out) {
    if (!cfg || !out) return fail(DC_ERR_INVALID, "null argument");
    if (cfg->latent_dim != DC_D || cfg->num_heads != DC_H || cfg->ff_size != DC_F)
        return fail(DC_ERR_UNSUPPORTED, "built for latent_dim=128, num_heads=8, ff_size=64 (got %d, %d, %d); latent_dim*4 must equal 512 "
                    "(transformer.py:385,404,482)", cfg->latent_dim, cfg->num_heads, cfg->ff_size);
    if (cfg->input_feats < 1 || cfg->input_feats > DC_PMAX) return fail(DC_ERR_UNSUPPORTED, "input_feats must be in [1,32]");
    if (cfg->num_layers < 1 || cfg->num_layers > DC_MAX_LAYERS) return fail(DC_ERR_UNSUPPORTED, "num_layers must be in [1,%d]", DC_MAX_LAYERS);
    // (bf16 attention operands - scores, weights and values on 8 mantissa bits - leave 1.0 - 1.8e-3 on x0 whatever the precise tail
    // (tools/fuzz_shapes.py, profiles/r06_fuzz_bf16_tail.txt): outside the parity bound, so the combination is not offered)
    if (cfg->no_eff && cfg->precision != DC_PREC_FP16)
        return fail(DC_ERR_UNSUPPORTED, "no_eff (full T x T attention) is built for the fp16 precision only (bf16 attention operands leave 1 - 2e-3 on x0: outside the 1e-3 parity bound)");
    if (cfg->precision < DC_PREC_BF16 || cfg->precision > DC_PREC_FP16) return fail(DC_ERR_INVALID, "unknown precision %d", cfg->precision);
    if (cfg->max_timesteps < 1) return fail(DC_ERR_INVALID, "max_timesteps must be >= 1");
    int ndev = 0;
#ifdef DC_HOST_SANITIZE
    // Sanitizer build of the HOST half (address + undefined-behaviour sanitizers on the CPU; GPU sanitizers are not available on this
    // pool): without a device the sampler is created "host only" - parameter store, validation, weight folding and packing into the
    // arena (pack_model; the music encoder's music_pack too) run as in production, nothing is uploaded or launched, and every entry point that needs the device fails with NO_DEVICE.
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        dc_sampler* h = new dc_sampler();
        h->cfg = *cfg;
        h->host_only = true;
        h->num_cu = 256;
        h->set_precision(cfg->precision);
        *out = h;
        return DC_OK;
    }
#endif
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(DC_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(DC_ERR_INVALID, "device %d out of range (0..%d)", cfg->device, ndev - 1);
    HIP_TRY(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(DC_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);
    dc_sampler* s = new dc_sampler();
    s->cfg = *cfg;
    s->num_cu = prop.multiProcessorCount;
    s->set_precision(cfg->precision);
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming) != hipSuccess) {
        delete s;
        return fail(DC_ERR_HIP, "stream/event creation failed");
    }
    *out = s;
    return DC_OK;
}

void dc_sampler_destroy(dc_sampler* s) {
    if (!s) return;
    if (s->host_only) {          // (sanitizer build without a device: the arena is host memory)
        free(s->d_arena);
        delete s;
        return;
    }
    hipSetDevice(s->cfg.device);
    hipDeviceSynchronize();
    drop_graph(s);
    void* ptrs[] = {s->d_arena, s->d_model, s->d_model_split, s->d_length, s->d_pp, s->d_s_hi, s->d_s_lo, s->d_E, s->d_h, s->d_recs, s->d_a_sa,
                    s->d_a_ca, s->d_x, s->d_snaps, s->d_recs_ca, s->d_nh_hi, s->d_nh_lo, s->d_iter,
                    s->d_t_clip, s->d_snap_cur, s->d_t_of_iter, s->d_snap_of_iter, s->d_coef_cur, s->d_x0_prev, s->d_coef_of_iter,
                    s->d_kv_sa[0], s->d_kv_sa[1], s->d_kv_ca, s->d_stamps, s->d_film_rate, s->d_status, s->d_smooth_coef, s->d_zslot, s->d_kslot, s->d_zstep, s->d_a_ca16, s->d_gran,
                    s->d_wslot, s->d_raw, s->d_xf2_proj, s->d_xf2_out, s->d_pp_share, s->d_xp, s->d_win_start, s->d_win_weight, s->d_winslot};
    for (void* p : ptrs)
        if (p) hipFree(p);
    dc_music_destroy(s->music);
    if (s->ev_in) hipEventDestroy(s->ev_in);
    if (s->ev_out) hipEventDestroy(s->ev_out);
    if (s->stream) hipStreamDestroy(s->stream);
    delete s;
}

int dc_sampler_set_param(dc_sampler* s, const char* name, const float* data, int64_t numel) {
    if (!s || !name || !data || numel < 0) return fail(DC_ERR_INVALID, "null argument");
    const std::string n(name);
    if (music_param(n)) {
        for (const auto& r : dc_music_required(DC_C))
            if (r.first == n) {
                if ((size_t)numel != r.second) return fail(DC_ERR_PARAM, "parameter %s has %lld elements, expected %zu", name, (long long)numel, r.second);
                s->params[n].assign(data, data + numel);
                s->finalized = false;
                return DC_OK;
            }
        return DC_OK;
    }
    for (const auto& r : required_params(s->cfg))
        if (r.name == n) {
            if ((size_t)numel != r.numel) return fail(DC_ERR_PARAM, "parameter %s has %lld elements, expected %zu", name, (long long)numel, r.numel);
            s->params[n].assign(data, data + numel);
            s->finalized = false;
            return DC_OK;
        }
    return fail(DC_ERR_PARAM, "unknown parameter key '%s'", name);
}

int dc_sampler_finalize_params(dc_sampler* s) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    for (const auto& r : required_params(s->cfg))
        if (!find(s, r.name)) return fail(DC_ERR_PARAM, "missing parameter '%s'", r.name.c_str());
    if (!s->host_only) HIP_TRY(hipSetDevice(s->cfg.device));
    drop_graph(s);
    s->cap_G = 0;   // NT may have changed: force workspace rebuild
    {
        ModelImage image;
        pack_model(s->cfg, *s, s->params, image);
        const int rc = upload_model(s, image);
        if (rc) return rc;
    }
    if (s->music) {
        dc_music_destroy(s->music);
        s->music = nullptr;
    }
    bool any_music = false;
    for (const auto& kv : s->params) any_music = any_music || music_param(kv.first);
    if (any_music) {
        std::string err;
        if (s->host_only) {      // (no device to build the encoder on: its BatchNorm folding and packing run all the same, for the sanitizers)
            if (!dc_music_check(s->params, DC_C, &err)) return fail(DC_ERR_PARAM, "music encoder: %s", err.c_str());
            music_pack(s->params);
        } else {
            s->music = dc_music_build(s->params, DC_C, &err);
            if (!s->music) return fail(DC_ERR_PARAM, "music encoder: %s", err.c_str());
            // one fp16 plane where the denoiser rounds the features to 16-bit operands anyway, split planes for the split-operand precisions
            dc_music_set_format(s->music, s->me_format >= 0 ? s->me_format : (s->split_small ? DC_ME_SPLIT : DC_ME_FP16));
        }
    }
    s->finalized = true;
    s->cond_set = false;
    return DC_OK;
}

// dc_sampler_set_conditioning over B clips; the guided entry point calls it with its 2 B internal clips
static int set_conditioning(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length, int32_t B, int32_t T,
                            void* stream) {
    if (!s || !s->finalized) return fail(DC_ERR_INVALID, "sampler not finalized");
    if (!d_xf_proj || !d_xf_out || B < 1 || T < 1) return fail(DC_ERR_INVALID, "bad conditioning arguments (need B >= 1, T >= 1)");
    if (T < 32 && clip_stride(s, B, T) < 32)
        return fail(DC_ERR_UNSUPPORTED, "T=%d: clips shorter than 32 frames need the padded clip stride (linear attention, DC_NO_PAD unset)", T);
    if (clip_stride(s, B, T) / 32 + 2 > 128) return fail(DC_ERR_UNSUPPORTED, "T=%d: the attention combine holds at most 128 token groups per clip (T <= 4032)", T);
    if (T > s->cfg.num_frames) return fail(DC_ERR_INVALID, "T=%d exceeds num_frames=%d rows of sequence_embedding", T, s->cfg.num_frames);
    if (s->host_only) return fail(DC_ERR_NO_DEVICE, "host-only sampler (sanitizer build without a device)");
    HIP_TRY(hipSetDevice(s->cfg.device));
    int rc;
    if ((rc = ensure_workspace(s, B, T))) return rc;
    s->pp_last = nullptr;      // (no FiLM GEMM has run on this conditioning yet)
    std::vector<int> len(B, T);
    if (h_length)
        for (int b = 0; b < B; ++b) {
            if (h_length[b] < 1 || h_length[b] > T) return fail(DC_ERR_INVALID, "length[%d]=%d outside [1,%d]", b, h_length[b], T);
            len[b] = h_length[b];
        }
    hipStream_t user = (hipStream_t)stream, st = s->stream;
    if ((rc = sync_in(s, user))) return rc;
    const int M = s->M, G = s->G, L = s->cfg.num_layers;
    const int Tx = T;
    T = s->T;                         // clip stride of the token space from here on (>= Tx)
    // The clip lengths are uploaded only when they differ from what the device holds (a service or an evaluation run passes the same
    // ones batch after batch): the upload reads host memory and needs the stream synchronisation below, which would otherwise make
    // every call wait for the previous batch's sampling loop (evaluate.py keeps the GPU's queue full).
    const bool same_len = s->len_dev == len && s->len_dev_ptr == s->d_length;
    if (!same_len) {
        HIP_TRY(hipStreamSynchronize(st));                 // an earlier upload out of the member vector is done
        s->len_dev = len;
        s->len_dev_ptr = nullptr;
        HIP_TRY(hipMemcpyAsync(s->d_length, s->len_dev.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
    }
    // emb's step-invariant term: linear(xf_proj) as fp32 operand image
    // (split-bf16 MFMAs, k_cond_pp64; DC_COND_512=1: the fp32 FMA form)
    if (!getenv("DC_COND_512"))
        HIP_TRY(dc_launch_cond_pp64(st, d_xf_proj, s->h_model.lin_pack, s->h_model.lin_b, s->d_pp, M, G, T, Tx));
    else
        HIP_TRY(dc_launch_cond_embed(st, 0, d_xf_proj, s->h_model.lin_wt, s->h_model.lin_b, s->d_pp, nullptr, nullptr, M, G, T, Tx));
    // cross-attention: linear(xf_out) -> text_norm (affine folded into K/V) -> per-layer K,V -> A_ca; one-time cost: always split
    // precision (plain bf16 here alone costs ~2e-3 on A_cross).  The linear-attention records come straight from the 64 music
    // features (`linear` composed into the projections on the host, k_cond_ca_partials64: an eighth of the products, no [tokens][512]
    // image in between); DC_COND_512=1 and the full-attention keys / values take the image (k_cond_embed<1>).
    const bool cond64 = !s->cfg.no_eff && !getenv("DC_COND_512");
    if (!cond64)
        HIP_TRY(dc_launch_cond_embed(st, 1, d_xf_out, s->h_model.lin_wt, s->h_model.lin_b, nullptr, s->d_nh_hi, s->d_nh_lo, M, G, T, Tx));
    if (s->cfg.no_eff) {
        HIP_TRY(dc_launch_ca_kv(st, s->small_fmt, s->d_model, s->d_nh_hi, s->d_nh_lo, s->d_kv_ca, M, T, G, B, s->KT, L));
    } else {
        if (cond64)      // (1 / std per token goes through the unused image buffer)
            HIP_TRY(dc_launch_ca_partials64(st, s->d_model, d_xf_out, s->h_model.lin_gram, reinterpret_cast<float*>(s->d_nh_hi), s->d_recs_ca, M, T, G, L, Tx));
        else
            HIP_TRY(dc_launch_ca_partials(st, s->d_model, s->d_nh_hi, s->d_nh_lo, s->d_recs_ca, M, T, G, L, Tx));
        HIP_TRY(dc_launch_attn_combine(st, s->small_fmt, s->d_recs_ca, s->d_a_ca, T, G, B, L, 32));
        if (!s->split_small) HIP_TRY(dc_launch_cond_af16(st, s->small_fmt, s->d_a_ca, s->d_a_ca16, L * B));      // (small batches: dc_layer16.hip)
    }
    if (!same_len) {
        HIP_TRY(hipStreamSynchronize(st));   // the lengths came out of host memory
        s->len_dev_ptr = s->d_length;
    }
    s->cond_set = true;
    return sync_out(s, user);
}

int dc_sampler_set_conditioning(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length,
                                int32_t B, int32_t T, void* stream) {
    const int rc = set_conditioning(s, d_xf_proj, d_xf_out, h_length, B, T, stream);
    // a plain conditioning switches guidance and takes off (a failed call on such a sampler leaves no conditioning set: the internal
    // batch may be half rebuilt)
    if (s && (s->guided || s->takes > 1 || s->win_W > 0)) s->guided = false, s->takes = 1, s->win_W = s->win_L = 0, s->cond_set = rc == DC_OK;
    return rc;      // (known values set on the guided / takes conditioning are dropped by the next loop: known_set_for)
}

// The conditionings whose internal batch is built here: `takes` runs of the caller's B clips (take-major), then - guided - as many
// unconditional shadows, every frame carrying the null pair.  takes = 1 guided is dc_sampler_set_conditioning_guided.
// Classifier-free guidance: the reference trains its denoiser for it - MotionTransformer.encode_music (models/transformer.py:389,451-459)
// zeroes a token's music features with probability cond_mask_prob = 0.1 before `proj` - and has no sampling counterpart.
static int set_conditioning_images(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length, int32_t B,
                                   int32_t T, int32_t takes, const float* h_null_proj, const float* h_null_out, void* stream) {
    const bool guided = h_null_proj != nullptr;
    if (!d_xf_proj || !d_xf_out || B < 1 || T < 1) return fail(DC_ERR_INVALID, "bad conditioning arguments (need B >= 1, T >= 1)");
    const long long Bi = (long long)B * takes * (guided ? 2 : 1);      // internal clips
    if (Bi > (1 << 30)) return fail(DC_ERR_INVALID, "B=%d, takes=%d: the internal batch holds %lld clips", B, takes, Bi);
    if (s->host_only) return fail(DC_ERR_NO_DEVICE, "host-only sampler (sanitizer build without a device)");
    HIP_TRY(hipSetDevice(s->cfg.device));
    s->guided = false, s->takes = 1, s->win_W = s->win_L = 0, s->cond_set = false;
    // the feature images of the internal clips: the caller's B, `takes` times, then every frame of the shadows carrying the null pair
    const size_t rows = (size_t)B * T, crows = rows * takes, irows = (size_t)Bi * T;
    int rc;
    // (no captured launch reads the two images: the pre-pass below runs on the stream itself)
    if ((rc = grow(s, s->d_xf2_proj, s->cap_xf2_proj, irows * 64, 4, false))) return rc;
    if ((rc = grow(s, s->d_xf2_out, s->cap_xf2_out, irows * 64, 4, false))) return rc;
    hipStream_t user = (hipStream_t)stream;
    for (int j = 0; j < takes; ++j) {
        HIP_TRY(hipMemcpyAsync(s->d_xf2_proj + (size_t)j * rows * 64, d_xf_proj, rows * 64 * 4, hipMemcpyDeviceToDevice, user));
        HIP_TRY(hipMemcpyAsync(s->d_xf2_out + (size_t)j * rows * 64, d_xf_out, rows * 64 * 4, hipMemcpyDeviceToDevice, user));
    }
    if (guided) {
        DcNull64 np{}, no{};
        memcpy(np.v, h_null_proj, sizeof np.v);
        memcpy(no.v, h_null_out, sizeof no.v);
        HIP_TRY(dc_launch_fill_rows64(user, s->d_xf2_proj + crows * 64, crows, np));
        HIP_TRY(dc_launch_fill_rows64(user, s->d_xf2_out + crows * 64, crows, no));
    }
    std::vector<int32_t> len2;
    if (h_length)
        for (long long j = 0; j < Bi / B; ++j) len2.insert(len2.end(), h_length, h_length + B);
    if ((rc = set_conditioning(s, s->d_xf2_proj, s->d_xf2_out, h_length ? len2.data() : nullptr, (int)Bi, T, stream))) return rc;
    s->cond_set = false;
    if (guided) {
        if ((rc = grow(s, s->d_raw, s->cap_raw, irows * s->cfg.input_feats, 4, true))) return rc;
        if (!s->d_wslot && (rc = dev_alloc(s, s->d_wslot, 16))) return rc;
        s->guide_w = 1.f;
        // guided takes: the FiLM GEMM over one take and the null column reads an operand image of its own (whatever the switches say
        // now: they are read again by every loop) - behind the pre-pass, which the caller's stream has been ordered after
        const FilmShare sh = film_share(s->B, s->T, s->G, true, takes, !s->split_film, Switches{});
        if (sh.period < sh.wrap) {
            const size_t gbytes = (size_t)32 * 64 * 8 * 4;      // one group of d_pp (ensure_workspace)
            if ((rc = grow(s, s->d_pp_share, s->cap_pp_share, (size_t)sh.groups, gbytes, true))) return rc;
            char* dst = reinterpret_cast<char*>(s->d_pp_share);
            const char* src = reinterpret_cast<const char*>(s->d_pp);
            HIP_TRY(hipMemcpyAsync(dst, src, (size_t)sh.period * gbytes, hipMemcpyDeviceToDevice, user));
            HIP_TRY(hipMemcpyAsync(dst + (size_t)sh.period * gbytes, src + (size_t)sh.wrap * gbytes, gbytes, hipMemcpyDeviceToDevice, user));
        }
    }
    s->guided = guided;
    s->takes = takes;
    s->cond_set = true;
    return DC_OK;
}

int dc_sampler_set_conditioning_guided(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length, int32_t B,
                                       int32_t T, const float* h_null_proj, const float* h_null_out, void* stream) {
    if (!s || !s->finalized) return fail(DC_ERR_INVALID, "sampler not finalized");
    if (!h_null_proj || !h_null_out) return fail(DC_ERR_INVALID, "guided conditioning: the null pair (h_null_proj[64], h_null_out[64]) is NULL");
    return set_conditioning_images(s, d_xf_proj, d_xf_out, h_length, B, T, 1, h_null_proj, h_null_out, stream);
}

int dc_sampler_set_conditioning_takes(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length, int32_t B,
                                      int32_t T, int32_t takes, const float* h_null_proj, const float* h_null_out, void* stream) {
    if (!s || !s->finalized) return fail(DC_ERR_INVALID, "sampler not finalized");
    if (takes < 1) return fail(DC_ERR_INVALID, "takes=%d: a conditioning holds at least one take per music", takes);
    if ((h_null_proj != nullptr) != (h_null_out != nullptr))
        return fail(DC_ERR_INVALID, "takes: the null pair is both vectors (guided) or neither (unguided); one of h_null_proj, h_null_out is NULL");
    if (takes == 1 && !h_null_proj) return dc_sampler_set_conditioning(s, d_xf_proj, d_xf_out, h_length, B, T, stream);
    return set_conditioning_images(s, d_xf_proj, d_xf_out, h_length, B, T, takes, h_null_proj, h_null_out, stream);
}

int dc_windows_check(const int32_t* h_start, const float* h_weight, int32_t W, int32_t T, int32_t L, const int32_t* h_length) {
    if (h_length) return fail(DC_ERR_INVALID, "windows are full: a conditioning over windows takes no h_length");
    const std::string why = windows_plan_error(h_start, h_weight, W, T, L);
    return why.empty() ? DC_OK : fail(DC_ERR_INVALID, "%s", why.c_str());
}

int dc_sampler_set_conditioning_windows(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length,
                                        const int32_t* h_start, const float* h_weight, int32_t B, int32_t W, int32_t T, int32_t L,
                                        const float* h_null_proj, const float* h_null_out, void* stream) {
    if (!s || !s->finalized) return fail(DC_ERR_INVALID, "sampler not finalized");
    if (B < 1) return fail(DC_ERR_INVALID, "bad conditioning arguments (need B >= 1, T >= 1)");
    if ((h_null_proj != nullptr) != (h_null_out != nullptr))
        return fail(DC_ERR_INVALID, "windows: the null pair is both vectors (guided) or neither (unguided); one of h_null_proj, h_null_out is NULL");
    int rc;      // the plan, on the host, before anything is enqueued or allocated
    if ((rc = dc_windows_check(h_start, h_weight, W, T, L, h_length))) return rc;
    const bool guided = h_null_proj != nullptr;
    if ((long long)B * W > (1 << 29)) return fail(DC_ERR_INVALID, "B=%d, W=%d: the internal batch holds %lld windows", B, W, (long long)B * W);
    // the internal batch: W B clips of T frames, window-major as the caller's features are (+ their shadows)
    if (guided)
        rc = set_conditioning_images(s, d_xf_proj, d_xf_out, nullptr, B * W, T, 1, h_null_proj, h_null_out, stream);
    else
        rc = dc_sampler_set_conditioning(s, d_xf_proj, d_xf_out, nullptr, B * W, T, stream);
    if (rc) return rc;
    s->cond_set = false;
    const size_t irows = (size_t)s->B * T, P = (size_t)s->cfg.input_feats;
    if ((rc = grow(s, s->d_raw, s->cap_raw, irows * P, 4, true))) return rc;
    if ((rc = grow(s, s->d_xp, s->cap_xp, (size_t)B * L * P, 4, true))) return rc;
    if ((rc = grow(s, s->d_win_start, s->cap_win_start, (size_t)W, 4, false))) return rc;       // (captured launches read the slot, not these)
    if ((rc = grow(s, s->d_win_weight, s->cap_win_weight, (size_t)W * T, 4, false))) return rc;
    if (!s->d_winslot && (rc = dev_alloc(s, s->d_winslot, sizeof(DcWindows)))) return rc;
    // the tables go up behind the sampler's earlier loops, which may still read the previous plan's (synchronous: host arrays)
    hipStream_t st = s->stream;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpyAsync(s->d_win_start, h_start, (size_t)W * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(s->d_win_weight, h_weight, (size_t)W * T * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(dc_launch_set_windows(st, s->d_winslot, s->d_win_start, s->d_win_weight));
    HIP_TRY(hipStreamSynchronize(st));
    s->win_W = W, s->win_L = L;
    s->cond_set = true;
    return DC_OK;
}

int dc_sampler_set_guidance_scale(dc_sampler* s, float w) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    if (!std::isfinite(w)) return fail(DC_ERR_INVALID, "guidance scale must be finite");
    if (!s->guided) return fail(DC_ERR_INVALID, "dc_sampler_set_conditioning_guided must be called first: the scale belongs to a guided conditioning");
    s->guide_w = w;
    return DC_OK;
}

int dc_sampler_set_precise_tail(dc_sampler* s, int32_t steps) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    if (steps < -1) return fail(DC_ERR_INVALID, "precise tail: steps >= 0, or -1 for the precision's default");
    s->tail_split = steps;
    return DC_OK;
}

int32_t dc_precise_tail_default(int32_t precision) {
    return precise_tail_default(precision);
}

int dc_sampler_set_clip_aligned(dc_sampler* s, int32_t mode) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    if (mode < -1 || mode > 1) return fail(DC_ERR_INVALID, "clip-aligned units: 1 (always), 0 (flat units), -1 (the library's rule)");
    s->clip_aligned = mode;
    return DC_OK;
}

int dc_sampler_set_idle_wave_path(dc_sampler* s, int32_t on) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    s->idle_wave_path = on != 0;
    return DC_OK;
}

int dc_sampler_set_precise_forward(dc_sampler* s, int32_t on) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    s->precise_forward = on != 0;
    return DC_OK;
}

int dc_sampler_set_combine_exchange(dc_sampler* s, int32_t on) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    s->l16_own = on == 0;
    return DC_OK;
}

int dc_sampler_set_encoder_format(dc_sampler* s, int32_t format) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    if (format != DC_ME_SPLIT && format != DC_ME_FP16) return fail(DC_ERR_INVALID, "encoder format %d (DC_ME_SPLIT = 0, DC_ME_FP16 = 1)", format);
    s->me_format = format;                                  // (kept across dc_sampler_finalize)
    if (s->music) dc_music_set_format(s->music, format);
    return DC_OK;
}

int dc_sampler_encode_music(dc_sampler* s, const float* d_mel, int32_t B, int32_t Tm, int32_t n_mels, float* d_xf_proj,
                            float* d_xf_out, void* stream) {
    if (!s || !s->finalized) return fail(DC_ERR_INVALID, "sampler not finalized");
    if (!s->music) return fail(DC_ERR_PARAM, "music encoder parameters (music_encoder.*, proj.*) were not supplied");
    if (!d_mel || !d_xf_proj || !d_xf_out || B < 1) return fail(DC_ERR_INVALID, "bad encode_music arguments");
    if (n_mels != 128) return fail(DC_ERR_UNSUPPORTED, "mel spectrograms must have 128 bins (conv4 takes 32 channels x 16 bins), got %d", n_mels);
    // (conv3 / conv4 run on (Tm - 1) / 3 + 1 rows, and reflection padding needs two: the reference's ReflectionPad2d raises below 4 frames)
    if (Tm < 4) return fail(DC_ERR_INVALID, "need at least 4 mel frames (reflection padding of the (Tm - 1) / 3 + 1 rows behind the stride-3 pool), got %d", Tm);
    HIP_TRY(hipSetDevice(s->cfg.device));
    hipStream_t user = (hipStream_t)stream, st = s->stream;
    int rc;
    if ((rc = sync_in(s, user))) return rc;
    std::string err;
    const hipError_t e = dc_music_encode(s->music, d_mel, B, Tm, d_xf_proj, d_xf_out, st, &err);
    if (e != hipSuccess) return fail(DC_ERR_HIP, "encode_music: %s %s", hipGetErrorString(e), err.c_str());
    return sync_out(s, user);
}

// Hat matrix H = A (A^T A)^-1 A^T of the degree-`order` polynomial fit over `window` equally spaced samples, fp64 normal
// equations with positions centred and scaled to [-1, 1] (well conditioned for the window sizes in use).
int dc_savgol_coefficients(int32_t window, int32_t order, float* h_coef) {
    if (window < 3 || !(window & 1) || window > 99 || order < 0 || order >= window || order > 10 || !h_coef)
        return fail(DC_ERR_INVALID, "savgol: need an odd window in [3,99] and 0 <= order < window (order <= 10)");
    const int w = window, n = order + 1, hw = w / 2;
    std::vector<double> A((size_t)w * n), G((size_t)n * n, 0.0), Ginv((size_t)n * n, 0.0);
    for (int i = 0; i < w; ++i) {
        const double u = (double)(i - hw) / hw;
        double pw = 1.0;
        for (int j = 0; j < n; ++j) {
            A[(size_t)i * n + j] = pw;
            pw *= u;
        }
    }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            double acc = 0.0;
            for (int i = 0; i < w; ++i) acc += A[(size_t)i * n + a] * A[(size_t)i * n + b];
            G[(size_t)a * n + b] = acc;
        }
    // Gauss-Jordan inverse with partial pivoting (n <= 11)
    std::vector<double> M((size_t)n * 2 * n, 0.0);
    for (int a = 0; a < n; ++a) {
        for (int b = 0; b < n; ++b) M[(size_t)a * 2 * n + b] = G[(size_t)a * n + b];
        M[(size_t)a * 2 * n + n + a] = 1.0;
    }
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(M[(size_t)r * 2 * n + c]) > std::fabs(M[(size_t)piv * 2 * n + c])) piv = r;
        if (std::fabs(M[(size_t)piv * 2 * n + c]) < 1e-300) return fail(DC_ERR_INVALID, "savgol: singular normal equations");
        if (piv != c)
            for (int k = 0; k < 2 * n; ++k) std::swap(M[(size_t)piv * 2 * n + k], M[(size_t)c * 2 * n + k]);
        const double d = M[(size_t)c * 2 * n + c];
        for (int k = 0; k < 2 * n; ++k) M[(size_t)c * 2 * n + k] /= d;
        for (int r = 0; r < n; ++r)
            if (r != c) {
                const double f = M[(size_t)r * 2 * n + c];
                if (f != 0.0)
                    for (int k = 0; k < 2 * n; ++k) M[(size_t)r * 2 * n + k] -= f * M[(size_t)c * 2 * n + k];
            }
    }
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) Ginv[(size_t)a * n + b] = M[(size_t)a * 2 * n + n + b];
    for (int i = 0; i < w; ++i)
        for (int k = 0; k < w; ++k) {
            double acc = 0.0;
            for (int a = 0; a < n; ++a) {
                double t = 0.0;
                for (int b = 0; b < n; ++b) t += Ginv[(size_t)a * n + b] * A[(size_t)k * n + b];
                acc += A[(size_t)i * n + a] * t;
            }
            h_coef[(size_t)i * w + k] = (float)acc;
        }
    return DC_OK;
}

int dc_sampler_set_smoothing(dc_sampler* s, int32_t window, int32_t order) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    HIP_TRY(hipSetDevice(s->cfg.device));
    if (window == 0) {
        s->smooth_window = 0;
        return DC_OK;
    }
    if (window == s->smooth_table_window && order == s->smooth_order && s->d_smooth_coef) {      // the table on the device is this one
        s->smooth_window = window;
        return DC_OK;
    }
    std::vector<float> coef((size_t)(window > 0 ? window : 0) * (window > 0 ? window : 0));
    int rc = dc_savgol_coefficients(window, order, coef.data());
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));          // an earlier loop may still read the old table
    if ((rc = dev_alloc(s, s->d_smooth_coef, coef.size() * 4))) return rc;
    HIP_TRY(hipMemcpy(s->d_smooth_coef, coef.data(), coef.size() * 4, hipMemcpyHostToDevice));
    s->smooth_window = s->smooth_table_window = window;
    s->smooth_order = order;
    return DC_OK;
}

int dc_savgol_filter(const float* d_in, float* d_out, int32_t B, int32_t T, int32_t P, int32_t window, int32_t order, void* stream) {
    if (!d_in || !d_out || d_in == d_out || B < 1 || P < 1) return fail(DC_ERR_INVALID, "savgol: bad arguments (in-place is not supported)");
    if (T < window) return fail(DC_ERR_INVALID, "savgol: T=%d shorter than the window %d", T, window);
    std::vector<float> coef((size_t)window * window);
    int rc = dc_savgol_coefficients(window, order, coef.data());
    if (rc) return rc;
    float* d_coef = nullptr;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMallocAsync((void**)&d_coef, coef.size() * 4, st));
    HIP_TRY(hipMemcpyAsync(d_coef, coef.data(), coef.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));          // `coef` is pageable host memory
    HIP_TRY(dc_launch_savgol(st, d_in, d_out, d_coef, B, T, P, window));
    HIP_TRY(hipFreeAsync(d_coef, st));
    return DC_OK;
}

int dc_sampler_denoise(dc_sampler* s, const float* d_x, const int32_t* h_timesteps, float* d_out, void* stream) {
    return denoise(s, d_x, h_timesteps, d_out, stream, Hooks{});
}

int dc_sampler_ddim_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t num_steps, const float* h_coef,
                         const int32_t* h_snap_iters, int32_t n_snap, float* d_snaps, void* stream) {
    const std::vector<float> rows = rows_of_table(h_coef, num_steps, 4);
    LoopCall c;
    c.d_noise = d_noise, c.d_out = d_out, c.n = num_steps, c.h_rows = h_coef ? rows.data() : nullptr;
    c.h_snap_iters = h_snap_iters, c.n_snap = n_snap, c.d_snaps = d_snaps, c.stream = stream;
    return run_loop(s, c);
}

int dc_sampler_ddim_loop_ex(dc_sampler* s, const float* d_noise, float* d_out, int32_t num_steps, const float* h_coef8,
                            int32_t flags, const float* d_step_noise, const int32_t* h_snap_iters, int32_t n_snap, float* d_snaps,
                            void* stream) {
    const std::vector<float> rows = rows_of_table(h_coef8, num_steps, 8);
    LoopCall c;
    c.d_noise = d_noise, c.d_out = d_out, c.n = num_steps, c.h_rows = h_coef8 ? rows.data() : nullptr, c.flags = flags, c.d_step_noise = d_step_noise;
    c.h_snap_iters = h_snap_iters, c.n_snap = n_snap, c.d_snaps = d_snaps, c.stream = stream;
    return run_loop(s, c);
}

int dc_sampler_solver_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t n, const int32_t* h_timesteps, const float* h_rows,
                           int32_t flags, const float* d_step_noise, const int32_t* h_snap_iters, int32_t n_snap, float* d_snaps, void* stream) {
    LoopCall c;
    c.d_noise = d_noise, c.d_out = d_out, c.n = n, c.listed = true, c.h_timesteps = h_timesteps, c.h_rows = h_rows, c.flags = flags;
    c.d_step_noise = d_step_noise, c.h_snap_iters = h_snap_iters, c.n_snap = n_snap, c.d_snaps = d_snaps, c.stream = stream;
    return run_loop(s, c);
}

int dc_sampler_set_known(dc_sampler* s, const float* d_known, const float* d_mask, const float* d_known_noise) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    if (!d_known && !d_mask && !d_known_noise) {
        s->known_val = s->known_mask = s->known_noise = nullptr;
        return DC_OK;
    }
    if (d_mask && !d_known) return fail(DC_ERR_INVALID, "known values: a mask without values (d_known is NULL)");
    if (d_mask && !d_known_noise) return fail(DC_ERR_INVALID, "known values: a mask without noise (d_known_noise is NULL; the known elements need one fixed draw)");
    if (!d_mask) return fail(DC_ERR_INVALID, "known values: values or noise without a mask (d_mask is NULL)");
    if (!s->cond_set) return fail(DC_ERR_INVALID, "dc_sampler_set_conditioning must be called first: known values belong to its (B, T)");
    s->known_val = d_known, s->known_mask = d_mask, s->known_noise = d_known_noise;
    s->known_set_for = s->known_for();
    return DC_OK;
}

int dc_sampler_set_step_noise_seed(dc_sampler* s, uint64_t seed) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    s->noise_seed = seed;
    s->noise_first = 0;
    s->noise_seed_set = true;
    return DC_OK;
}

int dc_sampler_set_step_noise_seed_at(dc_sampler* s, uint64_t seed, uint64_t first_element) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    s->noise_seed = seed;
    s->noise_first = first_element;
    s->noise_seed_set = true;
    return DC_OK;
}

int dc_step_noise_fill(float* d_out, int64_t n, uint64_t seed, int32_t iteration, void* stream) {
    if (!d_out || n < 0 || iteration < 0) return fail(DC_ERR_INVALID, "bad step-noise arguments");
    if (n == 0) return DC_OK;
    HIP_TRY(dc_launch_step_noise((hipStream_t)stream, d_out, (size_t)n, seed, nullptr, nullptr, iteration, nullptr, 0));
    return DC_OK;
}

int dc_sampler_status(dc_sampler* s, int32_t* h_status, int32_t clear) {
    if (!s || !h_status) return fail(DC_ERR_INVALID, "null argument");
    *h_status = 0;
    if (!s->d_status) return DC_OK;                      // nothing has run yet
    HIP_TRY(hipSetDevice(s->cfg.device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(h_status, s->d_status, 4, hipMemcpyDeviceToHost));
    // a timed-out combine exchange means the launch's workgroups were not co-resident (a shared GPU, or a second sampler's launches
    // on another stream): this sampler's later loops run the form without the exchange (a re-run of the failed loop is then valid)
    if (*h_status & DC_STATUS_SYNC_TIMEOUT) s->l16_own = true;
    if ((*h_status & DC_STATUS_NONFINITE) && !(*h_status & DC_STATUS_SYNC_TIMEOUT) && s->d_E && s->G > 0) {
        // diagnosis (failure path only): was it the fp16 storage of the FiLM tiles?  The range check is not in the production GEMM's
        // epilogue (it measured at 4 % of that kernel); the tiles are scanned here instead - the last step's as they stand, then,
        // while nothing was found, the tiles of every other timestep of the last loop (the GEMM re-run per timestep: the modulation
        // depends on t, and a value that saturates only early in the loop would otherwise read as an operand overflow)
        // (the groups the last loop's GEMM wrote: behind a guided loop with a shared column the tiles past them are stale or were never
        // written; the re-runs below cover the same groups)
        const int eg = s->last_film_groups > 0 ? std::min(s->last_film_groups, s->G) : s->G;
        const size_t ebytes = (size_t)eg * s->NT * 64 * 32;
        HIP_TRY(dc_launch_scan_f16(s->stream, s->d_E, ebytes, s->d_status));
        HIP_TRY(hipStreamSynchronize(s->stream));
        HIP_TRY(hipMemcpy(h_status, s->d_status, 4, hipMemcpyDeviceToHost));
        if (!(*h_status & DC_STATUS_F16_SAT) && s->cond_set && s->tables_S > 1 && s->d_t_clip) {
            std::vector<int> tc((size_t)s->B);
            for (int i = 0; i + 1 < s->tables_S && !(*h_status & DC_STATUS_F16_SAT); ++i) {
                std::fill(tc.begin(), tc.end(), s->tab_t[i]);
                HIP_TRY(hipMemcpy(s->d_t_clip, tc.data(), tc.size() * 4, hipMemcpyHostToDevice));
                if (s->split_film)
                    HIP_TRY(dc_launch_silu_emb(s->stream, s->film_fmt, true, s->d_pp, s->h_model.temb, s->d_t_clip, s->d_s_hi, s->d_s_lo, s->G, s->T, s->B));
                DcFilmArgs fa = film_args(s, s->split_film ? nullptr : (s->pp_last ? s->pp_last : s->d_pp), s->d_t_clip);
                fa.G = eg;
                HIP_TRY(dc_launch_film_gemm(s->stream, s->film_fmt, s->split_film, fa));
                HIP_TRY(dc_launch_scan_f16(s->stream, s->d_E, ebytes, s->d_status));
                HIP_TRY(hipStreamSynchronize(s->stream));
                HIP_TRY(hipMemcpy(h_status, s->d_status, 4, hipMemcpyDeviceToHost));
            }
        }
    }
    if (clear) HIP_TRY(hipMemset(s->d_status, 0, 4));
    return DC_OK;
}

int dc_sampler_profile_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t num_steps, const float* h_coef,
                            float* h_ms, int32_t* h_count, int32_t n, void* stream) {
    const std::vector<float> rows = rows_of_table(h_coef, num_steps, 4);
    LoopCall c;
    c.d_noise = d_noise, c.d_out = d_out, c.n = num_steps, c.h_rows = h_coef ? rows.data() : nullptr, c.stream = stream;
    c.profile = true, c.h_ms = h_ms, c.h_count = h_count, c.n_kernels = n;
    return run_loop(s, c);
}

int dc_sampler_solver_profile_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t n, const int32_t* h_timesteps, const float* h_rows,
                                   int32_t flags, float* h_ms, int32_t* h_count, int32_t n_kernels, void* stream) {
    LoopCall c;
    c.d_noise = d_noise, c.d_out = d_out, c.n = n, c.listed = true, c.h_timesteps = h_timesteps, c.h_rows = h_rows, c.flags = flags, c.stream = stream;
    c.profile = true, c.h_ms = h_ms, c.h_count = h_count, c.n_kernels = n_kernels;
    return run_loop(s, c);
}

int dc_sampler_debug_denoise(dc_sampler* s, const float* d_x, const int32_t* h_timesteps, float* d_out,
                             int32_t n_layers, int32_t stage, void* stream) {
    if (!s) return fail(DC_ERR_INVALID, "null sampler");
    return denoise(s, d_x, h_timesteps, d_out, stream, Hooks{n_layers, stage, -1});
}

int dc_sampler_debug_layer(dc_sampler* s, const float* h_h, const int32_t* h_timesteps, int32_t layer, int32_t first_stage,
                           int32_t stage, void* stream) {
    if (!s || !s->finalized || !s->cond_set) return fail(DC_ERR_INVALID, "sampler not ready (finalize + set_conditioning first)");
    if (!h_h || !h_timesteps) return fail(DC_ERR_INVALID, "null pointer argument");
    if (s->guided) return fail(DC_ERR_INVALID, "the conditioning is guided (dc_sampler_set_conditioning_guided): the debug entry points run plain conditionings");
    if (s->takes > 1) return fail(DC_ERR_INVALID, "the conditioning holds %d takes per music (dc_sampler_set_conditioning_takes): the debug entry points run plain conditionings", s->takes);
    if (s->win_W > 0) return fail(DC_ERR_INVALID, "the conditioning holds the windows of longer pieces (dc_sampler_set_conditioning_windows): the debug entry points run plain conditionings");
    if (layer < 0 || layer >= s->cfg.num_layers || first_stage < 1 || stage > 3 || first_stage > stage)
        return fail(DC_ERR_INVALID, "layer / stage out of range (need 1 <= first_stage <= last_stage <= 3)");
    if (s->cfg.no_eff) return fail(DC_ERR_UNSUPPORTED, "dc_sampler_debug_layer covers the linear-attention layers");
    HIP_TRY(hipSetDevice(s->cfg.device));
    // row-major [M][128] -> residual-stream image [G][tile][quarter][64 lanes][4] (dc_kernels.hip load_h)
    const size_t G = (size_t)s->G;
    std::vector<float> img(G * 4 * 4 * 64 * 4, 0.f);
    for (size_t g = 0; g < G; ++g)
        for (int t = 0; t < 4; ++t)
            for (int q = 0; q < 4; ++q)
                for (int l = 0; l < 64; ++l)
                    for (int i = 0; i < 4; ++i) {
                        const size_t tok = g * 32 + (l & 31);             // token space: clip stride s->T; h_h rows: [B][Tx]
                        const size_t bb = tok / s->T, nn = tok % s->T;
                        const int f = 32 * t + tile_row(4 * q + i, l >> 5);
                        if (tok < (size_t)s->M && nn < (size_t)s->Tx)
                            img[(((g * 4 + t) * 4 + q) * 64 + l) * 4 + i] = h_h[(bb * s->Tx + nn) * DC_D + f];
                    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(s->d_h, img.data(), img.size() * 4, hipMemcpyHostToDevice));
    // (x is not read on this path; out_mode is never reached)
    return denoise(s, s->d_x, h_timesteps, s->d_x, stream, Hooks{layer + 1, stage | ((first_stage - 1) << 16), layer});
}

int dc_sampler_debug_read(dc_sampler* s, const char* what, void* h_out, int64_t nbytes) {
    if (!s || !what || !h_out) return fail(DC_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(s->cfg.device));
    HIP_TRY(hipDeviceSynchronize());
    const std::string w(what);
    const size_t g = (size_t)s->G;
    const void* src = nullptr;
    size_t have = 0;
    if (w == "h") { src = s->d_h; have = g * 4 * 64 * 64; }
    else if (w == "pp") { src = s->d_pp; have = g * 32 * 64 * 32; }
    else if (w == "s_hi") { src = s->d_s_hi; have = g * 32 * 64 * 16; }
    else if (w == "s_lo") { src = s->d_s_lo; have = g * 32 * 64 * 16; }
    else if (w == "E") { src = s->d_E; have = g * s->NT * 64 * 32; }
    else if (w == "recs") { src = s->d_recs; have = g * 2 * DC_REC_FLOATS * 4; }
    else if (w == "a_sa") { src = s->d_a_sa; have = (size_t)s->B * 16 * 1024; }
    else if (w == "a_ca") { src = s->d_a_ca; have = (size_t)s->cfg.num_layers * s->B * 16 * 1024; }
    else if (w == "a_ca16") {          // filled for the 16-token layer kernel only: non-split formats, linear attention
        if (s->split_small || s->cfg.no_eff) return fail(DC_ERR_INVALID, "buffer 'a_ca16' not filled: this sampler never runs the 16-token layer kernel");
        src = s->d_a_ca16; have = (size_t)s->cfg.num_layers * s->B * 8 * 1024;
    }
    else if (w == "stamps") { src = s->d_stamps; have = (8 * 32 + 8 + 1024 + 1024 + 256 + 8 + 512) * 8; }
    else if (w == "temb") { src = s->h_model.temb; have = (size_t)s->cfg.max_timesteps * 512 * 4; }
    else if (w == "full_moves") {      // diagnostic builds only: {visits, moves} of the no_eff key loop's reference point, reset by the read
        if (nbytes != 16) return fail(DC_ERR_INVALID, "full_moves is 16 bytes");
        if (dc_full_moves_read((unsigned long long*)h_out, true) != hipSuccess) return fail(DC_ERR_UNSUPPORTED, "not a -DDC_DIAG_FULL_MOVES build");
        return DC_OK;
    }
    else return fail(DC_ERR_INVALID, "unknown debug buffer '%s'", what);
    if (!src) return fail(DC_ERR_INVALID, "buffer '%s' not allocated yet", what);
    if ((size_t)nbytes > have) return fail(DC_ERR_INVALID, "buffer '%s' holds %zu bytes, asked for %lld", what, have, (long long)nbytes);
    HIP_TRY(hipMemcpy(h_out, src, (size_t)nbytes, hipMemcpyDeviceToHost));
    return DC_OK;
}

int32_t dc_sampler_clip_stride(const dc_sampler* s) { return s ? s->T : 0; }

const char* dc_kernel_name(int32_t id) { return (id >= 0 && id < K_COUNT) ? kKernelNames[id] : ""; }
int32_t dc_kernel_count(void) { return K_COUNT; }
int64_t dc_sampler_workspace_bytes(const dc_sampler* s) { return s ? s->ws_bytes + (int64_t)s->arena_bytes : 0; }

}  // extern "C"
