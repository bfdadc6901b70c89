/*
 * dc_ddim.h - C ABI of libdc_ddim.so: the MI355X (gfx950) DDIM sampler of
 * Diffusion-Conductor's Diffusion_Stage.
 *
 * The reference has no FFI layer: its boundary is three Python call surfaces
 * (SURVEY.md section 8b).  These entry points are what a binding for that path binds
 * *below* those surfaces; each one names the reference code it replaces (paths
 * relative to Diffusion_Stage/).  Plain pointers and sizes only, no torch types.
 *
 * Conventions
 *   - every function returns DC_OK (0) or a negative dc_status; dc_last_error() gives
 *     the message of the last failure on the calling thread;
 *   - `d_` arguments are DEVICE pointers (caller-owned, e.g. tensor.data_ptr());
 *     `h_` arguments are HOST pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Work is
 *     ordered after everything already enqueued on `stream` and later work on `stream`
 *     is ordered after it; calls are asynchronous unless stated otherwise;
 *   - a dc_sampler is not thread-safe; use one per host thread / per GPU;
 *   - there is NO CPU fallback anywhere in this library.
 */
#ifndef DC_DDIM_H
#define DC_DDIM_H

#include <stdint.h>

/* The library is built with -fvisibility=hidden: these entry points are its whole dynamic symbol table
 * (tests/test_host_logic.py compares `nm -D` with this header). */
#define DC_EXPORT __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dc_sampler dc_sampler;

typedef enum dc_status {
    DC_OK = 0,
    DC_ERR_INVALID = -1,      /* bad argument / wrong call order          */
    DC_ERR_NO_DEVICE = -2,    /* no HIP device visible                    */
    DC_ERR_HIP = -3,          /* a HIP runtime call failed                */
    DC_ERR_PARAM = -4,        /* unknown / missing / mis-sized parameter  */
    DC_ERR_UNSUPPORTED = -5   /* configuration outside the built path     */
} dc_status;

/* MFMA operand precision of the denoiser (accumulation is always fp32; LayerNorm, softmax, SiLU/GELU,
 * FiLM and the DDIM update are fp32).  f16 and bf16 MFMA run at the same rate on gfx950; "split" means
 * x = hi + lo and three MFMAs per product (hi*hi + lo*hi + hi*lo), ~fp32 accurate.  In every mode the
 * two tiny pose projections (joint_embed 26->128, out 128->26) run split, and the one-time
 * cross-attention pre-pass runs split-bf16.  Measured rel-L2 on x0, DDIM-50: see DESIGN.md. */
typedef enum dc_precision {
    DC_PREC_BF16 = 0,   /* every GEMM plain bf16; meets the 1e-3 bound through its precise tail (below) */
    DC_PREC_MIXED = 1,  /* 128-wide GEMMs (Q/K/V, attention, out-proj, FFN) split-bf16; FiLM GEMM f16 */
    DC_PREC_BF16X3 = 2, /* split-bf16 everywhere (validation mode)                                   */
    DC_PREC_FP16 = 3    /* default: every GEMM plain f16, one MFMA per product                       */
} dc_precision;

/* Mirrors the constructor arguments the sampler path consumes:
 * MotionTransformer.__init__ (models/transformer.py:360-374) and
 * tools/visualization.py:169-178 (build_models). */
typedef struct dc_config {
    int32_t input_feats;   /* 26  (dim_pose, 13 joints x 2)            */
    int32_t num_frames;    /* 1800 rows of sequence_embedding          */
    int32_t latent_dim;    /* 128 (only value the reference supports)  */
    int32_t ff_size;       /* 64                                       */
    int32_t num_layers;    /* 8                                        */
    int32_t num_heads;     /* 8                                        */
    int32_t no_eff;        /* 0 = linear attention (default), 1 = full T x T attention (DC_PREC_FP16 only: bf16 attention operands are outside the parity bound) */
    int32_t precision;     /* dc_precision                             */
    int32_t max_timesteps; /* size of the timestep-embedding table (>= diffusion_steps), e.g. 1000 */
    int32_t device;        /* HIP device ordinal                       */
} dc_config;

DC_EXPORT const char* dc_last_error(void);
DC_EXPORT const char* dc_version(void);

/* ------------------------------------------------------------------------------------
 * Host-only helpers (no GPU needed; usable and tested on a CPU-only box).
 * ---------------------------------------------------------------------------------- */

/* get_named_beta_schedule('linear', n) (models/gaussian_diffusion.py:228-245) and the
 * tables GaussianDiffusion.__init__ derives from it (:342-361), all fp64, each [n]. */
DC_EXPORT int dc_linear_beta_schedule(int32_t num_steps, double* h_betas, double* h_alphas_cumprod,
                            double* h_alphas_cumprod_prev, double* h_sqrt_recip_alphas_cumprod,
                            double* h_sqrt_recipm1_alphas_cumprod);

/* The four fp32 scalars ddim_sample (models/gaussian_diffusion.py:812-830) uses at
 * timestep t with eta = 0, from fp64 alphas_cumprod[n]:
 *   h_coef[t*4 + 0] = (float)sqrt(1/abar_t)            (sqrt_recip_alphas_cumprod)
 *   h_coef[t*4 + 1] = (float)sqrt(1/abar_t - 1)        (sqrt_recipm1_alphas_cumprod)
 *   h_coef[t*4 + 2] = sqrtf((float)abar_{t-1})         (coefficient of pred_xstart)
 *   h_coef[t*4 + 3] = sqrtf(1 - (float)abar_{t-1})     (coefficient of eps)          */
DC_EXPORT int dc_ddim_coefficients(int32_t num_steps, const double* h_alphas_cumprod, float* h_coef);

/* The same for any eta >= 0 (models/gaussian_diffusion.py:814-826), eight floats per timestep, fp32 arithmetic on the
 * fp32-rounded table entries in the reference's own order:
 *   h_coef8[t*8 + 0..2] as above;  sigma = eta sqrt((1-abar_{t-1})/(1-abar_t)) sqrt(1-abar_t/abar_{t-1})
 *   h_coef8[t*8 + 3] = sqrtf(1 - abar_{t-1} - sigma^2)   (coefficient of eps)
 *   h_coef8[t*8 + 4] = sigma                             (coefficient of the noise draw; 0 at t = 0 = the reference's nonzero_mask)
 *   h_coef8[t*8 + 5..7] = 0 */
DC_EXPORT int dc_ddim_coefficients_ex(int32_t num_steps, const double* h_alphas_cumprod, float eta, float* h_coef8);

/* The table of a loop that samples AROUND KNOWN VALUES (dc_sampler_set_known): dc_ddim_coefficients_ex's row, plus the noise levels
 * the known elements are held at -
 *   h_coef8[t*8 + 0..4] as dc_ddim_coefficients_ex, bit for bit
 *   h_coef8[t*8 + 5] = sqrtf(1 - (float)abar_{t-1})    (dc_ddim_coefficients' column 3; exactly 0 at t = 0, where slot 2 is exactly 1)
 *   h_coef8[t*8 + 6] = sqrtf((float)abar_t),  h_coef8[t*8 + 7] = sqrtf(1 - (float)abar_t)
 * h_start2 (may be NULL) receives the level at which the loop of num_steps steps starts, sqrt(abar_{S-1}) and sqrt(1 - abar_{S-1})
 * (slots 6, 7 of the last row: the library blends x_T with them).  A loop without known values reads slots 0..4 only: the table
 * serves it as well. */
DC_EXPORT int dc_ddim_coefficients_known(int32_t num_steps, const double* h_alphas_cumprod, float eta, float* h_coef8, float* h_start2);

/* Sampling on a SUB-SEQUENCE of the checkpoint's timesteps, first or second order.  The reference has neither: its ddim_sample_loop
 * walks every timestep of the schedule it was built with (models/gaussian_diffusion.py:943), and its only deterministic update is the
 * first-order one of ddim_sample (:812-830).  h_timesteps int32 [n]: strictly decreasing, inside [0, n_train) - the numbers the model
 * sees; h_alphas_cumprod fp64 [n_train] of the TRAINING schedule.  With a_i = abar[t_i] and a'_i = abar[t_{i+1}] (a'_{n-1} = 1: the
 * last step lands on the clean sample), row i - DC_SOLVER_ROW floats, indexed by ITERATION - holds
 *   h_rows[i][0..7]  dc_ddim_coefficients_known's slots with (abar_t, abar_{t-1}) replaced by (a_i, a'_i): the same fp32 roundings in
 *                    the same order (one routine computes both), so h_timesteps = n_train-1 .. 0 gives that table's rows, reversed, bit
 *                    for bit: the first-order update (:812-830) on the sub-schedule, what improved-diffusion calls SpacedDiffusion
 *   h_rows[i][8]     kappa_i, the history coefficient of the second-order multistep update (DPM-Solver++ 2M, x0-prediction form):
 *                      x_{i+1} = [first-order update] + kappa_i (x0_i - x0_{i-1}),     x0_i = the step's predicted x0;
 *                      lambda(a) = 1/2 ln(a / (1 - a)),  h_i = lambda(a'_i) - lambda(a_i),  r_i = h_{i-1} / h_i,
 *                      kappa_i = ( sqrt(a'_i) - sqrt(1 - a'_i) sqrt(a_i) / sqrt(1 - a_i) ) / (2 r_i)      (fp64, rounded once)
 *                    nonzero only for order == 2 and 0 < i < n-1: the first step has no history, the last one is first order, so the
 *                    final sample stays the model's own x0
 *   h_rows[i][9..]   0
 * h_start2 (may be NULL): sqrt(a_0), sqrt(1 - a_0), the level a loop around known values starts at.
 * DC_ERR_INVALID: order outside {1, 2}; order 2 with eta != 0 (the multistep update is deterministic); n < 1; a list that is not
 * strictly decreasing or leaves [0, n_train).  Host only. */
#define DC_SOLVER_ROW 12
DC_EXPORT int dc_solver_table(int32_t n_train, const double* h_alphas_cumprod, const int32_t* h_timesteps, int32_t n, float eta,
                              int32_t order, float* h_rows, float* h_start2);

/* Test hook: pack a row-major Linear weight W[n_out][k_in] (torch layout) into the
 * MFMA fragment-major bf16 image the kernels read (see DESIGN.md "weight image").
 * `chained` != 0 uses the accumulator-as-operand k order, 0 the natural k order.
 * h_hi / h_lo receive ceil(n_out/32)*ceil(k_in/32)*2*64*8 uint16 (bf16 bits) each. */
DC_EXPORT int dc_pack_weight(const float* h_w, int32_t n_out, int32_t k_in, int32_t chained,
                   uint16_t* h_hi, uint16_t* h_lo);

/* ------------------------------------------------------------------------------------
 * Sampler object
 * ---------------------------------------------------------------------------------- */

/* Replaces constructing MotionTransformer (models/transformer.py:360-445) +
 * GaussianDiffusion (models/gaussian_diffusion.py:328-379) for sampling. */
DC_EXPORT int dc_sampler_create(const dc_config* cfg, dc_sampler** out);
DC_EXPORT void dc_sampler_destroy(dc_sampler* s);

/* Replaces nn.Module.load_state_dict for the entries of state['encoder']
 * (trainers/ddpm_trainer.py:303-319): call once per float tensor with the reference's
 * own key (e.g. "temporal_decoder_blocks.3.sa_block.query.weight") and its contiguous
 * fp32 data, then dc_sampler_finalize_params.  Unknown keys -> DC_ERR_PARAM. */
DC_EXPORT int dc_sampler_set_param(dc_sampler* s, const char* name, const float* h_data, int64_t numel);

/* Packs all parameters into the device weight image and builds the
 * timestep_embedding + time_embed table (models/transformer.py:8-25, 410-414, 482).
 * Missing entries -> DC_ERR_PARAM.  Synchronous. */
DC_EXPORT int dc_sampler_finalize_params(dc_sampler* s);

/* Step-invariant part of MotionTransformer.forward (models/transformer.py:479-482 and
 * the K/V/attention half of LinearTemporalCrossAttention.forward :149-155): applies
 * `linear` to xf_proj / xf_out, and builds the per-clip cross-attention matrices for
 * all layers.  d_xf_proj, d_xf_out: fp32 [B, T, 64] (the pair encode_music returns);
 * h_length: int32 [B] (model_kwargs['length'], 1 <= length <= T), NULL = all T.  1 <= T <= min(num_frames, 4032); full attention
 * (`no_eff`) needs T >= 32 (DC_ERR_UNSUPPORTED below that).
 * Must be called before dc_sampler_denoise / dc_sampler_ddim_loop; (re)allocates the
 * workspace for (B, T). */
DC_EXPORT int dc_sampler_set_conditioning(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out,
                                const int32_t* h_length, int32_t B, int32_t T, void* stream);

/* MotionTransformer.encode_music in eval mode (models/transformer.py:447-459) with the MusicEncoder conv stack
 * (:289-340) as MFMA kernels: d_mel fp32 [B, Tm, n_mels=128] (the tensor generate_music_motion builds at
 * trainers/ddpm_trainer.py:186-189) -> d_xf_out = music_encoder(mel) and d_xf_proj = proj(d_xf_out), both fp32
 * [B, (Tm-1)/3+1, 64], caller-allocated; Tm >= 4 (the reference's reflection padding raises below that).  Needs the `music_encoder.*` and `proj.*` state_dict entries
 * (optional as a group in dc_sampler_set_param; DC_ERR_PARAM here when they were not supplied). */
DC_EXPORT int dc_sampler_encode_music(dc_sampler* s, const float* d_mel, int32_t B, int32_t Tm, int32_t n_mels,
                            float* d_xf_proj, float* d_xf_out, void* stream);

/* Activation format of the MusicEncoder kernels (no counterpart in the reference, whose encoder is fp32 PyTorch):
 *   DC_ME_SPLIT (0): two bf16 planes per activation and three MFMAs per product - 6e-6 relative at the encoder's output;
 *   DC_ME_FP16  (1): one fp16 plane, one MFMA per product, half the bytes - 3.7e-4 at the encoder's output (every activation is
 *                    rounded to 11 bits once per layer), 1.3e-4 of x0 after DDIM-50, about half the time (2.1 vs 4.2 ms per 32 clips).
 * Default: DC_ME_FP16 for the precisions whose denoiser rounds these features to 16-bit operands anyway (DC_PREC_FP16, DC_PREC_BF16),
 * DC_ME_SPLIT for the split-operand precisions.  The environment variable DC_ME_PREC=f16|split (read per call) overrides both. */
/* Precise tail of the sampling loops (DC_PREC_FP16, DC_PREC_BF16; no counterpart in the reference, which computes in fp32): the last
 * `steps` model evaluations of a loop run their 128-wide GEMMs on SPLIT operands (hi + lo halves of the same 16-bit weight images, three
 * MFMAs per product) instead of plain ones.  What a 16-bit mode loses against the reference is almost entirely the WEIGHTS' rounding
 * in the final evaluations (DDIM's last step returns the model's own prediction of x0).  Golden DDIM-50, rel-L2 of x0:
 *   fp16:  5.0e-4 with steps = 0,  2.3e-4 with 1,  1.6e-4 with 2,  1.2e-4 with 4   (+0.45 % of the loop per step at bs = 32)
 *   bf16:  3.1e-3 with steps = 0,  9.5e-4 with 2,  6.8e-4 with 4,  5.4e-4 with 8   - the bf16-operand mode that meets the 1e-3 bound
 *          (round 5's figures, the tail's FiLM GEMM on bf16 operands).  Since round 6 the bf16 precision's split evaluations take the FiLM
 *          GEMM's operands in fp16 - they are "mixed"-precision evaluations: 1.42e-3 with 1, 8.5e-4 with 2, 5.6e-4 with 4, 3.5e-4 with 8;
 *          default 6 (4 left 1.1e-3 on one short ragged batch of tools/fuzz_shapes.py, 6: 8.6e-4, 8: 7.3e-4)
 * Default (steps never set): 1 for fp16, 6 for bf16 (dc_precise_tail_default).  (Clip strides of whole 32-frame groups run the split evaluations in the
 * workgroup-record form on clip-aligned units, others - T = 900 x 128 unpadded, short clips - in the per-group record form: 5.2e-4 ->
 * 2.6e-4 there at no measurable cost.)  Loops of an EPSILON model (DC_UPDATE_EPSILON) run EVERY evaluation on split operands unless a
 * number was set here: their final sample carries what the plain evaluations left in x_t (fp16, eta = 0: 1.4 - 1.8e-3 with any shorter
 * tail, 1.5e-4 all split; with full attention such a loop is REFUSED at eta = 0 - DC_ERR_UNSUPPORTED: 2.3e-4 ... 1.26e-3 over randomized loops even
 * with every GEMM split, the attention's scores, weights and values being plain fp16 - and runs at eta > 0, <= 2e-4), and so do loops of the bf16 precision over clips of fewer than 100 frames (a clip's error is then a norm over
 * few numbers and the worst clip of a batch of dozens reached 1.27e-3 with the default tail: 39 clips of 36 frames, tools/fuzz_shapes.py;
 * such loops are launch-bound, the split form costs them little).  Applies to linear and full attention alike (`no_eff`, fp16: its split instantiation keeps scores, weights and
 * values plain 16-bit); ignored for the split precisions.  DC_PRECISE_TAIL=k in the environment
 * overrides it.  (In a loop that has a tail the plain
 * evaluations read FiLM scale tiles that hold G' itself - one mixed-precision FMA per element instead of two -, the split ones G' - 1;
 * loops without a tail keep G' - 1 everywhere.) */
DC_EXPORT int dc_sampler_set_precise_tail(dc_sampler* s, int32_t steps);      /* steps = -1: back to the precision's default */
DC_EXPORT int32_t dc_precise_tail_default(int32_t precision);                    /* DC_PREC_FP16: 1, DC_PREC_BF16: see above, others 0 */

/* dc_sampler_denoise (MotionTransformer.forward, transformer.py:469-497) on split operands - the precise tail's evaluation form - when
 * on != 0; default off (plain operands of the precision).  For callers that step a sampler THROUGH single evaluations and whose update
 * keeps the evaluations' error (an EPSILON or PREVIOUS_X model, cond_fn: gaussian_diffusion.py:510-520, 581-603): the Python sampler
 * switches it on for exactly those loops.  The bf16 precision's split evaluations also take their FiLM GEMM operands in fp16 (they are
 * then the evaluations of the "mixed" precision).  Ignored for the split precisions (already split). */
DC_EXPORT int dc_sampler_set_precise_forward(dc_sampler* s, int32_t on);

#define DC_ME_SPLIT 0
#define DC_ME_FP16 1
DC_EXPORT int dc_sampler_set_encoder_format(dc_sampler* s, int32_t format);

/* One MotionTransformer.forward (models/transformer.py:469-497) on the conditioning set
 * above: d_x fp32 [B, T, input_feats], h_timesteps int32 [B] -> d_out fp32 [B, T, input_feats]. */
DC_EXPORT int dc_sampler_denoise(dc_sampler* s, const float* d_x, const int32_t* h_timesteps,
                       float* d_out, void* stream);

/* GaussianDiffusion.ddim_sample_loop (models/gaussian_diffusion.py:871-965) with
 * model_mean_type=START_X, clip_denoised=False, eta=0, cond_fn=denoised_fn=None, as
 * DDPMTrainer.generate_music_motion calls it (trainers/ddpm_trainer.py:190-200).
 *   d_noise  fp32 [B,T,P]  x_T (the `noise=` argument; the caller draws it)
 *   d_out    fp32 [B,T,P]  final sample (== pred_xstart of the last step)
 *   num_steps              diffusion_steps S; timesteps run S-1 .. 0
 *   h_coef   fp32 [S,4]    per-timestep scalars, see dc_ddim_coefficients
 *   h_snap_iters int32[n_snap], d_snaps fp32 [n_snap,B,T,P]: `idxs` - the sample after
 *                          iteration i (0 = after the first step) is also stored; may be NULL/0.
 * The step sequence is captured once into a hipGraph per (B,T,S) and replayed. */
DC_EXPORT int dc_sampler_ddim_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t num_steps,
                         const float* h_coef, const int32_t* h_snap_iters, int32_t n_snap,
                         float* d_snaps, void* stream);

/* The same loop with the other branches of the reference's sampler on the device (replaces the rest of p_mean_variance /
 * ddim_sample, models/gaussian_diffusion.py:503-521, 812-830; ddim_sample_loop's own default is clip_denoised=True, :876):
 *   h_coef8  fp32 [S,8]    per-timestep scalars from dc_ddim_coefficients_ex (eta folded in: sigma, sqrt(1-abar_prev-sigma^2))
 *   flags                  DC_UPDATE_CLIP_DENOISED: pred_xstart.clamp(-1, 1) (:506-507);
 *                          DC_UPDATE_EPSILON: the denoiser predicts epsilon, pred_xstart = sqrt(1/abar) x_t - sqrt(1/abar-1) out
 *                          (ModelMeanType.EPSILON, :516-521, 539-544)
 *   d_step_noise fp32 [S,B,T,P]  the draws the reference takes with th.randn_like(x) at iteration i = 0 .. S-1 (:822); used when
 *                          any sigma != 0 (eta > 0), ignored (may be NULL) otherwise.  NULL with sigma != 0: the library generates
 *                          the draws step by step (dc_sampler_set_step_noise_seed must have been called).  The tensor's address is
 *                          read through a device slot: another tensor on the next call does not re-capture the hipGraph.
 * Everything else as dc_sampler_ddim_loop; flags = 0 with an eta = 0 table is that call.  denoised_fn / cond_fn are host
 * callbacks and stay on the caller's side of the ABI (per-step dc_sampler_denoise). */
#define DC_UPDATE_CLIP_DENOISED 1
#define DC_UPDATE_EPSILON 2
DC_EXPORT int dc_sampler_ddim_loop_ex(dc_sampler* s, const float* d_noise, float* d_out, int32_t num_steps, const float* h_coef8,
                            int32_t flags, const float* d_step_noise, const int32_t* h_snap_iters, int32_t n_snap,
                            float* d_snaps, void* stream);

/* dc_sampler_ddim_loop_ex on the caller's timesteps and rows (dc_solver_table; no counterpart in the reference, see there):
 * iteration i evaluates the model at h_timesteps[i] and updates with h_rows[i] - every per-step table of the loop is indexed by
 * iteration, the timestep only selects the model's embedding.  n <= max_timesteps, every timestep < max_timesteps, strictly
 * decreasing (DC_ERR_INVALID otherwise, before anything is enqueued).  Rows with a history coefficient (slot 8) run the second-order
 * multistep update: the previous step's predicted x0 - after guidance, the EPSILON conversion and clipping - is kept in one more
 * [B,T,P] fp32 buffer of the workspace, zeroed when the loop starts, read and rewritten in place by the update in the last layer's
 * kernels, and carried across the graph replays of a long loop; the history term is added before known values are replaced.  Such rows need
 * sigma = 0.  d_step_noise is [n,B,T,P]; snapshot iterations count iterations of this loop.  Known values, guidance, smoothing, the
 * precise tail and DC_DISABLE_GRAPH apply as in dc_sampler_ddim_loop_ex; the hipGraph is keyed by (B, T, n, form) - another list of
 * the same length replays it.  dc_sampler_solver_profile_loop is dc_sampler_profile_loop for such a loop. */
DC_EXPORT int dc_sampler_solver_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t n, const int32_t* h_timesteps,
                                     const float* h_rows, int32_t flags, const float* d_step_noise, const int32_t* h_snap_iters,
                                     int32_t n_snap, float* d_snaps, void* stream);
DC_EXPORT int dc_sampler_solver_profile_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t n, const int32_t* h_timesteps,
                                             const float* h_rows, int32_t flags, float* h_ms, int32_t* h_count, int32_t n_kernels,
                                             void* stream);

/* Sampling around known values (no counterpart in the reference's DDIM loop; its ancestral p_sample has a pre_seq hook,
 * gaussian_diffusion.py:634-646, with fresh noise per step - not this).  d_known, d_mask, d_known_noise: fp32 [B,T,P] each, for the
 * (B, T) of the last dc_sampler_set_conditioning.  An element whose mask is nonzero is KNOWN: at every noise level abar the loops hold it at
 *   x = sqrt(abar) known + sqrt(1 - abar) known_noise
 * - x_T at abar_{S-1} before the first evaluation (the library blends it; d_noise is not written), every x_{t-1} a step writes at
 * abar_{t-1}, snapshots included.  ONE fixed draw per element puts the known region on a deterministic DDIM trajectory; at t = 0,
 * abar_prev = 1 and the final sample equals d_known bit for bit there (before smoothing, which runs after the replacement).  eta > 0
 * noise, clipping and the EPSILON parameterisation act on the unknown elements only; DC_STATUS_NONFINITE still reports on the model's
 * prediction of every element.  An all-zero mask gives the bits of a loop without known values.  The loops then need the table of
 * dc_ddim_coefficients_known (DC_ERR_INVALID with any other).  The tensors are read while a loop runs and their addresses go through
 * device slots: other tensors on the next call do not re-capture the hipGraph.  The setting serves the following loops until it is
 * cleared - three NULLs - or dc_sampler_set_conditioning / _guided / _takes changes the caller's (B, T) or its takes count, or switches
 * guidance on or off (the tensors belong to the conditioning they were set on).  DC_ERR_INVALID: a mask without values, a mask without noise,
 * values or noise without a mask. */
DC_EXPORT int dc_sampler_set_known(dc_sampler* s, const float* d_known, const float* d_mask, const float* d_known_noise);

/* Classifier-free guidance.  The reference trains its denoiser for it - MotionTransformer.encode_music (models/transformer.py:389,
 * 451-459) zeroes the music features of a token with probability cond_mask_prob = 0.1 before `proj` - and has NO sampling
 * counterpart: its samplers never evaluate the unconditional branch.  This call is dc_sampler_set_conditioning for a guided loop: the
 * sampler then evaluates 2 B internal clips per step - clip b with the caller's xf_proj[b], xf_out[b], length[b], clip B + b its
 * unconditional shadow, every frame carrying the null pair (h_null_proj[64], h_null_out[64]; host arrays) and length[b] - both on the
 * same x_t[b], and combines the two model outputs before anything else of the update, in fp32 and in this order:
 *   out = c + (w - 1) (c - u)          c conditional, u unconditional output, w the guidance scale
 * followed by the update of dc_sampler_ddim_loop_ex (START_X or EPSILON, clipping, eta noise) and the replacement of known values,
 * unchanged.  w = 1 returns c bit for bit whenever u is finite.  DC_STATUS_NONFINITE looks at c, u and the combined prediction.
 * The null pair of the reference's masking taken to every token is null_out = 0 and null_proj = proj.bias (proj(0)).
 * Everything the caller passes to the loops and to dc_sampler_set_known stays [B,T,P] (d_noise, d_out, snapshots, step noise, seeded
 * step noise and its first_element); the workspace is sized for 2 B.  dc_sampler_ddim_loop, _ex and dc_sampler_profile_loop run guided
 * whenever the conditioning is guided; dc_sampler_denoise and the debug entry points return DC_ERR_INVALID on it (per-clip timesteps
 * break the unconditional half's shared FiLM column; step-through callers combine on their side).  A plain
 * dc_sampler_set_conditioning switches guidance off again.  DC_ERR_INVALID: NULL null vectors. */
DC_EXPORT int dc_sampler_set_conditioning_guided(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length,
                                       int32_t B, int32_t T, const float* h_null_proj, const float* h_null_out, void* stream);

/* Several TAKES per music (no counterpart in the reference, whose sampler draws one motion per music and call:
 * trainers/ddpm_trainer.py:186-200).  dc_sampler_set_conditioning for `takes` >= 1 samples of each of B musics (d_xf_proj, d_xf_out
 * [B,T,64], h_length[B] as there): the sampler then runs takes * B clips, TAKE-MAJOR - caller clip j * B + b is take j of music b, with
 * music b's features and length.  Everything the caller hands to the loops and to dc_sampler_set_known is [takes * B, T, P] in that
 * order: d_noise, d_out, snapshots, step noise, seeded step noise and its first_element, the known tensors.  The takes of one music differ
 * through their noise alone.  What they share is the conditioning: a loop step has one timestep, so the FiLM scale / shift tiles of take
 * j are those of take 0 bit for bit, and where one take is a whole number Gc = B T' / 32 of 32-token groups (T' the clip stride,
 * dc_sampler_clip_stride) the step's FiLM GEMM computes one take's groups and token group g reads the tiles of group g mod Gc - a
 * `takes`-th of the loop's largest kernel.  Elsewhere (B T' no multiple of 32, Gc = 1 - one clip of at most 32 frames -, DC_PREC_BF16X3,
 * DC_TAKES_FULL_FILM=1 in the environment) the GEMM covers every group.  Either way the result equals, bit for bit, dc_sampler_set_conditioning on the features tiled `takes`
 * times.  The one-time pre-pass runs over all takes * B clips.
 * h_null_proj, h_null_out: both NULL - unguided; both given - guided as dc_sampler_set_conditioning_guided, 2 * takes * B internal clips,
 * the conditional clips first, then their shadows (which share one null column as there); exactly one NULL: DC_ERR_INVALID.
 * takes = 1 is dc_sampler_set_conditioning / dc_sampler_set_conditioning_guided, bit for bit.  A plain dc_sampler_set_conditioning
 * switches takes off.  dc_sampler_denoise and the debug entry points return DC_ERR_INVALID on a conditioning with takes > 1 (their
 * per-clip timesteps break the sharing).  Known values belong to the (B, T, guided, takes) they were set on.  The captured hipGraph is
 * keyed by the wrap period as well: 2 takes of 2 musics and a plain conditioning of 4 clips never replay each other's graph.
 * DC_ERR_INVALID: takes < 1. */
DC_EXPORT int dc_sampler_set_conditioning_takes(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length,
                                                int32_t B, int32_t T, int32_t takes, const float* h_null_proj, const float* h_null_out,
                                                void* stream);

/* Overlapping WINDOWS of a longer piece in ONE loop, blended at every step (no counterpart in the reference, which samples one window;
 * the scheme is MultiDiffusion's).  A piece has L frames and is covered by W windows of T frames at ascending starts
 * s_0 = 0 < ... < s_{W-1} = L - T, without gaps (s_{k+1} <= s_k + T) and with at most 4 windows over a frame.  The loop's state is ONE
 * tensor in piece space, x [B, L, P].  At every step
 *   1. window k's frames are rows [s_k, s_k + T) of x: overlapping windows read the same x_t;
 *   2. the model is evaluated on the W B windows, window-major - internal clip k B + b is window k of piece b, with its own music
 *      features (d_xf_proj, d_xf_out: fp32 [W B, T, 64] in that order) - and the last layer stores the raw output;
 *   3. for every piece element,  out = sum_k w[k][f - s_k] raw_k[f - s_k]  over the windows that cover frame f, in ascending k: fp32,
 *      no contraction, the accumulator starting from the first product, w = h_weight, fp32 [W][T];
 *   4. the update of dc_sampler_ddim_loop_ex / dc_sampler_solver_loop and the replacement of known values are applied to `out`
 *      exactly as a guided loop applies them: eta noise, clipping, EPSILON, the multistep term, snapshots, DC_STATUS_NONFINITE;
 *      noise, step noise, known values, the multistep history and snapshots are all [B, L, P];
 *   5. x_{t-1} is written to piece space and to every covering window's slot of the internal x.
 * With the null pair given the conditioning is guided as dc_sampler_set_conditioning_guided: the conditional and the unconditional raw
 * outputs are blended each (step 3), combined as c + (w - 1)(c - u), then updated; 2 W B internal clips.
 * The loop entry points then take and return [B, L, P] (d_noise, d_out, d_snaps, d_step_noise per iteration, seeded step noise, the
 * tensors of dc_sampler_set_known, smoothing runs over the L frames).  A frame under one window, whose weight is then exactly 1, takes
 * that window's output bit for bit: W = 1 (L = T), and windows that do not overlap, give the bits of the plain loop on those clips
 * in the same launch form.  Starts and weights reach the kernels through device tables: another plan of the same (B, W, T, L) replays
 * the captured hipGraph.  dc_sampler_denoise and the debug entry points return DC_ERR_INVALID on such a conditioning; a plain
 * dc_sampler_set_conditioning switches windows off; known values belong to the (B, W, T, L) they were set on.  Windows do not combine
 * with takes.  Synchronous (the tables are host arrays).
 * DC_ERR_INVALID, on the host before anything is enqueued (dc_windows_check is that check alone, no sampler or GPU needed): starts that
 * are unordered or leave a gap, s_0 != 0, s_{W-1} != L - T, more than 4 windows over a frame, W > 65535, a weight that is negative or
 * not finite, weights over a frame that do not sum to 1 within 4 ulp of fp32 (summed in fp64), an h_length (windows are full: must be
 * NULL), exactly one vector of the null pair. */
DC_EXPORT int dc_sampler_set_conditioning_windows(dc_sampler* s, const float* d_xf_proj, const float* d_xf_out, const int32_t* h_length,
                                                  const int32_t* h_start, const float* h_weight, int32_t B, int32_t W, int32_t T, int32_t L,
                                                  const float* h_null_proj, const float* h_null_out, void* stream);
DC_EXPORT int dc_windows_check(const int32_t* h_start, const float* h_weight, int32_t W, int32_t T, int32_t L, const int32_t* h_length);

/* The guidance scale w of the loops on a guided conditioning (same reference lines: transformer.py:389,451-459 train for it, no sampling
 * counterpart).  1 after every dc_sampler_set_conditioning_guided.  Must be finite (DC_ERR_INVALID), and a guided conditioning must be
 * set.  The scale reaches the kernels through a device slot: another scale replays the same hipGraph. */
DC_EXPORT int dc_sampler_set_guidance_scale(dc_sampler* s, float w);

/* eta > 0 without a noise tensor.  After this call a dc_sampler_ddim_loop_ex with sigma != 0 and d_step_noise == NULL
 * generates the draws of each iteration itself at the head of the step that consumes them (one [B,T,P] buffer instead of the
 * [S,B,T,P] tensor: 6 GB at S = 1000, bs = 32): Philox4x32-10 keyed by `seed`, counter = (element, iteration), Box-Muller.
 * Draw (seed, iteration, element) does not depend on the batch layout or launch form.  The reference draws with
 * th.randn_like on its own device generator (:822), which no other implementation can reproduce - parity tests pass the
 * draws explicitly (d_step_noise); dc_step_noise_fill writes the library's draws of one iteration into a caller buffer
 * (n = B*T*P elements), so a [S,B,T,P] tensor that reproduces a seeded run can be assembled.
 * A seed serves ONE loop: the dc_sampler_ddim_loop_ex that uses it consumes it, and a later loop with sigma != 0, no tensor and no
 * new seed fails with DC_ERR_INVALID instead of replaying the same draws.
 * dc_sampler_set_step_noise_seed_at: the same for a sampler that holds clips [lo, hi) of a larger batch (one rank of a sharded
 * run, sharding.py): first_element = lo*T*P is the index of its first element in the whole batch's [B,T,P] draw, so that every
 * rank seeded alike draws exactly the rows the unsharded run (gaussian_diffusion.py:822: ONE th.randn_like over the batch) gives
 * its clips - never the same rows on every rank. */
DC_EXPORT int dc_sampler_set_step_noise_seed(dc_sampler* s, uint64_t seed);
DC_EXPORT int dc_sampler_set_step_noise_seed_at(dc_sampler* s, uint64_t seed, uint64_t first_element);
DC_EXPORT int dc_step_noise_fill(float* d_out, int64_t n, uint64_t seed, int32_t iteration, void* stream);

/* Numeric health of the sampler's LAST sampling loop (the word is reset when a loop starts), plus whatever a
 * dc_sampler_denoise since then added (no reference counterpart: the reference computes in fp32).  Waits for the sampler's
 * work, then returns the OR of
 *   DC_STATUS_NONFINITE    a predicted x0 (the denoiser's output) was inf or nan;
 *   DC_STATUS_F16_SATURATED  a FiLM modulation value (StylizationBlock scale / shift, transformer.py:74-78) left the fp16 range
 *                          in which every precision mode stores it: the checkpoint is outside what the library supports.
 *                          Sources: the range check in the epilogue of the split-path FiLM GEMM (bf16x3 / bf16 modes: the bit
 *                          can then appear without NONFINITE), and - in every mode, behind a NONFINITE report - a scan of the
 *                          FiLM tiles of every timestep of the last loop (the GEMM is re-run per timestep on this failure path).
 *                          NONFINITE without this bit in the fp16 mode means an fp16 OPERAND overflowed: use precision "mixed"
 *                          (bf16-range operands; Python: MotionTransformer(precision="auto") switches and re-runs by itself).
 *   DC_STATUS_TIMEOUT      small batches only (B * ceil(T / 64) <= CUs): a workgroup gave up waiting for the slices of its clip's attention
 *                          combine, which the clip's workgroups exchange inside a layer launch - they are co-resident by construction unless
 *                          the GPU is shared with other work; the wait is bounded (~0.1 s) and the loop's results are then invalid.
 *                          One timeout per loop at most: once the bit is set, the loop's remaining launches stop waiting.  Reading
 *                          the bit through dc_sampler_status LATCHES the form without the exchange on this sampler
 *                          (dc_sampler_set_combine_exchange(s, 0)), so re-running the loop gives a valid result; callers that share a
 *                          GPU, or run several small-batch samplers on streams of one process, should select that form up front.
 *                          DC_L16_OWN_COMBINE=1 in the environment selects it for every sampler of the process.
 * clear != 0 resets the word. */
#define DC_STATUS_NONFINITE 1
#define DC_STATUS_F16_SATURATED 2
#define DC_STATUS_TIMEOUT 4
DC_EXPORT int dc_sampler_status(dc_sampler* s, int32_t* h_status, int32_t clear);

/* Batch invariance (the reference's key softmax is per clip, transformer.py:111): on clip-aligned units - no workgroup's tokens span two
 * clips - a clip's result is bit-identical whatever the batch around it, and equal to sampling it alone in the same launch form.  Small
 * batches and the split-operand evaluations always run them.  The wide form (the chip full: bs = 32 x 1800) runs them by default
 * whenever they cost no extra round of workgroups over the chip (mode -1, the library's rule; +1.6 ... +2.1 % per loop at bs = 32 x 1800,
 * 256 instead of 228 workgroups); otherwise flat 256-token units, where a unit that contains a clip edge exponentiates both clips' keys
 * against one maximum and a clip depends on its neighbours at the rounding level (up to 4e-4, inside the parity bound).
 * mode 1: clip-aligned units always; 0: flat units (the throughput form); -1: the rule.  Needs a clip stride of whole 32-frame groups
 * (dc_sampler_clip_stride) and T >= 256; ignored otherwise. */
DC_EXPORT int dc_sampler_set_clip_aligned(dc_sampler* s, int32_t mode);

/* Clip-aligned units pad a clip to whole 256-token workgroups: at 1800 frames the eighth workgroup of a clip has one wave with tokens
 * and seven without.  on != 0 (default): in the wide plain layer kernel such a padding wave issues its shares of the weight-image copies,
 * takes part in the workgroup's combine, barriers and record tail, and does nothing else.  on == 0: it runs the whole layer on the clip's
 * last group, as it did before this setting existed - the comparison form.  Results are bit-identical either way (nothing a padding wave
 * computes reaches an output); a change re-captures the loop's graph.  No reference counterpart. */
DC_EXPORT int dc_sampler_set_idle_wave_path(dc_sampler* s, int32_t on);

/* Small batches (B * ceil(T / 64) <= CUs): on != 0 (default) lets a clip's workgroups share the combine of the attention unit records
 * inside a layer launch (-8 % per layer launch at one clip per call; needs the launch's workgroups co-resident, see DC_STATUS_TIMEOUT);
 * on == 0 makes every workgroup combine alone - no in-launch wait, safe beside other work on the GPU.  No reference counterpart
 * (the reference's attention is one einsum, transformer.py:113-116). */
DC_EXPORT int dc_sampler_set_combine_exchange(dc_sampler* s, int32_t on);

/* Timing hook for bench.py: device time (ms, HIP events on the library's own stream)
 * of the last dc_sampler_ddim_loop and the summed duration + launch count of its
 * dominant kernel are not observable from outside a graph, so the library can run the
 * same loop eagerly with per-kernel events.  Fills h_ms[kernel_id] with the total ms
 * and h_count[kernel_id] with launches for each kernel id < n (see dc_kernel_name). */
DC_EXPORT int dc_sampler_profile_loop(dc_sampler* s, const float* d_noise, float* d_out, int32_t num_steps,
                            const float* h_coef, float* h_ms, int32_t* h_count, int32_t n, void* stream);
DC_EXPORT const char* dc_kernel_name(int32_t kernel_id);
DC_EXPORT int32_t dc_kernel_count(void);

/* Test hooks (tests/ only).  dc_sampler_debug_denoise runs dc_sampler_denoise but stops after
 * `n_layers` decoder layers, the last one cut after stage 1 = self-attention, 2 = cross-attention,
 * 3 = FFN (0 = whole layer), leaving the residual stream in the internal buffer "h".
 * dc_sampler_debug_read copies an internal device buffer to the host (synchronous); names:
 * "h" "pp" "s_hi" "s_lo" "E" "recs" "a_sa" "a_ca" "a_ca16" "temb" (layouts: DESIGN.md; "a_ca16", the 16-token layer
 * kernel's copy of "a_ca", is filled for non-split formats with linear attention only: DC_ERR_INVALID elsewhere). */
DC_EXPORT int dc_sampler_debug_denoise(dc_sampler* s, const float* d_x, const int32_t* h_timesteps, float* d_out,
                             int32_t n_layers, int32_t stage, void* stream);
DC_EXPORT int dc_sampler_debug_read(dc_sampler* s, const char* what, void* h_out, int64_t nbytes);
/* Test hook: decoder layer `layer` alone on a GIVEN residual stream - h_h is host fp32 [B*T][128] row-major, the `h` a
 * LinearTemporalDiffusionTransformerDecoderLayer.forward receives (models/transformer.py:192-196); emb comes from
 * h_timesteps and the conditioning set before.  Blocks first_stage .. last_stage of the layer run (1 = sa_block,
 * 2 = ca_block, 3 = ffn; 1..3 = the whole layer); the result is left in the internal buffer "h" (dc_sampler_debug_read).
 * Lets the block-level known answers of tests/golden/g3_blocks.npz gate the kernels directly. */
DC_EXPORT int dc_sampler_debug_layer(dc_sampler* s, const float* h_h, const int32_t* h_timesteps, int32_t layer, int32_t first_stage,
                           int32_t last_stage, void* stream);

/* Post-processing of the sampled poses as tools/visualization.py applies it (smooth_motion :20-26, called with kernel=19,
 * order 5 at :126): scipy.signal.savgol_filter(mode="interp") along time for every pose channel.
 * dc_savgol_coefficients: host only; h_coef receives the [window][window] hat matrix of the polynomial fit (row window/2 =
 * the FIR taps, rows 0..window/2-1 and window/2+1.. the edge frames).  dc_savgol_filter: d_in, d_out fp32 [B, T, P] device
 * pointers (distinct), T >= window. */
DC_EXPORT int dc_savgol_coefficients(int32_t window, int32_t order, float* h_coef);
/* The same filter as part of the sampling loop: after this call dc_sampler_ddim_loop / _ex write
 * the SMOOTHED x0 to d_out - the filter reads the loop's final x0 and writes the caller's tensor in place of the plain copy, so
 * smoothing costs no pass of its own.  window = 0 switches it off again; snapshots (`idxs`) stay unsmoothed. */
DC_EXPORT int dc_sampler_set_smoothing(dc_sampler* s, int32_t window, int32_t order);
DC_EXPORT int dc_savgol_filter(const float* d_in, float* d_out, int32_t B, int32_t T, int32_t P, int32_t window, int32_t order,
                     void* stream);

/* ------------------------------------------------------------------------------------
 * Motion encoder: M2SNet's ST-GCN (the latent space of the evaluation metrics)
 * ---------------------------------------------------------------------------------- */

/* Opaque handle of one encoder (device-resident folded weights + activation planes).  Not thread-safe.
 * Replaces constructing MotionEncoder_STGCN (trainers/ddpm_trainer.py:27-43; tools/eval_new_metrics.py:39-55) on the
 * device `device`.  dc_motion_encoder_destroy, like dc_m2snet_destroy and dc_m2sgan_destroy below, frees on the handle's device and
 * puts the caller's current device back. */
typedef struct dc_motion_encoder dc_motion_encoder;
DC_EXPORT int dc_motion_encoder_create(int32_t device, dc_motion_encoder** out);
DC_EXPORT void dc_motion_encoder_destroy(dc_motion_encoder* e);

/* Replaces load_state_dict of MotionPretrain (trainers/ddpm_trainer.py:66-80): one call per state_dict entry with the key
 * WITHOUT the checkpoint's "module.motion_encoder." prefix (e.g. "st_gcn.st_gcn_networks.3.tcn.2.weight", "fc.1.running_var")
 * and its contiguous fp32 data.  Unknown key or wrong numel -> DC_ERR_PARAM.  st_gcn.fcn.* and the num_batches_tracked
 * counters are accepted and ignored (the reference never applies them in eval mode). */
DC_EXPORT int dc_motion_encoder_set_param(dc_motion_encoder* e, const char* name, const float* h_data, int64_t numel);

/* Folds every BatchNorm (eval mode, running statistics) into the conv in front of it, A * edge_importance[l] into the graph
 * mix, and uploads the image.  An entry the encoder computes with that was never set -> DC_ERR_PARAM.  Synchronous. */
DC_EXPORT int dc_motion_encoder_finalize(dc_motion_encoder* e);

/* MotionEncoder_STGCN.features(x)[-1] in eval mode (trainers/ddpm_trainer.py:45-63; the latent the metrics of
 * tools/eval_old_metrics.py:89-100 and tools/eval_new_metrics.py:159-252 use): d_motion fp32 [B, T, 13, 2] -> d_out fp32
 * [B, 64, T] (caller-allocated).  B >= 1, T >= 1.  A clip's latent is bit-identical whatever the batch around it.
 * DC_ERR_INVALID before dc_motion_encoder_finalize. */
DC_EXPORT int dc_motion_encoder_encode(dc_motion_encoder* e, const float* d_motion, int32_t B, int32_t T, float* d_out,
                                       void* stream);

/* ---- M2SNet: the learned music-motion synchronisation score ------------------------------------------------------------------
 * Replaces constructing M2SNet (Contrastive_Stage/models/M2SNet.py:7-18: a MusicEncoder, a MotionEncoder_STGCN and fuse_layer) on
 * the device `device`.  The handle owns its own music encoder - M2SNet's `music_encoder.*` weights are not the diffusion
 * checkpoint's - and its own motion encoder. */
typedef struct dc_m2snet dc_m2snet;
DC_EXPORT int dc_m2snet_create(int32_t device, dc_m2snet** out);
DC_EXPORT void dc_m2snet_destroy(dc_m2snet* n);

/* Replaces M2SNet.load_state_dict (Contrastive_Stage/M2SNet_train.py loads the DataParallel state_dict): one call per entry with
 * the key WITHOUT the "module." prefix - "music_encoder.*" (MusicEncoder.py:30-53), "motion_encoder.*" (MotionEncoder.py:6-15) and
 * "fuse_layer.{0,2,4}.{weight,bias}" (M2SNet.py:14-18), 234 entries - and its contiguous fp32 data.  Unknown key or wrong numel
 * -> DC_ERR_PARAM.  The num_batches_tracked counters and motion_encoder.st_gcn.fcn.* are accepted and ignored. */
DC_EXPORT int dc_m2snet_set_param(dc_m2snet* n, const char* name, const float* h_data, int64_t numel);

/* Replaces M2SNet.eval() + .to(device): folds every BatchNorm (running statistics) into the conv in front of it and uploads the
 * three weight images.  An entry that was never set -> DC_ERR_PARAM.  Synchronous.  Every entry point below returns
 * DC_ERR_INVALID before it. */
DC_EXPORT int dc_m2snet_finalize(dc_m2snet* n);

/* Replaces hx = self.music_encoder(x) (M2SNet.py:32; MusicEncoder.forward, MusicEncoder.py:46-53): d_mel fp32 [B, Tm, 128] ->
 * d_music_latent fp32 [B, T, 64], T = (Tm-1)/3+1, caller-allocated; Tm >= 4 (the reference's reflection padding raises below).
 * Always the DC_ME_SPLIT format (6e-6 at the encoder's output); DC_ME_PREC does not apply to this encoder. */
DC_EXPORT int dc_m2snet_encode_music(dc_m2snet* n, const float* d_mel, int32_t B, int32_t Tm, float* d_music_latent, void* stream);

/* Replaces torch.cat([hx, hy], dim=2) and fuse_layer (M2SNet.py:34-35, 14-18) on latents the caller holds: d_music_latent fp32
 * [B, T, 64] (as dc_m2snet_encode_music writes it, 16-byte aligned) and d_motion_latent fp32 [B, 64, T] (as
 * dc_motion_encoder_encode writes it), read as they are -> d_prob fp32 [B, T], the per-frame probability that the motion is in
 * sync with the music, and, unless NULL, d_logit fp32 [B, T], the value in front of the sigmoid.  B >= 1, T >= 1.  Exact-fp32
 * products in k order; a frame's result depends on that frame alone and is bit-identical whatever the batch around it. */
DC_EXPORT int dc_m2snet_fuse(dc_m2snet* n, const float* d_music_latent, const float* d_motion_latent, int32_t B, int32_t T,
                             float* d_prob, float* d_logit, void* stream);

/* Replaces M2SNet.forward (M2SNet.py:31-36), the quantity Contrastive_Stage/M2SNet_eval.py:58-107 averages: d_mel fp32
 * [B, Tm, 128] and d_motion fp32 [B, T, 13, 2] -> d_prob / d_logit as above.  T must equal (Tm-1)/3+1 and Tm >= 4, DC_ERR_INVALID
 * otherwise, before anything is enqueued.  The latents live in the handle's workspace (grown on demand; 64 clips per pass). */
DC_EXPORT int dc_m2snet_score(dc_m2snet* n, const float* d_mel, const float* d_motion, int32_t B, int32_t Tm, int32_t T,
                              float* d_prob, float* d_logit, void* stream);

/* Every music against every motion: replaces M2SNet.forward's torch.cat + fuse_layer (M2SNet.py:31-36) on all Bm x Bn pairs and
 * the per-pair reductions of Contrastive_Stage/M2SNet_eval.py:58-68 (torch.mean(pred), np.sum(pred > 0.5), np.sum(pred < 0.5)).
 * d_music_latent fp32 [Bm, T, 64] (16-byte aligned) and d_motion_latent fp32 [Bn, 64, T], as dc_m2snet_fuse takes them.  The valid
 * frames of pair (i, j) are t < min(h_len_music[i], h_len_motion[j]); either array (int32, on the host) may be NULL, meaning T; a
 * length outside [1, T] is DC_ERR_INVALID.  Outputs, caller-allocated on the device:
 *   d_sum   fp32  [Bm, Bn]     the sum of the per-frame probabilities over the pair's valid frames
 *   d_above int32 [Bm, Bn]     the number of valid frames with p > 0.5
 *   d_below int32 [Bm, Bn]     the number of valid frames with p < 0.5 (a frame at exactly 0.5, or NaN, counts in neither)
 *   d_prob  fp32  [Bm, Bn, T]  unless NULL: every frame's probability (valid or not)
 * Every probability is bit-identical to what dc_m2snet_fuse returns for that pair: layer 0's chain runs k = 0 .. 63 over the music
 * once per 32-frame tile and a copy of it is continued with each motion, in dc_m2snet_fuse's order.  The sum is taken in one fixed
 * order that depends on T alone (a 32-lane tree per tile, then the tiles ascending; no atomics), so a pair's three numbers do not
 * depend on Bm, Bn, the pair's position or the internal passes.  Partials live in the handle's workspace.  With a length array the
 * call waits for the stream once (the upload of the lengths); without, it only enqueues.  Nothing is written on an error. */
DC_EXPORT int dc_m2snet_fuse_pairs(dc_m2snet* n, const float* d_music_latent, const float* d_motion_latent, int32_t Bm, int32_t Bn,
                                   int32_t T, const int32_t* h_len_music, const int32_t* h_len_motion, float* d_sum, int32_t* d_above,
                                   int32_t* d_below, float* d_prob, void* stream);

/* The number of motions one wave of dc_m2snet_fuse_pairs walks per launch (a test straddles it). */
DC_EXPORT int32_t dc_m2snet_pairs_share(void);

/* ---- M2S-GAN generator: the baseline the diffusion denoiser is compared against ----------------------------------------------
 * Replaces constructing Generator (Contrastive_Stage/models/Generator.py:52-65: a MusicEncoder, the noise branch's four
 * ConvTranspose1d + noise_BN, and PoseDecoderTCN on the DialtedCNN of models/TCN.py) on the device `device`.  Implemented in
 * csrc/dc_m2sgan.hip; none of it is on the sampling path. */
typedef struct dc_m2sgan dc_m2sgan;
DC_EXPORT int dc_m2sgan_create(int32_t device, dc_m2sgan** out);
DC_EXPORT void dc_m2sgan_destroy(dc_m2sgan* g);

/* Replaces Generator.load_state_dict (Contrastive_Stage/M2SGAN_eval.py:451 loads the plain state_dict): one call per entry - 278
 * of them - with its key and contiguous fp32 data.  The parameters are "music_encoder.*" (MusicEncoder.py:30-53),
 * "tcn.TCN.tcn.tcn.network.{0..5}.{conv1,conv2}.{bias,weight_g,weight_v}", ".{bn1,bn2}.{weight,bias,running_mean,running_var}",
 * "tcn.TCN.tcn.tcn.network.0.downsample.{weight,bias}" (TCN.py:22-39), "tcn.TCN.tcn.linear.*" (:77), "tcn.fc.{0,2,4}.*"
 * (Generator.py:39-43), "noise_convTranspose.{0,2,4,6}.*" and "noise_BN.*" (:59-65).  The ".net.{0,2,5,7}.*" entries of a block -
 * the same tensors under their nn.Sequential names - and the num_batches_tracked counters are accepted (their sizes checked)
 * and ignored.  Unknown key or wrong numel -> DC_ERR_PARAM. */
DC_EXPORT int dc_m2sgan_set_param(dc_m2sgan* g, const char* name, const float* h_data, int64_t numel);

/* Replaces Generator.eval() + .to(device): folds weight norm (TCN.py:22, 29) and every BatchNorm (running statistics) into one
 * fp32 weight and bias per convolution, noise_BN into a scale and shift behind the last ReLU of the noise branch, packs and
 * uploads.  An entry the generator computes with that was never set -> DC_ERR_PARAM.  Synchronous.  Every entry point below
 * returns DC_ERR_INVALID before it. */
DC_EXPORT int dc_m2sgan_finalize(dc_m2sgan* g);

/* The shapes of the entry points below: d_mel fp32 [B, Tm, 128], d_noise fp32 [B, Ln, 8], T = (Tm-1)/3+1 = 30 Ln frames.
 * DC_ERR_INVALID before anything is enqueued: B < 1, Tm < 4, T != (Tm-1)/3+1, T != 30 Ln, T <= 128 (the reference raises there:
 * the last temporal block's reflection padding of 128 frames needs T > 128; the shortest length is T = 150), a NULL pointer.
 * Every product of the temporal blocks and the head is exact fp32 in k order; a clip's result is bit-identical whatever the batch
 * around it, and on every rerun.  Intermediate planes live in the handle's workspace (grown on demand; 32 clips per pass).
 * A handle serves ONE stream at a time: its workspace and weight image are shared by all its calls, and growing the workspace
 * waits for the calling stream only.  Calls on another stream must be ordered behind the earlier ones by the caller; not thread-safe.
 *
 * dc_m2sgan_features replaces Generator.features (Generator.py:79-86): cat(music_encoder(x), noise_BN(noise_convTranspose(noise^T))^T)
 * -> d_feat fp32 [B, T, 128].  The music encoder always runs the DC_ME_SPLIT format; DC_ME_PREC does not apply to it. */
DC_EXPORT int dc_m2sgan_features(dc_m2sgan* g, const float* d_mel, int32_t B, int32_t Tm, const float* d_noise, int32_t Ln, float* d_feat,
                                 void* stream);
/* Replaces self.tcn(input) (Generator.py:73; PoseDecoderTCN.forward :45-49, TCN.forward TCN.py:83-86, TemporalBlock.forward
 * :49-52) on features the caller holds: d_feat fp32 [B, T, 128] (16-byte aligned) -> d_pose fp32 [B, T, 26]. */
DC_EXPORT int dc_m2sgan_decode(dc_m2sgan* g, const float* d_feat, int32_t B, int32_t T, float* d_pose, void* stream);
/* Replaces Generator.forward (Generator.py:67-77): -> d_pose fp32 [B, T, 26] (the reference views it as [B, T, 13, 2]). */
DC_EXPORT int dc_m2sgan_generate(dc_m2sgan* g, const float* d_mel, int32_t B, int32_t Tm, const float* d_noise, int32_t Ln, float* d_pose,
                                 void* stream);
/* Test hook: the residual stream after the first n_blocks (1 .. 6) TemporalBlocks (TCN.py:49-52) of d_feat -> d_h fp32 [B, T, 64]. */
DC_EXPORT int dc_m2sgan_debug_blocks(dc_m2sgan* g, const float* d_feat, int32_t B, int32_t T, int32_t n_blocks, float* d_h, void* stream);
/* Test hook, host only: one weight-normed Conv1d (weight_g [cout], weight_v [cout, cin, k], bias; TCN.py:22-23) and the eval-mode
 * BatchNorm1d behind it (:25) as finalize folds them -> h_w fp32 [cout, k cin] (column tap cin + ci: the k order of the
 * convolution's GEMM), h_b fp32 [cout].  Computed in fp64, rounded once. */
DC_EXPORT int dc_m2sgan_fold_conv(const float* weight_g, const float* weight_v, const float* conv_bias, const float* bn_weight,
                                  const float* bn_bias, const float* bn_mean, const float* bn_var, int32_t cout, int32_t cin, int32_t k,
                                  float* h_w, float* h_b);

/* Replaces the choice of `self.tcn` in Generator.__init__ (Generator.py:57-58: PoseDecoderTCN, or PoseDecoderBiLSTM for the
 * CNN-LSTM baseline).  Call it before dc_m2sgan_finalize; a handle that never calls it decodes with the TCN, as before.
 * DC_M2SGAN_DECODER_NONE makes a features-only generator whose pose decoder is a dc_bilstm: set_param and finalize then take the
 * "music_encoder.*", "noise_convTranspose.*" and "noise_BN.*" entries only and refuse every "tcn.*" entry (DC_ERR_PARAM);
 * dc_m2sgan_features works for every T = 30 Ln (no TemporalBlock bounds it from below); dc_m2sgan_decode, _generate and
 * _debug_blocks return DC_ERR_INVALID.  Another value -> DC_ERR_INVALID. */
enum { DC_M2SGAN_DECODER_TCN = 0, DC_M2SGAN_DECODER_NONE = 1 };
DC_EXPORT int dc_m2sgan_set_decoder(dc_m2sgan* g, int32_t decoder);

/* ---- BiLSTM pose decoder: the decoder of the CNN-LSTM baselines ---------------------------------------------------------------
 * Replaces constructing PoseDecoderBiLSTM(In, 26) (Contrastive_Stage/models/Generator.py:7-25: nn.LSTM(In, 128, num_layers = 2,
 * bidirectional, batch_first, dropout 0.5 - the identity in eval mode) and the head `out`) on the device `device`: the `tcn` of
 * the CNN-LSTM Generator (:58, In = 128) and the `lstm` of Generator_CVPR_LSTM (:89-100, In = 20).  Implemented in
 * csrc/dc_bilstm.hip; none of it is on the sampling path.  dc_bilstm_destroy frees on the handle's device and puts the caller's
 * current device back. */
typedef struct dc_bilstm dc_bilstm;
DC_EXPORT int dc_bilstm_create(int32_t device, dc_bilstm** out);
DC_EXPORT void dc_bilstm_destroy(dc_bilstm* m);

/* Replaces PoseDecoderBiLSTM.load_state_dict: one call per entry with its key and contiguous fp32 data.  The keys are exactly the
 * module's: "LSTM.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0,1}" and the same with "_reverse" (Generator.py:20-21; gate rows in
 * torch's order i, f, g, o) and "out.{0,2,4}.{weight,bias}" (:22-25).  "LSTM.weight_ih_l0[_reverse]" is [512, In] for any
 * 1 <= In <= 128.  Unknown key or wrong numel -> DC_ERR_PARAM. */
DC_EXPORT int dc_bilstm_set_param(dc_bilstm* m, const char* name, const float* h_data, int64_t numel);

/* Replaces .eval() + .to(device): In = numel(LSTM.weight_ih_l0) / 512; sums b_ih + b_hh (fp64, rounded once), packs and uploads.
 * A missing entry, or one whose size does not fit In -> DC_ERR_PARAM.  Synchronous.  The entry points below return DC_ERR_INVALID
 * before it. */
DC_EXPORT int dc_bilstm_finalize(dc_bilstm* m);
/* In of a finalized handle (0 before). */
DC_EXPORT int32_t dc_bilstm_input_size(const dc_bilstm* m);

/* Replaces PoseDecoderBiLSTM.forward (Generator.py:27-31): d_feat fp32 [B, T, In] -> d_pose fp32 [B, T, 26], any B >= 1 and
 * T >= 1 (else DC_ERR_INVALID, before anything is enqueued).  Everything is enqueued on `stream`; the only host wait is a
 * workspace that has to grow.  Clips are processed in passes of dc_bilstm_pass_clips(B, T); a clip's poses do not depend on the
 * batch it is in.  A handle serves one stream at a time, as a dc_m2sgan does; not thread-safe. */
DC_EXPORT int dc_bilstm_decode(dc_bilstm* m, const float* d_feat, int32_t B, int32_t T, float* d_pose, void* stream);
/* Test hook: the output of self.LSTM (Generator.py:28) cut after `layers` (1 or 2) layers, cat(forward, reverse) -> d_h fp32 [B, T, 256]. */
DC_EXPORT int dc_bilstm_hidden(dc_bilstm* m, const float* d_feat, int32_t B, int32_t T, int32_t layers, float* d_h, void* stream);
/* Host only: clips per pass = min(B, 128, floor(2^28 / (1536 T))), at least 1 - a pass's workspace of 1536 floats per frame (the
 * gate pre-activations of both directions and the two layers' outputs) stays within 1 GiB.  0 for B < 1 or T < 1. */
DC_EXPORT int32_t dc_bilstm_pass_clips(int32_t B, int32_t T);

/* ---- Realism and rhythm: the Welch spectrum, the speed contour, the standard deviation and the M2S-GAN critic -------------------
 * The four scores of Contrastive_Stage/M2SGAN_eval.py:100-133 that look at how the motion moves.  Implemented in
 * csrc/dc_rhythm.hip; none of it is on the sampling path.  All arithmetic is fp32, every output is a fixed-order sum without
 * atomics: a clip's numbers are bit-identical on every rerun, in any batch and at any place in it.  A handle serves ONE stream at
 * a time (its workspace is shared by all its calls); not thread-safe.
 *
 * dc_rhythm owns the Welch window-and-twiddle table (built in fp64 on the host at create time, rounded once) and a workspace. */
typedef struct dc_rhythm dc_rhythm;
DC_EXPORT int dc_rhythm_create(int32_t device, dc_rhythm** out);
DC_EXPORT void dc_rhythm_destroy(dc_rhythm* h);

/* Replaces the scipy.signal.welch(x, 30) calls of rhythm_density_error (Contrastive_Stage/utils/loss.py:173-186) and the sum over
 * the 26 channels with its "/= 26": d_motion fp32 [B, T, 26] -> d_psd fp32 [B, 32], bins 0 .. 31 of PSD.sum(channels) / 26 (the
 * error itself reads bins 6 .. 25: metrics.rhythm_density_error).  scipy's defaults: nperseg = 256, noverlap = 128, periodic
 * Hann window, constant detrend per segment (removed BEFORE the window), density scaling |X_k|^2 / (30 sum w^2), one-sided doubling
 * of bins 1 .. 127, the mean over the (T - 128) / 128 segments (the tail is dropped, nothing is padded).  fs = 30 whatever the
 * clip's frame rate, as in the reference.  The signal.spectrogram calls at loss.py:168-171 fill arrays nobody reads and have no
 * counterpart.  DC_ERR_INVALID before anything is enqueued: B < 1, T < 256 (scipy shortens the window there, and the score
 * changes meaning), a NULL pointer. */
DC_EXPORT int dc_rhythm_psd(dc_rhythm* h, const float* d_motion, int32_t B, int32_t T, float* d_psd, void* stream);

/* Replaces the speed contour of strengh_contour_error (loss.py:129-142) and the standard deviation of M2SGAN_eval.py:101-102:
 * d_motion fp32 [B, T, 26] ->
 *   d_contour fp32 [B, W], W = (T - 60) / 30 + 1: d_contour[b, w] = the mean over frames 30 w .. 30 w + 59 of
 *             |mean over the 26 channels of (x[t-1] - x[t])|, the velocity at frame 0 being 0 (AvgPool1d(60, 30); per clip - the
 *             reference's unsqueeze(0) would mix the clips of a batch larger than 1);
 *   d_sd fp32 [B]: the mean over the 26 channels of the unbiased standard deviation over time (two passes, mean first).
 * Either output may be NULL.  DC_ERR_INVALID before anything is enqueued: B < 1, T < 60, a NULL handle or motion. */
DC_EXPORT int dc_rhythm_contour(dc_rhythm* h, const float* d_motion, int32_t B, int32_t T, float* d_contour, float* d_sd, void* stream);

/* Replaces motion_peak_onehot (Diffusion_Stage/tools/eval_new_metrics.py:285-309, Contrastive_Stage/M2SGAN_eval.py:310-332), the
 * motion half of beat consistency: d_motion fp32 [B, T, 26] (13 joints x (x, y)), h_length host int32 [B] or NULL (every clip T
 * frames) ->
 *   d_envelope fp32 [B, T] or NULL: the summed joint speed with the reference's float32 BITS.  e[0] = 0; for t >= 1 the sum over
 *             the 13 joints of sqrt(dx dx + dy dy), dx = x[t] - x[t-1] - every difference, product, sum and the (correctly
 *             rounded) square root rounded on its own, nothing contracted into an FMA -, the 13 norms added in the order of
 *             numpy's float32 reduction over 13 contiguous values: ((n0+n1)+(n2+n3)) + ((n4+n5)+(n6+n7)), then + n8 ... + n12 one
 *             after the other.  0 at frames >= the clip's length.  NULL: the envelope lives in the handle's workspace;
 *   d_beats uint8 [B, T]: 1 where scipy.signal.argrelextrema(e, np.less, order=`order`) - mode='clip', the default the reference
 *             relies on - finds a minimum: e[t] < e[clip(t - s)] and e[t] < e[clip(t + s)] for every s = 1 .. order, clip clamping
 *             to [0, L - 1], L the clip's length.  Strict: no plateau minimum, never frame 0, no frame <= order (e[0] = 0), never
 *             frame L - 1; 0 at frames >= L, whatever the motion holds there.
 * `order` is 10 in the reference; 1 .. 64 are accepted.  T is not bounded by LDS.  One workgroup per clip, no atomics: bit-identical
 * on a rerun, in any batch and at any place in it.  DC_ERR_INVALID before anything is enqueued: B < 1, T < 1, `order` outside
 * 1 .. 64, a length outside [1, T], a NULL handle, motion or beats pointer, a motion that is not 8-byte aligned. */
DC_EXPORT int dc_rhythm_motion_beats(dc_rhythm* h, const float* d_motion, const int32_t* h_length, int32_t B, int32_t T, int32_t order,
                                     float* d_envelope, uint8_t* d_beats, void* stream);

/* Replaces alignment_score (eval_new_metrics.py:253-275, M2SGAN_eval.py:345-367) with the music beats as an INPUT - get_music_beat
 * (librosa's tracker, a function of the clip's mel alone) stays outside: d_motion_beats uint8 [B, T] and d_music_beats uint8
 * [B, Lm], nonzero = a beat.  Music beat i sits at i / music_stride motion frames; its distance to motion beat m is
 * d = (float)|i - music_stride m| / (float)music_stride (integers until the one division).  music_stride = 1 is the reference, which
 * compares the two index lists as they are (90-fps mel frames against 30-fps motion frames, eval_new_metrics.py:312-315); 3 puts
 * both on one clock.
 *   d_scores[b, 0]  BC: the mean over the clip's music beats of expf(-d^2 / (2 sigma^2)), d to the NEAREST motion beat; 0 when the
 *                   clip has no motion beat (:255-256, tested first), NaN when it has motion beats and no music beat (the reference
 *                   divides by zero there);
 *   d_scores[b, 1]  Beat Align, the AIST++ direction the reference keeps commented out at :262-267: the mean over the motion beats
 *                   of the same Gaussian of the distance to the nearest music beat; 0 without music beats (tested first), NaN with
 *                   music beats and no motion beat;
 *   d_counts int32 [B, 2] or NULL: the number of music beats and of motion beats.
 * Sums are fp32 in a fixed order that depends on the positions alone (csrc/dc_rhythm.hip, k_beat_scores): a clip's scores are
 * bit-identical on a rerun, in any batch, at any place in it and behind any zero padding of its music beats.  The two sorted index
 * lists live in the handle's workspace.  DC_ERR_INVALID before anything is enqueued: B, T or Lm < 1, music_stride < 1, sigma not
 * finite or <= 0, a NULL handle, beats or scores pointer. */
DC_EXPORT int dc_rhythm_beat_scores(dc_rhythm* h, const uint8_t* d_motion_beats, int32_t B, int32_t T, const uint8_t* d_music_beats,
                                    int32_t Lm, int32_t music_stride, float sigma, float* d_scores, int32_t* d_counts, void* stream);

/* Replaces constructing Discriminator_1DCNN (Contrastive_Stage/models/Discriminator.py:5-27), the M2S-GAN critic whose
 * D(real) - D(fake) is the W-distance of M2SGAN_eval.py:107-109, on the device `device`. */
typedef struct dc_discriminator dc_discriminator;
DC_EXPORT int dc_discriminator_create(int32_t device, dc_discriminator** out);
DC_EXPORT void dc_discriminator_destroy(dc_discriminator* d);

/* Replaces Discriminator_1DCNN.load_state_dict (M2SGAN_eval.py:453 loads the plain state_dict): one call per entry - 12 of them,
 * "motion_encoder.{0,3,6}.{weight,bias}" (Discriminator.py:8-20) and "fc.{0,2,4}.{weight,bias}" (:21-27), 52 641 values - with its
 * key (WITHOUT a DataParallel "module." prefix: the Python loaders strip it) and contiguous fp32 data.  Unknown key or wrong numel
 * -> DC_ERR_PARAM. */
DC_EXPORT int dc_discriminator_set_param(dc_discriminator* d, const char* name, const float* h_data, int64_t numel);

/* Replaces .eval() + .to(device): permutes the convolutions' weights into the k order of their GEMMs, packs and uploads.  An
 * entry that was never set -> DC_ERR_PARAM.  Synchronous.  The two entry points below return DC_ERR_INVALID before it. */
DC_EXPORT int dc_discriminator_finalize(dc_discriminator* d);

/* Replaces Discriminator_1DCNN.features (Discriminator.py:36-41): d_motion fp32 [B, T, 26] -> d_feat fp32 [B, 64, L3] behind three
 * stages of Conv1d(kernel 5, zero padding 2) + ReLU + MaxPool1d(5, stride 3 / 2 / 2); L1 = (T-5)/3+1, L2 = (L1-5)/2+1,
 * L3 = (L2-5)/2+1 (a pool's tail is dropped).  Exact-fp32 products in k order (K = 130, 320, 320).  DC_ERR_INVALID before anything
 * is enqueued: B < 1, T < 41 (L3 < 1), a NULL pointer.  The pooled planes live in the handle's workspace (32 clips per pass). */
DC_EXPORT int dc_discriminator_features(dc_discriminator* d, const float* d_motion, int32_t B, int32_t T, float* d_feat, void* stream);
/* Replaces Discriminator_1DCNN.forward (Discriminator.py:29-34): the per-frame fc (64 -> 32 -> 32 -> 1, ReLU between) on the
 * features and the mean over the L3 frames -> d_out fp32 [B]. */
DC_EXPORT int dc_discriminator_score(dc_discriminator* d, const float* d_motion, int32_t B, int32_t T, float* d_out, void* stream);

/* ---- The mel spectrogram of a waveform: the first step of "audio in, poses out" -------------------------------------------------
 * extract_mel_feature (Diffusion_Stage/tools/visualization.py:152-167 = Contrastive_Stage/utils/music_utils.py:8-23 =
 * ProspectiveCup/utils/music_utils.py) behind librosa.load, implemented in csrc/dc_mel.hip.  Fixed: n_fft = 2048, hop = 256,
 * n_mels = 128, the periodic Hann window, center = True, power 2.  All arithmetic is fp32 on tables built in fp64 on the host and
 * rounded once; no atomics, every sum in a fixed order: a clip's numbers are bit-identical on a rerun, alone or in a batch with
 * clips of other lengths, and in any chunking.  A non-finite sample makes its clip's features NaN in every element, as numpy's
 * max does through `ref` (a maximum that is +inf counts as NaN: the reference's transform leaves inf - inf there), and touches no
 * other clip.  A handle serves ONE stream at a time (its workspace is shared by its calls); not thread-safe.
 *
 * dc_mel owns the window, the FFT twiddles and the sparse Slaney filterbank of its sample rate, and a workspace.  `sr` (the
 * reference's librosa.load resamples to 22050) moves the filterbank and the default output length only; `pad_mode` is how
 * librosa.stft pads the n_fft / 2 samples in front of and behind the clip: DC_MEL_PAD_CONSTANT zeros (librosa >= 0.10),
 * DC_MEL_PAD_REFLECT y[1024 .. 1] and y[n-2 .. n-1025] (librosa < 0.10) - the reference pins no version; the two differ in the
 * first and last four frames.  DC_ERR_INVALID: sr < 1, another pad_mode, a NULL `out`. */
typedef struct dc_mel dc_mel;
#define DC_MEL_PAD_CONSTANT 0
#define DC_MEL_PAD_REFLECT 1
DC_EXPORT int dc_mel_create(int32_t device, int32_t sr, int32_t pad_mode, dc_mel** out);
DC_EXPORT void dc_mel_destroy(dc_mel* h);

/* Host only, no device: what dc_mel_create uploads for `sr` (any pointer may be NULL).  h_window fp32 [2048]: 0.5 - 0.5 cos(2 pi n /
 * 2048); h_twiddle fp32 [2048][2]: cos and -sin of 2 pi j / 2048; the filterbank librosa.filters.mel(sr, 2048, 128) - Slaney scale and
 * norm - as runs of non-zero bins: filter m covers bins h_first[m] .. h_first[m] + h_count[m] - 1 of the 1025, its weights follow those
 * of filter m - 1 in h_weights (`max_weights` floats of room; *h_total receives their number, 2018 at 22050 Hz).  DC_ERR_INVALID: sr < 1,
 * h_weights too small. */
DC_EXPORT int dc_mel_tables(int32_t sr, float* h_window, float* h_twiddle, int32_t* h_first, int32_t* h_count, float* h_weights,
                            int32_t max_weights, int32_t* h_total);
/* Host only: the reference's int(len(y) / sr * 90) (visualization.py:160) - a double division, a double product, truncation - the
 * default output length of n samples; 0 for n < 0 or sr < 1. */
DC_EXPORT int32_t dc_mel_out_frames(int64_t n, int32_t sr);
/* Host only: the clips dc_mel_features runs per pass at N samples (its power plane stays within 512 MiB; at most 32). */
DC_EXPORT int32_t dc_mel_pass_clips(int32_t N);

/* Replaces librosa.feature.melspectrogram(y=y, sr=sr, n_mels=128, hop_length=256).T (visualization.py:162) per clip: d_wave fp32
 * [B, N], h_lengths host int32 [B] or NULL (every clip N samples; samples behind a clip's length are not read) -> d_pow fp32
 * [B, F, 128], F = 1 + N / 256 frames of the padded signal; rows behind a clip's own 1 + n_b / 256 frames are 0.  One fused pass per
 * frame - window, 2048-point real FFT in LDS, re^2 + im^2, the sparse triangles -: a spectrum never goes to global memory.
 * DC_ERR_INVALID before anything is enqueued: B < 1, N < 2048, a length outside [2048, N] (librosa only warns below one window),
 * a NULL pointer. */
DC_EXPORT int dc_mel_power(dc_mel* h, const float* d_wave, const int32_t* h_lengths, int32_t B, int32_t N, float* d_pow, void* stream);

/* Replaces extract_mel_feature's lines :159-167 per clip: dc_mel_power into the workspace, then librosa.power_to_db(mel, ref=np.max)
 * - dB = 10 log10(max(p, 1e-10)) - 10 log10(max(ref, 1e-10)) with ref the maximum over the clip's OWN frames, clamped at
 * max_dB - 80 -, |dB + 80| / 80, np.flip along the bands (output channel c is band 127 - c) and cv2.resize's INTER_LINEAR along time
 * from the clip's F_b frames to Tm_b: x = (float)((j + 0.5) (F_b / Tm_b) - 0.5) in double, i = floor(x), w = x - i; i < 0 -> (0, 0);
 * i >= F_b - 1 -> (F_b - 1, 0); out = v[i] (1 - w) + v[i + 1] w in fp32.  Tm_b = h_out_frames[b] (host int32 [B]) or, with NULL,
 * dc_mel_out_frames of the clip's length; rows behind Tm_b are 0.  d_mel fp32 [B, Tm, 128] is the layout dc_sampler_encode_music
 * reads.  A silent clip is exactly 1.0 everywhere.  DC_ERR_INVALID before anything is enqueued: dc_mel_power's, Tm < 1, an output
 * length outside [1, Tm]. */
DC_EXPORT int dc_mel_features(dc_mel* h, const float* d_wave, const int32_t* h_lengths, int32_t B, int32_t N, const int32_t* h_out_frames,
                              int32_t Tm, float* d_mel, void* stream);

/* ---- Held-out denoising losses: the forward value of the objective a checkpoint was trained on ---------------------------------
 * GaussianDiffusion.training_losses (models/gaussian_diffusion.py:1002-1090) and the weighting of DDPMTrainer.backward_G
 * (trainers/ddpm_trainer.py:223-268) as an EVALUATOR: one model evaluation per clip and noise level, no gradients.  The model
 * evaluation between the noising and the reductions is dc_sampler_denoise (per-clip timesteps), the latents of the feature term are
 * dc_motion_encoder_encode.  Implemented in csrc/dc_loss.hip; none of it is on the sampling path. */

/* The two scalars of q_sample per clip, from the tables GaussianDiffusion.__init__ builds at :352-353 (sqrt_alphas_cumprod,
 * sqrt_one_minus_alphas_cumprod), cast the way _extract_into_tensor (:1168-1181) casts them: for h_timesteps int32 [B]
 *   h_a[b] = (float)sqrt(abar[t_b]),   h_s[b] = (float)sqrt(1.0 - abar[t_b])       (fp64, rounded once)
 * h_alphas_cumprod fp64 [n_train].  DC_ERR_INVALID for a timestep outside [0, n_train).  Host only. */
DC_EXPORT int dc_q_sample_coefficients(int32_t n_train, const double* h_alphas_cumprod, const int32_t* h_timesteps, int32_t B,
                                       float* h_a, float* h_s);

/* GaussianDiffusion.q_sample (models/gaussian_diffusion.py:398-416): d_xt[b] = h_a[b] * d_x0[b] + h_s[b] * noise[b] over fp32
 * [B, T, P], h_a / h_s host arrays [B] (dc_q_sample_coefficients).  Two rounded products and one rounded sum per element, never
 * contracted: the bits of the reference's fp32 tensor expression.
 *   d_noise != NULL: that tensor (the reference's `noise=` argument); seed, iteration, first_element are not read and d_noise_out
 *                    must be NULL.
 *   d_noise == NULL: the library's Philox stream, draw (seed, iteration, first_element + element) - exactly what
 *                    dc_step_noise_fill writes for (seed, iteration) at that element, so a clip's draw does not depend on the batch
 *                    it sits in when first_element is its offset in the whole data set's draw.  The reference draws th.randn_like
 *                    on its own generator (:1017-1018).  d_noise_out (may be NULL) receives the draws: an EPSILON model's target.
 * d_xt, d_noise_out and d_x0 are distinct buffers.  B, T, P >= 1. */
DC_EXPORT int dc_q_sample(const float* d_x0, const float* d_noise, const float* h_a, const float* h_s, int32_t B, int32_t T, int32_t P,
                          uint64_t seed, int32_t iteration, uint64_t first_element, float* d_noise_out, float* d_xt, void* stream);

/* The reductions of training_losses (:1075-1083) and the masked reconstruction sum of backward_G (ddpm_trainer.py:232-233), PER CLIP:
 * d_pred, d_target fp32 [B, T, 26] (8-byte aligned), h_length int32 [B] (NULL = all T) -> d_terms fp32 [B][DC_LOSS_TERMS]:
 *   [0]  mse_b = mean over (T, 26) of (target - pred)^2                               (:1079; not masked, as in the reference)
 *   [1]  rec_b = sum over frames t < length_b of the mean over the 26 channels of (pred - target)^2
 *                                                       (the numerator of ddpm_trainer.py:232-233; the batch scalar is sum rec_b / sum length_b)
 *   [2] [3] [4]  mean over (T - 1, group) of (pred[t+1] - pred[t])^2, channel groups body {10..13, 22..25}, elbow {14..21},
 *                head {0..9}                                                                                     (:1075-1082)
 *   [5]  mean over (T - 1, 26) of ((target[t+1] - target[t]) - (pred[t+1] - pred[t]))^2                          (:1083)
 *   [6] [7]  0
 * Every clip has the same element count, so the reference's batch scalars are the plain means of these over the clips, and a clip's
 * numbers do not depend on its neighbours.  One workgroup of 256 threads per clip: a fixed number of fp32 partials combined in a
 * fixed tree, no floating-point atomics - a rerun is bit-identical (orders and the error bound they give: csrc/dc_loss.hip).
 * DC_ERR_INVALID before any device call: P != 26, T < 2 (the velocity means run over no elements; the reference returns NaN there),
 * a length outside [1, T], a NULL or misaligned tensor. */
#define DC_LOSS_TERMS 8
DC_EXPORT int dc_motion_loss_terms(const float* d_pred, const float* d_target, const int32_t* h_length, int32_t B, int32_t T, int32_t P,
                                   float* d_terms, void* stream);

/* The latent feature term of backward_G (ddpm_trainer.py:237-238: L1Loss of features(fake)[-1] against features(real)[-1]), PER CLIP:
 * d_a, d_b fp32 [B, 64, T] as dc_motion_encoder_encode writes them (16-byte aligned) -> d_out fp32 [B], the clip's mean |a - b|.
 * The reference's scalar is the plain mean over the clips.  Same reduction rules as dc_motion_loss_terms.  B, T >= 1. */
DC_EXPORT int dc_latent_l1(const float* d_a, const float* d_b, int32_t B, int32_t T, float* d_out, void* stream);

/* ---- The variational bound: scoring a checkpoint in bits per dimension ---------------------------------------------------------
 * GaussianDiffusion.calc_bpd_loop (models/gaussian_diffusion.py:1110-1165) evaluates the model at EVERY timestep and, behind each
 * evaluation, _vb_terms_bpd (:967-1000) with normal_kl (:162-188) and discretized_gaussian_log_likelihood (:199-225), the x0 error
 * (:1149) and the epsilon error (:1150-1151); _prior_bpd (:1092-1108) closes the sum.  The model evaluation is dc_sampler_denoise, the
 * noising dc_q_sample; what follows an evaluation is ONE fused pass here.  Implemented in csrc/dc_loss.hip; not on the sampling path. */

/* The reference's enums (:275-308, enum.auto() in their order). */
#define DC_VB_MEAN_PREVIOUS_X 1
#define DC_VB_MEAN_START_X 2
#define DC_VB_MEAN_EPSILON 3
#define DC_VB_VAR_LEARNED 1
#define DC_VB_VAR_FIXED_SMALL 2
#define DC_VB_VAR_FIXED_LARGE 3
#define DC_VB_VAR_LEARNED_RANGE 4

/* The per-clip scalars of one step, from the tables GaussianDiffusion.__init__ builds of h_betas fp64 [n_train] (:328-379), each
 * (float) of the fp64 entry - what _extract_into_tensor(...).float() (:1168-1181) yields.  h_coef fp32 [B][DC_VB_COEF]:
 *   [0] [1]  posterior_mean_coef1 / coef2 [t]                                   (:373-379)
 *   [2]      posterior_log_variance_clipped [t]  (= min_log of LEARNED_RANGE)   (:368-372)
 *   [3]      the model's log-variance: FIXED_SMALL the same entry, FIXED_LARGE log(append(posterior_variance[1], betas[1:]))[t]
 *            (:488-503), LEARNED_RANGE max_log = log(betas)[t] (:479-480), LEARNED 0 (not read)
 *   [4] [5]  sqrt_recip_alphas_cumprod [t], sqrt_recipm1_alphas_cumprod [t]     (:357-358)
 *   [6]      1 where t == 0 (the step whose term is the decoder NLL, :999), else 0
 *   [7] [8]  (1 / posterior_mean_coef1) [t], (posterior_mean_coef2 / posterior_mean_coef1) [t]: PREVIOUS_X's pred_xstart (:545-553)
 *   [9..11]  0
 * DC_ERR_INVALID: a timestep outside [0, n_train), a beta outside (0, 1], an unknown var_type, FIXED_LARGE with n_train < 2.
 * Host only. */
#define DC_VB_COEF 12
DC_EXPORT int dc_vb_coefficients(int32_t n_train, const double* h_betas, int32_t var_type, const int32_t* h_timesteps, int32_t B,
                                 float* h_coef);

/* _vb_terms_bpd (:967-1000) behind p_mean_variance (:442-536), and the two errors of calc_bpd_loop (:1149-1151), PER CLIP: d_x0, d_xt,
 * d_model_out (the mean-parameter half of the model's output), d_var_values (the other half of a LEARNED / LEARNED_RANGE model, NULL
 * for a fixed variance), d_noise (the draw d_xt was noised with; NULL: slot 4 is not computed) fp32 [B, T, P], h_coef of
 * dc_vb_coefficients -> d_terms fp32 [B][DC_VB_TERMS]:
 *   [0]  output = t == 0 ? decoder_nll : kl                                     (:999)
 *   [1]  kl = mean normal_kl(true_mean, true_log_variance_clipped, mean, log_variance) / log 2          (:986-989)
 *   [2]  decoder_nll = - mean discretized_gaussian_log_likelihood(x0, mean, 0.5 log_variance) / log 2   (:991-995)
 *   [3]  xstart_mse = mean (pred_xstart - x0)^2                                 (:1149)
 *   [4]  mse = mean (eps - noise)^2, eps = _predict_eps_from_xstart(x_t, t, pred_xstart)   (:1150-1151; 0 without d_noise)
 *   [5..7]  0
 * The per-element expressions are the reference's fp32 expressions in the reference's order, never contracted, with tanhf / logf /
 * expf: where fp32 tanh saturates the clamp at 1e-12 gives log 1e-12, as in the reference.  mean_type DC_VB_MEAN_*, var_type
 * DC_VB_VAR_*, clip_denoised as p_mean_variance's.  Any P >= 1.  Deterministic and batch-independent: a clip is reduced by a number
 * of workgroups that depends on T * P only, their partial sums (d_workspace, dc_vb_workspace_floats(B, T, P) floats) are added in
 * index order by a second launch; no floating-point atomics (orders and rounding counts: csrc/dc_loss.hip).
 * DC_ERR_INVALID before any device call: a NULL pointer, B, T or P < 1, T * P >= 2^31 - 1, an unknown type, d_var_values missing for a
 * learned variance or given beside a fixed one. */
#define DC_VB_TERMS 8
DC_EXPORT int64_t dc_vb_workspace_floats(int32_t B, int32_t T, int32_t P);
DC_EXPORT int dc_vb_terms(const float* d_x0, const float* d_xt, const float* d_model_out, const float* d_var_values, const float* d_noise,
                          const float* h_coef, int32_t mean_type, int32_t var_type, int32_t clip_denoised, int32_t B, int32_t T,
                          int32_t P, float* d_workspace, float* d_terms, void* stream);

/* _prior_bpd (:1092-1108): d_out[b] = mean over (T, P) of normal_kl(h_a[b] * x0, h_logvar[b], 0, 0) / log 2, with h_a[b] =
 * (float)sqrt_alphas_cumprod[S - 1] and h_logvar[b] = (float)log_one_minus_alphas_cumprod[S - 1] (host arrays [B]).  One workgroup per
 * clip, same reduction rules. */
DC_EXPORT int dc_prior_kl(const float* d_x0, const float* h_a, const float* h_logvar, int32_t B, int32_t T, int32_t P, float* d_out,
                          void* stream);

/* Introspection used by tests: bytes of device workspace currently held; frames per clip of the sampler's internal token space
 * (the T of dc_sampler_set_conditioning, padded to whole 32-frame groups where the clip-aligned kernels run): the layout of the
 * buffers dc_sampler_debug_read returns. */
DC_EXPORT int64_t dc_sampler_workspace_bytes(const dc_sampler* s);
DC_EXPORT int32_t dc_sampler_clip_stride(const dc_sampler* s);

#ifdef __cplusplus
}
#endif
#endif /* DC_DDIM_H */
