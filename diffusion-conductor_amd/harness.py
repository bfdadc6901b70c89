"""Drop-in for the sampling half of the reference's ``DDPMTrainer``.

Mirrors Diffusion_Stage/trainers/ddpm_trainer.py: constructor (:82-108, minus the training-only
MotionPretrain/ST-GCN and mmcv imports), ``load`` (:303-319), ``eval_mode``, ``to`` and
``generate_music_motion`` (:183-201).  Extensions over the reference: ``music_mel`` may be a
batch ``[B,5400,128]``; ``noise=`` / ``seed=`` make sampling reproducible; under an initialised
``torch.distributed`` group the clips are sharded over ranks (sharding.py);
``generate_long_music_motion`` conducts music longer than one window by chaining windows around
the frames already generated (``plan_windows``); ``validation_losses`` is the forward value of
``forward`` + ``backward_G`` (:132-163, 223-268) on held-out clips, without gradients.
"""
from __future__ import annotations

import numpy as np
import torch

from .sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule
from .sharding import dist_info, sharded_sample


LONG_OVERLAP = 300       # frames (10 s at 30 fps) a window of generate_long_music_motion shares with its predecessor by default


def plan_windows(L, T, overlap):
    """The windows of a piece of L frames sampled T frames at a time: [(start, known)] in sampling order.  Window k starts at
    k * (T - overlap); the LAST window is aligned to the end of the piece (start L - T), so every window has T frames.  `known` is
    the number of leading frames of the window that earlier windows have produced (0 for the first; `overlap` for the regular
    ones; whatever is already there for the last).  Pure; raises ValueError for L < T or an overlap outside [0, T)."""
    L, T, overlap = int(L), int(T), int(overlap)
    if T < 1 or not 0 <= overlap < T:
        raise ValueError(f"overlap must be in [0, {T}) frames, got {overlap}")
    if L < T:
        raise ValueError(f"a piece of {L} frames is shorter than one window of {T}")
    starts = [0]
    while starts[-1] + T < L:
        starts.append(min(starts[-1] + T - overlap, L - T))
    return [(s, 0 if k == 0 else starts[k - 1] + T - s) for k, s in enumerate(starts)]


def window_weights(L, T, starts, blend="tent"):
    """The blend weights of a piece of L frames sampled JOINTLY over windows of T frames at `starts` (ascending, from 0 to L - T, no
    gap): fp32 [W, T], row k the weight of window k's local frames.  A window's raw weight at local frame j is min(j + 1, T - j)
    (blend="tent": 1 at the window's edges, rising linearly to its middle, so a window hands a frame over to its neighbour across
    their overlap) or 1 (blend="uniform": the plain mean); the raw weights are normalised over the windows that cover a frame in
    fp64 and rounded to fp32 once, so they sum to 1 within an fp32 ulp, and a frame under a single window gets exactly 1.0.
    Pure; ValueError for starts that are not such a cover or an unknown blend.  (dc_sampler_set_conditioning_windows checks the
    cover count - at most 4 windows over a frame - and the sums again.)"""
    L, T = int(L), int(T)
    st = [int(s) for s in np.asarray(starts).reshape(-1)]
    if blend not in ("tent", "uniform"):
        raise ValueError(f"blend must be 'tent' or 'uniform', got {blend!r}")
    if T < 1 or L < T or not st or st[0] != 0 or st[-1] != L - T or any(b <= a or b > a + T for a, b in zip(st, st[1:])):
        raise ValueError(f"starts must ascend from 0 to L - T = {L - T} without leaving a gap between windows of {T} frames, got {st}")
    j = np.arange(T)
    raw = np.minimum(j + 1, T - j).astype(np.float64) if blend == "tent" else np.ones(T, np.float64)
    total, cover = np.zeros(L, np.float64), np.zeros(L, np.int64)
    for s in st:
        total[s:s + T] += raw
        cover[s:s + T] += 1
    w = np.empty((len(st), T), np.float32)
    for k, s in enumerate(st):
        wk = raw / total[s:s + T]
        wk[cover[s:s + T] == 1] = 1.0
        w[k] = wk.astype(np.float32)
    return w


class DDPMTrainer(object):
    def __init__(self, args, encoder):
        self.opt = args
        self.device = args.device
        self.encoder = encoder
        self.diffusion_steps = args.diffusion_steps
        betas = get_named_beta_schedule("linear", self.diffusion_steps)
        self.diffusion = GaussianDiffusion(betas=betas, model_mean_type=ModelMeanType.START_X,
                                           model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)
        if getattr(args, "is_train", False):
            raise NotImplementedError("this package covers the sampling path only")
        self.to(self.device)

    def to(self, device):
        self.encoder.to(device)

    def eval_mode(self):
        self.encoder.eval()

    def load(self, model_dir):
        """ddpm_trainer.py:303-319 (inference branch): checkpoint['encoder'] with strict=False."""
        checkpoint = torch.load(model_dir, map_location="cpu")
        self.encoder.load_state_dict(checkpoint["encoder"], strict=False)
        return checkpoint.get("ep", 0), checkpoint.get("total_it", 0)

    @staticmethod
    def _solver_kwargs(steps, spacing, solver):
        """The keywords of ddim_sample_loop for a loop on a sub-sequence of timesteps; none when the defaults were left (the
        loop is then called as before)."""
        if steps is None and solver == "ddim":
            return {}
        return {"steps": steps, "spacing": spacing, "solver": solver}

    def _sample_local(self, mel, noise, dim_pose, idxs, smooth=None, guidance_scale=None, skw={}, takes=1):
        xf_proj, xf_out = self.encoder.encode_music(mel, self.device)
        B, T = mel.shape[0], xf_proj.shape[1]
        tkw = {} if takes == 1 else {"takes": takes}      # (one take: the loop is called as before)
        try:
            return self.diffusion.ddim_sample_loop(
                self.encoder, (takes * B, T, dim_pose), noise=noise, clip_denoised=False, progress=False,
                model_kwargs={"xf_proj": xf_proj, "xf_out": xf_out,
                              "length": torch.LongTensor([T] * B)},
                idxs=idxs, smooth=smooth, guidance_scale=guidance_scale, **skw, **tkw)
        except FloatingPointError:
            # The loop's numeric check failed.  If the music features themselves are not finite, the fp16-plane MusicEncoder
            # overflowed (an activation beyond 65504; the reference's mel is normalised to [0, 1], so this takes unusual input):
            # encode once more on the split bf16 planes (fp32 range) and sample again.  Anything else is the caller's to see.
            if getattr(self.encoder, "encoder_format", "split") == "split" or bool(torch.isfinite(xf_out).all()):
                raise
            self.encoder.encoder_format = "split"
            nat = getattr(self.encoder, "_native", None)
            if nat is not None:
                nat.set_encoder_format("split")
            return self._sample_local(mel, noise, dim_pose, idxs, smooth, guidance_scale, skw, takes)

    def generate_music_motion(self, music_mel, dim_pose, batch_size=1024, idxs=[], noise=None, seed=None, smooth=None,
                              guidance_scale=None, steps=None, spacing="uniform", solver="ddim", takes=1):
        """music_mel: np.ndarray/tensor [5400,128] (reference) or [B,5400,128] -> tensor [B,1800,dim_pose].
        takes: samples per music (default 1) -> tensor [takes * B, 1800, dim_pose], TAKE-MAJOR: row j * B + b is take j of music b
        (result.view(takes, B, 1800, dim_pose)[j, b]).  The music is encoded once and the takes share every step's conditioning work
        (GaussianDiffusion.ddim_sample_loop, takes=); `noise`, when given, is [takes * B, 1800, dim_pose] in the same order, and `seed`
        draws that many clips - the takes differ through their noise alone.  Not sharded over the ranks of a group yet.
        smooth: None, or the Savitzky-Golay kernel size (order 5) tools/visualization.py:126 smooths the keypoints with - applied
        by the sampling loop's final write.
        guidance_scale: None, or the classifier-free guidance scale of the loop (GaussianDiffusion.ddim_sample_loop; each rank of a
        sharded run builds the unconditional shadows of its own clips).
        steps, spacing, solver: sample on `steps` of the schedule's timesteps picked by `spacing`, with the first-order update
        ("ddim") or the second-order multistep one ("dpmpp2m"; GaussianDiffusion.ddim_sample_loop - `idxs` then count that loop's
        iterations).  Left at their defaults the loop walks every timestep, as before.  Not sharded over the ranks of a group yet."""
        skw = self._solver_kwargs(steps, spacing, solver)
        mel = torch.as_tensor(np.asarray(music_mel) if not torch.is_tensor(music_mel) else music_mel)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        # A pinned fp32 host batch stays on the host: encode_music copies it in chunks beside the encoder (denoiser.py,
        # _encode_music_pipelined), and a rank of a sharded run copies only its own clips.  Everything else (pageable host
        # memory - the driver stages it through its own pinned buffers anyway -, other dtypes, device tensors) goes to the
        # device here, as ddpm_trainer.py:185 does.
        if not (not mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous() and mel.is_pinned()):
            mel = mel.to(self.device, dtype=torch.float32)
        B, T = mel.shape[0], (mel.shape[1] - 1) // 3 + 1       # frames encode_music produces (MusicEncoder pools time by 3)
        _, world = dist_info()
        if skw and world > 1:
            raise NotImplementedError("steps= / solver= are not sharded over the ranks of a torch.distributed group yet")
        if int(takes) != takes or int(takes) < 1:
            raise ValueError(f"takes must be an integer >= 1, got {takes!r}")
        takes = int(takes)
        if takes > 1 and world > 1:
            raise NotImplementedError("takes= are not sharded over the ranks of a torch.distributed group yet")
        grouped = torch.distributed.is_available() and torch.distributed.is_initialized()     # a world-size-1 group still gathers
        if noise is None and (seed is not None or world > 1):
            # x_T for the WHOLE batch from one generator, sliced per shard: with every rank drawing from its own default
            # generator, identically seeded ranks would hand all shards the same noise rows.  Without a seed, rank 0's draw
            # is broadcast.
            g = torch.Generator()
            if seed is not None:
                g.manual_seed(int(seed))
            else:
                s0 = torch.tensor([g.seed() & 0x7fffffffffffffff], dtype=torch.int64, device=self.device if world > 1 else "cpu")
                if world > 1:
                    import torch.distributed as dist
                    dist.broadcast(s0, src=0)
                g.manual_seed(int(s0.item()))
            noise = torch.randn(takes * B, T, dim_pose, generator=g)
        if noise is not None:
            noise = torch.as_tensor(noise).to(self.device, dtype=torch.float32)
        sm = (int(smooth), 5) if smooth else None
        with torch.no_grad():
            if not grouped or len(idxs) or takes > 1:      # (takes: a single rank, checked above)
                return self._sample_local(mel, noise, dim_pose, idxs, sm, guidance_scale, skw, takes)
            return sharded_sample(lambda m, n: self._sample_local(m, n, dim_pose, [], sm, guidance_scale, skw), mel, noise, out_shape=(T, dim_pose),
                                  device=self.device)

    def _validation_batch(self, xf_proj, xf_out, x0, lengths, t, noise=None, noise_seed=None, motion_encoder=None):
        """One noise level of validation_losses on music that is already encoded: x0 [B, T, 26] on the device, lengths / t host
        int arrays [B].  Handing the SAME xf_proj / xf_out tensors to several calls reuses the conditioning pre-pass (the encoder
        keys it by tensor identity)."""
        from . import native
        from .metrics import denoising_loss_scalars
        B, T = int(x0.shape[0]), int(x0.shape[1])
        tt = torch.as_tensor(np.asarray(t, np.int64)).to(x0.device)
        out = self.diffusion.training_losses(self.encoder, x0, tt, noise=noise, noise_seed=noise_seed,
                                             model_kwargs={"xf_proj": xf_proj, "xf_out": xf_out, "length": torch.as_tensor(np.asarray(lengths, np.int64))})
        feat = None
        if motion_encoder is not None:
            # features(.)[-1] of the prediction and of the target (ddpm_trainer.py:225-229), right behind the reductions on the stream
            fake = motion_encoder.latent(out["pred"].reshape(B, T, 13, 2))
            real = motion_encoder.latent(out["target"].reshape(B, T, 13, 2))
            feat = native.latent_l1(fake, real) if fake.is_cuda else (fake - real).abs().mean(dim=(1, 2))
        terms = out["terms"].cpu()              # the one wait: every number below is host arithmetic on these B x 8 floats
        res = denoising_loss_scalars(terms, lengths, None if feat is None else feat.cpu())
        res.update(t=[int(v) for v in t], mse_per_clip=terms[:, 0].tolist(), terms=terms.numpy(),
                   latent_l1=None if feat is None else feat.cpu().numpy())
        return res

    def validation_losses(self, music_mel, motions, m_lens=None, t=None, noise=None, seed=None, motion_encoder=None, noise_seed=None):
        """The held-out value of the training objective (DDPMTrainer.forward + backward_G, ddpm_trainer.py:132-163, 223-268, without
        gradients): music_mel [B, 5400, 128] and motions [B, T, 13, 2] (or [B, T, 26]), or one clip of each; m_lens [B] frame counts
        (None: all T; values beyond T count as T, :143).  ONE model evaluation per clip.
        t: per-clip timesteps [B] or one int for all; None draws one uniform timestep per clip on the host from `seed` (the reference's
        UniformSampler protocol: np.random.choice over the schedule with equal weights).
        noise: the tensor to add ([B, T, 13, 2] or [B, T, 26]); None: the library's device stream, keyed by `noise_seed` = seed or
        (seed, iteration, first_element) (default: `seed`, or one drawn from torch's generator).
        motion_encoder (motion_encoder.MotionEncoder_STGCN or anything with its `latent`): adds the latent feature term.
        Returns the per-clip "t", "mse_per_clip", "terms" [B, 8] (and "latent_l1" [B] or None), the batch scalars "loss_mot_rec",
        "loss_mot_feat" (None without an encoder), "loss_velocity", "loss_velocity_elbow", "loss_velocity_head", "loss_velocity_body",
        and the total "loss" with "feat_included" (metrics.denoising_loss_scalars)."""
        mel = torch.as_tensor(np.asarray(music_mel) if not torch.is_tensor(music_mel) else music_mel)
        x0 = torch.as_tensor(np.asarray(motions) if not torch.is_tensor(motions) else motions)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        if x0.dim() == 3 and x0.shape[-1] == 2:
            x0 = x0.unsqueeze(0)
        B, T = int(x0.shape[0]), int(x0.shape[1])
        if mel.shape[0] != B:
            raise ValueError(f"{mel.shape[0]} musics for {B} motions")
        x0 = x0.to(self.device, dtype=torch.float32).reshape(B, T, -1).contiguous()
        lengths = np.full(B, T, np.int64) if m_lens is None else np.minimum(np.asarray(m_lens, np.int64).reshape(B), T)
        S = self.diffusion.num_timesteps
        if t is None:
            t = np.random.RandomState(None if seed is None else int(seed) & 0xffffffff).choice(S, size=(B,), p=np.ones(S) / S)
        t = np.broadcast_to(np.asarray(t.cpu() if torch.is_tensor(t) else t, np.int64).reshape(-1), (B,)).copy()
        if noise is not None:
            noise = torch.as_tensor(noise).to(self.device, dtype=torch.float32).reshape(B, T, -1).contiguous()
        elif noise_seed is None:
            noise_seed = int(seed) if seed is not None else int(torch.randint(0, 2 ** 62, (1,)).item())
        with torch.no_grad():
            xf_proj, xf_out = self.encoder.encode_music(mel if mel.is_cuda else mel.to(self.device, dtype=torch.float32), self.device)
            if xf_proj.shape[1] != T:
                raise ValueError(f"the music gives {xf_proj.shape[1]} frames, the motions have {T}")
            return self._validation_batch(xf_proj, xf_out, x0, lengths, t, noise, noise_seed, motion_encoder)

    def bound_bpd(self, music_mel, motions, m_lens=None, timesteps=None, seed=None):
        """The variational bound of the checkpoint on held-out clips, in bits per dimension (GaussianDiffusion.calc_bpd_loop,
        gaussian_diffusion.py:1110-1165): music_mel [B, 5400, 128] and motions [B, T, 13, 2] (or [B, T, 26]), or one clip of each; m_lens
        [B] frame counts for the model's mask (None: all T).  ONE encode_music call, then one model evaluation per timestep.
        timesteps: a list - only those (the sum is then left out); None - every timestep of the schedule.
        seed: of the library's device draws, step t's noise being (seed, iteration = t); None draws one from torch's generator.
        Returns the per-clip arrays "vb" [B, K], "xstart_mse" [B, K], "mse" [B, K] (columns by descending "timesteps"), "prior_bpd" [B],
        "total_bpd" [B] (None for a subset), and their means over the clips: "mean_total_bpd" (or None), "mean_prior_bpd", "mean_vb" [K],
        "mean_xstart_mse" [K], "mean_mse" [K]."""
        mel = torch.as_tensor(np.asarray(music_mel) if not torch.is_tensor(music_mel) else music_mel)
        x0 = torch.as_tensor(np.asarray(motions) if not torch.is_tensor(motions) else motions)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        if x0.dim() == 3 and x0.shape[-1] == 2:
            x0 = x0.unsqueeze(0)
        B, T = int(x0.shape[0]), int(x0.shape[1])
        if mel.shape[0] != B:
            raise ValueError(f"{mel.shape[0]} musics for {B} motions")
        x0 = x0.to(self.device, dtype=torch.float32).reshape(B, T, -1).contiguous()
        lengths = np.full(B, T, np.int64) if m_lens is None else np.minimum(np.asarray(m_lens, np.int64).reshape(B), T)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        with torch.no_grad():
            xf_proj, xf_out = self.encoder.encode_music(mel if mel.is_cuda else mel.to(self.device, dtype=torch.float32), self.device)
            if xf_proj.shape[1] != T:
                raise ValueError(f"the music gives {xf_proj.shape[1]} frames, the motions have {T}")
            return self._bound_batch(xf_proj, xf_out, x0, lengths, timesteps, seed)

    def _bound_batch(self, xf_proj, xf_out, x0, lengths, timesteps, seed):
        """bound_bpd on music that is already encoded: x0 [B, T, 26] on the device, lengths a host int array [B]."""
        S = int(self.diffusion.num_timesteps)
        r = self.diffusion.calc_bpd_loop(self.encoder, x0, clip_denoised=True, noise_seed=seed, timesteps=timesteps,
                                         model_kwargs={"xf_proj": xf_proj, "xf_out": xf_out, "length": torch.as_tensor(np.asarray(lengths, np.int64))})
        K = int(r["vb"].shape[1])
        full = r["total_bpd"] is not None
        # the one wait: every array below is a slice of this [B, 3 K + 2] host tensor
        flat = torch.cat([r["vb"], r["xstart_mse"], r["mse"], r["prior_bpd"][:, None],
                          (r["total_bpd"] if full else r["prior_bpd"])[:, None]], dim=1).cpu().numpy()
        out = {"timesteps": list(range(S))[::-1] if timesteps is None else sorted({int(v) for v in np.asarray(timesteps).reshape(-1)}, reverse=True),
               "vb": flat[:, :K], "xstart_mse": flat[:, K:2 * K], "mse": flat[:, 2 * K:3 * K], "prior_bpd": flat[:, 3 * K],
               "total_bpd": flat[:, 3 * K + 1] if full else None}
        out.update(mean_total_bpd=float(out["total_bpd"].mean()) if full else None, mean_prior_bpd=float(out["prior_bpd"].mean()),
                   mean_vb=out["vb"].mean(axis=0), mean_xstart_mse=out["xstart_mse"].mean(axis=0), mean_mse=out["mse"].mean(axis=0))
        return out

    def generate_long_music_motion(self, music_mel, dim_pose, overlap=LONG_OVERLAP, noise=None, seed=None, smooth=None, window=None,
                                   guidance_scale=None, steps=None, spacing="uniform", solver="ddim", joint=False, blend="tent",
                                   known=None, known_mask=None, known_noise=None):
        """Conduct music LONGER than one window: music_mel [Tm,128] or [B,Tm,128] (pieces of one length), Tm at least one window
        (3 * window mel frames; ValueError below that - generate_music_motion serves those) -> tensor [B, L, dim_pose] with
        L = (Tm-1)//3 + 1.

        The piece is sampled in windows of `window` frames (default: the model's num_frames, 1800 = 5400 mel frames) laid out by
        plan_windows: window k starts at frame k * (window - overlap), the last one at L - window.  The mel slices of all windows of
        all pieces go through ONE encode_music call (window k reads mel frames [3 start, 3 start + 3 window), the last window the
        piece's last 3 window frames); sampling is sequential over the windows and batched over the pieces.  Each window is a
        ddim_sample_loop AROUND KNOWN VALUES: its first `known` frames are the frames the earlier windows produced, every other
        frame is generated.  The output is the plain concatenation - no cross-fade: the loop returns known elements bit for bit,
        so the frames two windows share are identical in both.

        Noise: ONE tensor [B, L, dim_pose] for the whole piece (`noise=`, or drawn from `seed`, or from torch's default generator).
        Window k at frame s takes rows [s, s + window) of it both as its x_T and as its known_noise: a frame's fixed draw is the
        row of its ABSOLUTE position in the piece, which is the x_T row the previous window started that frame from.

        `overlap` (frames, default LONG_OVERLAP = 300: 10 s); `smooth`: the Savitzky-Golay kernel size (order 5), applied ONCE
        over the whole piece with dc_savgol_filter (per window it would break the seams).  Every window runs the same captured
        graph (the first with an all-zero mask) - also with `guidance_scale` (classifier-free guidance of every window's loop) and with `steps`, `spacing`, `solver` (every window's loop on that sub-sequence of timesteps, generate_music_motion; the solver's table carries the known slots and its last step lands on abar = 1, so the seams stay exact).  Not built: sharding pieces over the ranks of a torch.distributed group.

        `joint` (default False: the sequential path above, untouched): True samples ALL windows in ONE loop whose state is the whole
        piece [B, L, dim_pose] - at every step the model is evaluated on the W * B windows as one batch and its predictions are
        blended over the overlaps with window_weights(L, window, starts, `blend`) before the update (include/dc_ddim.h,
        dc_sampler_set_conditioning_windows; GaussianDiffusion.ddim_sample_loop, window_starts=).  Same plan_windows, same single
        encode_music call, same [B, L, dim_pose] noise.  No seam is causal any more, and `known`, `known_mask`, `known_noise` (as
        ddim_sample_loop takes them, over the whole piece) may hold any frames of the piece, its middle included; `smooth` is then
        folded into the loop's final write.  Needs overlap <= window / 2 (ValueError: beyond it a frame's weight is no longer a
        hand-over between two neighbours).  known= without joint=True is a ValueError."""
        from . import native
        _, world = dist_info()
        if world > 1:
            raise NotImplementedError("generate_long_music_motion does not shard pieces over the ranks of a torch.distributed group yet")
        if not joint and (known is not None or known_mask is not None or known_noise is not None):
            raise ValueError("known= over a whole piece needs joint=True: the sequential path gives every window's known frames itself")
        mel = torch.as_tensor(np.asarray(music_mel) if not torch.is_tensor(music_mel) else music_mel)
        if mel.dim() == 2:
            mel = mel.unsqueeze(0)
        mel = mel.to(self.device, dtype=torch.float32)
        B, Tm = mel.shape[0], mel.shape[1]
        T = int(window) if window else int(self.encoder.cfg.num_frames)
        Tw, L = 3 * T, (Tm - 1) // 3 + 1
        if Tm < Tw:
            raise ValueError(f"music of {Tm} mel frames is shorter than one window of {Tw}: use generate_music_motion")
        plan = plan_windows(L, T, overlap)
        W = len(plan)
        if joint and 2 * int(overlap) > T:
            raise ValueError(f"joint=True needs overlap <= window / 2 = {T // 2} frames, got {overlap}")
        if noise is None:
            g = None
            if seed is not None:
                g = torch.Generator()
                g.manual_seed(int(seed))
            noise = torch.randn(B, L, dim_pose, generator=g)
        noise = torch.as_tensor(noise).to(self.device, dtype=torch.float32)
        if tuple(noise.shape) != (B, L, dim_pose):
            raise ValueError(f"noise must be {(B, L, dim_pose)} (one row per frame of the piece), got {tuple(noise.shape)}")
        with torch.no_grad():
            mel_w = torch.stack([mel[:, min(3 * s, Tm - Tw):min(3 * s, Tm - Tw) + Tw] for s, _ in plan]).reshape(W * B, Tw, mel.shape[2])
            xf_proj, xf_out = self.encoder.encode_music(mel_w, self.device)
            if joint:      # one loop over the W * B windows (window-major, as encoded), its state the whole piece
                starts = [s for s, _ in plan]
                return self.diffusion.ddim_sample_loop(
                    self.encoder, (B, L, dim_pose), noise=noise, clip_denoised=False, progress=False,
                    model_kwargs={"xf_proj": xf_proj, "xf_out": xf_out}, window_starts=starts,
                    window_weights=window_weights(L, T, starts, blend), smooth=(int(smooth), 5) if smooth else None,
                    known=known, known_mask=known_mask, known_noise=known_noise, guidance_scale=guidance_scale,
                    **self._solver_kwargs(steps, spacing, solver))
            xf_proj, xf_out = xf_proj.view(W, B, T, -1), xf_out.view(W, B, T, -1)
            out = torch.zeros(B, L, dim_pose, dtype=torch.float32, device=self.device)
            length = torch.LongTensor([T] * B)
            for k, (s, kn) in enumerate(plan):
                x_T = noise[:, s:s + T].contiguous()
                mask = torch.zeros(B, T, device=self.device)
                mask[:, :kn] = 1
                out[:, s:s + T] = self.diffusion.ddim_sample_loop(
                    self.encoder, (B, T, dim_pose), noise=x_T, clip_denoised=False, progress=False,
                    model_kwargs={"xf_proj": xf_proj[k], "xf_out": xf_out[k], "length": length},
                    known=out[:, s:s + T].contiguous(), known_mask=mask, known_noise=x_T, guidance_scale=guidance_scale,
                    **self._solver_kwargs(steps, spacing, solver))
            if smooth:
                out = native.savgol_filter(out, int(smooth), 5)
        return out
