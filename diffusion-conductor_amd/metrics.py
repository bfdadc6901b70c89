"""Latent-space evaluation scores of the paper's results table: FGD, feature distance, diversity and Sync Error (SE).

Host numpy / scipy over the ST-GCN latents of motion_encoder.py (``latent(x)`` = the reference's ``features(x)[-1]``, one
[64, T] fp32 array per clip).  The arithmetic follows the reference's evaluation scripts step for step, dtypes included
(Diffusion_Stage/tools/eval_new_metrics.py:159-252 for FGD, feature distance and diversity; tools/eval_old_metrics.py:89-100,
171-197 for SE):

* the per-clip latents are stacked ROW-wise, ``np.vstack`` of [64, T] arrays -> [64 n, T]: every row (one latent channel of one
  clip) is a SAMPLE and the frames are the dimensions, so FGD is the Frechet distance between two T-dimensional Gaussians
  (1800-D on the dataset).  That is the reference's convention and what the paper's numbers mean; it is kept, and it needs
  clips of one length;
* means are float32 (numpy's mean of float32 data), ``np.cov`` and ``scipy.linalg.sqrtm`` run in float64; feature distance,
  diversity and SE are float32 reductions and come back as ``np.float32``, as in the reference.

``sync_stats`` is the one score that looks at the music: the mean predictions and the 0.5-threshold accuracy of M2SNet
(m2snet.py) over matched and mismatched music / motion pairs, as Contrastive_Stage/M2SNet_eval.py:58-107 reports them.

``denoising_loss_scalars`` is not a score of sampled motion: it combines the per-clip terms of the held-out denoising objective
(native.motion_loss_terms, native.latent_l1) into the batch scalars of DDPMTrainer.backward_G (trainers/ddpm_trainer.py:223-268).

``rhythm_density_error``, ``strength_contour_error`` and ``w_distance`` are the scores of the M2S-GAN evaluation
(Contrastive_Stage/M2SGAN_eval.py:100-133) that look at how the motion moves, over the small per-clip arrays rhythm.MotionRhythm
and discriminator.Discriminator_1DCNN compute on the device.  The reference evaluates at batch size 1 and averages the per-clip
values; these do the same.

Beat consistency (BC) and Beat Align come from SUPPLIED music beats: the reference's calculate_beat_scores
(eval_new_metrics.py:253-317) is librosa's beat tracker on the mel (get_music_beat - a function of the clip's mel alone, so a
property of the dataset: tools/music_beats_librosa.py writes it once per clip, ``load_music_beats`` reads it), the motion's beats
(motion_peak_onehot) and their alignment (alignment_score).  The last two run on the device (rhythm.MotionRhythm.motion_beats,
.beat_scores); ``motion_beats_host`` and ``beat_alignment_host`` restate them in numpy float32 - the CPU path for tests and for a
box without a GPU - and ``beat_consistency`` averages the per-clip scores.  The tracker itself is not built: it cannot be pinned
without librosa.
"""
from __future__ import annotations

import numpy as np


def _stack(latents, what):
    arrs = [np.asarray(a.detach().cpu() if hasattr(a, "detach") else a) for a in latents]
    if not arrs:
        raise ValueError(f"{what}: no clips")
    shapes = {a.shape for a in arrs}
    if len(shapes) != 1 or arrs[0].ndim != 2:
        raise ValueError(f"{what}: the reference stacks the per-clip latents [64, T] row-wise (np.vstack), which needs one shape "
                         f"for every clip; got {sorted(shapes)}")
    return np.vstack(arrs)


def calculate_frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """d^2 = |mu1 - mu2|^2 + Tr(sigma1 + sigma2 - 2 sqrt(sigma1 sigma2)), as Evaluator.calculate_frechet_distance
    (eval_new_metrics.py:201-252, after pytorch-fid): when sqrtm of the product is not finite it is taken again with `eps` added to
    both diagonals; a complex result whose diagonal has an imaginary part beyond 1e-3 raises ValueError, otherwise its real part
    is used."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError(f"mean / covariance shapes differ: {mu1.shape} vs {mu2.shape}, {sigma1.shape} vs {sigma2.shape}")
    diff = mu1 - mu2
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)


def frechet_gesture_distance(gen_latents, real_latents):
    """(fgd, feat_dist) of Evaluator.get_scores (eval_new_metrics.py:169-199): per-clip latents [64, T] of the generated and the
    real motions, in matching order.  fgd = 1e10 where calculate_frechet_distance raises ValueError (the reference's fallback);
    feat_dist = the mean over stacked rows of sum |real - gen|, an np.float32."""
    gen, real = _stack(gen_latents, "generated latents"), _stack(real_latents, "real latents")
    if gen.shape != real.shape:
        raise ValueError(f"generated {gen.shape} and real {real.shape} latents differ in shape")
    try:
        fgd = calculate_frechet_distance(np.mean(gen, axis=0), np.cov(gen, rowvar=False),
                                         np.mean(real, axis=0), np.cov(real, rowvar=False))
    except ValueError:
        fgd = 1e10
    feat_dist = np.mean(np.sum(np.absolute(real - gen), axis=-1))
    return fgd, feat_dist


def diversity_permutation(n, seed):
    """torch.randperm(n) from a fresh generator seeded with `seed`: the permutation the reference draws from the global RNG
    (eval_new_metrics.py:161) after torch.manual_seed(seed)."""
    import torch
    return torch.randperm(int(n), generator=torch.Generator().manual_seed(int(seed))).numpy()


def diversity_score(gen_latents, seed=0):
    """Evaluator.get_diversity_scores (eval_new_metrics.py:159-166): the first 500 generated clips against the clips at
    randperm(n)[:500], mean over stacked rows of sum |feat1 - feat2|; np.float32."""
    lat = list(gen_latents)
    feat1 = _stack(lat[:500], "generated latents")
    feat2 = _stack([lat[i] for i in diversity_permutation(len(lat), seed)[:500]], "generated latents")
    return np.mean(np.sum(np.absolute(feat1 - feat2), axis=-1))


def latent_mse(gen_latent, real_latent):
    """One clip's Sync Error term (eval_old_metrics.py:90-100, mse_loss_latent): mean((gen - real)^2) over its [64, T] latent,
    a float32 mean; np.float32."""
    g = np.asarray(gen_latent.detach().cpu() if hasattr(gen_latent, "detach") else gen_latent, np.float32)
    r = np.asarray(real_latent.detach().cpu() if hasattr(real_latent, "detach") else real_latent, np.float32)
    if g.shape != r.shape:
        raise ValueError(f"latent shapes differ: {g.shape} vs {r.shape}")
    return np.mean((g - r) ** 2)


def sync_error(per_clip):
    """final_latent_mse (eval_old_metrics.py:187-197): the per-clip latent_mse values summed in clip order from 0 (float32
    arithmetic, as the reference's accumulation of np.float32 terms), divided by the clip count."""
    vals = list(per_clip)
    if not vals:
        raise ValueError("sync_error: no clips")
    total = 0
    for v in vals:
        total += v
    return total / len(vals)


def sync_stats(pred_matched, pred_mismatched=None):
    """{"sync", "non_sync", "accuracy"} of M2SNet's per-frame predictions on matched pairs and on mismatched pairs (any shapes;
    tensors or arrays), as Contrastive_Stage/M2SNet_eval.py:60-67 computes them per batch: the two means are float32 means
    (`torch.mean(pred).item()`), accuracy = (count(matched > 0.5) + count(mismatched < 0.5)) / the number of predictions - a
    prediction of exactly 0.5 counts for neither side.  Without mismatched pairs "non_sync" is nan and the accuracy is the matched
    pairs' alone."""
    import torch

    def flat(p):
        t = p.detach().cpu() if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(np.asarray(p)))
        return t.to(torch.float32).reshape(-1)

    m = flat(pred_matched)
    n = flat(pred_mismatched) if pred_mismatched is not None else torch.empty(0)
    if m.numel() == 0:
        raise ValueError("sync_stats: no matched predictions")
    tp = np.sum(m.numpy() > 0.5)
    tf = np.sum(n.numpy() < 0.5)
    return {"sync": torch.mean(m).item(), "non_sync": torch.mean(n).item() if n.numel() else float("nan"),
            "accuracy": ((tp + tf) / (m.numel() + n.numel())).item()}


def retrieval_stats(score, top_k=(1, 2, 3)):
    """Ranks a square score matrix [N, N] whose entry (i, j) scores music i against motion j (higher = better matched) and whose
    diagonal holds the matched pairs - calculate_R_precision / calculate_top_k of Diffusion_Stage/utils/metrics.py:21-43 on scores
    instead of distances.  Row i's order is np.argsort(-score[i], kind="stable"): ties go to the lower column.  Returns
      "r_precision"   list over `top_k`: the share of rows whose own column is among the k best
      "top_k_table"   bool [N, max(top_k)]: column k - 1 = the own column is among the k best (calculate_top_k's cumulative table;
                      k > N, where the reference would index past the matrix, is True)
      "rank"          float [N]: the 1-based position of the own column in the row's order
      "mean_rank", "diag_mean", "offdiag_mean" (nan for N = 1), "margin" = diag_mean - offdiag_mean
    in float64.  A row holding a NaN has no order: its "rank" is nan, its table row False, and "r_precision" and "mean_rank", which
    average over every row, are nan - the NaN is never sorted into a place."""
    s = np.asarray(score, np.float64)
    if s.ndim != 2 or s.shape[0] != s.shape[1] or s.shape[0] < 1:
        raise ValueError(f"retrieval_stats: the scores must be a square [N, N] matrix with N >= 1, got {s.shape}")
    ks = [int(k) for k in top_k]
    if not ks or min(ks) < 1:
        raise ValueError(f"retrieval_stats: top_k must be positive integers, got {tuple(top_k)}")
    n = s.shape[0]
    bad = np.isnan(s).any(axis=1)
    order = np.argsort(-np.where(bad[:, None], 0.0, s), axis=1, kind="stable")
    hit = order == np.arange(n)[:, None]                 # calculate_top_k's bool_mat: one True per row
    rank = np.where(bad, np.nan, np.argmax(hit, axis=1) + 1.0)
    kmax = max(ks)
    table = np.logical_or.accumulate(np.concatenate([hit, np.zeros((n, max(0, kmax - n)), bool)], axis=1)[:, :kmax], axis=1)
    table &= ~bad[:, None]
    rp = [float("nan") if bad.any() else float(table[:, k - 1].mean()) for k in ks]
    eye = np.eye(n, dtype=bool)
    diag_mean = float(s[eye].mean())
    off_mean = float(s[~eye].mean()) if n > 1 else float("nan")
    return {"r_precision": rp, "top_k_table": table, "rank": rank, "mean_rank": float(rank.mean()), "diag_mean": diag_mean,
            "offdiag_mean": off_mean, "margin": diag_mean - off_mean}


def pair_accuracy(above, below, count):
    """The 0.5-threshold accuracy of Contrastive_Stage/M2SNet_eval.py:65-68 over an [N, N] pair matrix (M2SNet.fuse_pairs' "above",
    "below", "count": per pair, the valid frames with p > 0.5, with p < 0.5, and all of them), matched pairs on the diagonal:
    1/2 (sum_diag above / sum_diag count + sum_off below / sum_off count) - the reference's (TP + TF) / frames whenever matched and
    mismatched frames are equally many, as in its protocol; balanced, because here there are N - 1 mismatched pairs per matched one.
    N = 1 has no mismatched pair: the matched side alone.  float."""
    a, b, c = (np.asarray(x, np.int64) for x in (above, below, count))
    if a.ndim != 2 or a.shape[0] != a.shape[1] or a.shape[0] < 1 or b.shape != a.shape or c.shape != a.shape:
        raise ValueError(f"pair_accuracy: above, below and count must be one square shape, got {a.shape}, {b.shape}, {c.shape}")
    eye = np.eye(a.shape[0], dtype=bool)
    matched = a[eye].sum() / c[eye].sum()
    if a.shape[0] == 1:
        return float(matched)
    return float(0.5 * (matched + b[~eye].sum() / c[~eye].sum()))


# the weights of DDPMTrainer.backward_G (ddpm_trainer.py:252-256) and the clamp of its elbow term (:245)
LAMBDA_REC, LAMBDA_FEAT, LAMBDA_VELOCITY, LAMBDA_ELBOW, LAMBDA_HEAD = 1.0, 1e-6, 0.1, 0.1, 0.1
ELBOW_CLAMP = 2e-4


def denoising_loss_scalars(terms, lengths, latent_l1=None):
    """The batch scalars of DDPMTrainer.backward_G (ddpm_trainer.py:223-268) from per-clip numbers, in float64 on the host:
    `terms` [B, 8] (native.motion_loss_terms / GaussianDiffusion.training_losses()["terms"]: mse, masked reconstruction sum,
    velocity body / elbow / head, velocity), `lengths` [B] (the frames the reconstruction sum covered), `latent_l1` [B] (the per-clip
    mean |features(pred)[-1] - features(target)[-1]|, native.latent_l1) or None.
      loss_mot_rec        sum rec_b / sum length_b                                             (:232-233)
      loss_mot_feat       mean of latent_l1 over clips; None without it                        (:237-238)
      loss_velocity, loss_velocity_head, loss_velocity_body      means over clips              (:241-250; gaussian_diffusion.py:1080-1083)
      loss_velocity_elbow the clip mean clamped to [-2e-4, 2e-4], as the reference keeps it    (:245); velocity_elbow: unclamped
      mse                 mean of mse_b over clips                                             (gaussian_diffusion.py:1079)
      loss                rec + 1e-6 feat + 0.1 velocity - 0.1 loss_velocity_elbow + 0.1 head  (:258); the feat term is left out when
                          it is None, and "feat_included" says which."""
    t = np.asarray(terms.detach().cpu() if hasattr(terms, "detach") else terms, np.float64)
    if t.ndim != 2 or t.shape[1] != 8 or t.shape[0] < 1:
        raise ValueError(f"terms must be [B, 8] with B >= 1, got {t.shape}")
    ln = np.asarray(lengths.detach().cpu() if hasattr(lengths, "detach") else lengths, np.float64).reshape(-1)
    if ln.shape != (t.shape[0],) or (ln < 1).any():
        raise ValueError(f"lengths must be [{t.shape[0]}] positive frame counts, got {ln.tolist()}")
    feat = None
    if latent_l1 is not None:
        f = np.asarray(latent_l1.detach().cpu() if hasattr(latent_l1, "detach") else latent_l1, np.float64).reshape(-1)
        if f.shape != (t.shape[0],):
            raise ValueError(f"latent_l1 must be [{t.shape[0]}], got {f.shape}")
        feat = float(f.mean())
    rec = float(t[:, 1].sum() / ln.sum())
    body, elbow, head, vel = (float(t[:, k].mean()) for k in (2, 3, 4, 5))
    elbow_c = min(max(elbow, -ELBOW_CLAMP), ELBOW_CLAMP)
    loss = LAMBDA_REC * rec + LAMBDA_VELOCITY * vel - LAMBDA_ELBOW * elbow_c + LAMBDA_HEAD * head
    if feat is not None:
        loss += LAMBDA_FEAT * feat
    return {"loss": loss, "loss_mot_rec": rec, "loss_mot_feat": feat, "loss_velocity": vel, "loss_velocity_elbow": elbow_c,
            "loss_velocity_head": head, "loss_velocity_body": body, "velocity_elbow": elbow, "mse": float(t[:, 0].mean()),
            "feat_included": feat is not None}


RDE_BAND = (6, 26)      # `threshold`, `bins` of rhythm_density_error (loss.py:183-184): 0.70 .. 2.93 Hz at fs = 30, nperseg = 256


def _per_clip(a, what, width=None):
    a = np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)
    a = a if a.dtype in (np.float32, np.float64) else a.astype(np.float32)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or (width is not None and a.shape[1] < width):
        raise ValueError(f"{what}: expected one row per clip, got {a.shape}")
    return a


def rhythm_density_error(psd_real, psd_gen):
    """RDE of Contrastive_Stage/utils/loss.py:183-190 from the channel-averaged Welch PSDs [n, >= 26] (rhythm.MotionRhythm.psd) of the
    real and the generated clips: per clip log(mean((r[6:26] - g[6:26])^2) * 1e7 + 1) - the mean in the arrays' own dtype, the
    logarithm in float64, as in the reference - and the mean over the clips (M2SGAN_eval.py:162).  -> (per clip float64 [n], mean)."""
    r, g = _per_clip(psd_real, "psd_real", RDE_BAND[1]), _per_clip(psd_gen, "psd_gen", RDE_BAND[1])
    if r.shape != g.shape:
        raise ValueError(f"rhythm_density_error: {r.shape} real and {g.shape} generated spectra")
    lo, hi = RDE_BAND
    per = np.array([np.log(np.float64(((r[i, lo:hi] - g[i, lo:hi]) ** 2).mean()) * 1e7 + 1) for i in range(r.shape[0])], np.float64)
    return per, float(per.mean())


def strength_contour_error(contour_real, contour_gen):
    """SCE of loss.py:149-151 from the speed contours [n, W] (rhythm.MotionRhythm.contour): per clip log(mean_w((g - r)^2) * 1e7 + 1)
    in float32, as the reference's torch expression, and the mean over the clips (M2SGAN_eval.py:163).  -> (per clip float32 [n], mean)."""
    r, g = _per_clip(contour_real, "contour_real"), _per_clip(contour_gen, "contour_gen")
    if r.shape != g.shape:
        raise ValueError(f"strength_contour_error: {r.shape} real and {g.shape} generated contours")
    r, g = r.astype(np.float32), g.astype(np.float32)
    per = np.array([np.log(((g[i] - r[i]) ** 2).mean(dtype=np.float32) * np.float32(1e7) + np.float32(1)) for i in range(r.shape[0])], np.float32)
    return per, float(per.astype(np.float64).mean())


def w_distance(d_real, d_gen):
    """The W-distance of M2SGAN_eval.py:107-109, 150-151: the mean over the clips of D(real) - D(fake), critic scores [n] or [n, 1]."""
    r = np.asarray(d_real.detach().cpu() if hasattr(d_real, "detach") else d_real, np.float32).reshape(-1)
    g = np.asarray(d_gen.detach().cpu() if hasattr(d_gen, "detach") else d_gen, np.float32).reshape(-1)
    if r.shape != g.shape or not r.size:
        raise ValueError(f"w_distance: {r.shape} real and {g.shape} generated scores")
    return float((r - g).astype(np.float64).mean())


def standard_deviation_percentage(sd_gen, sd_real):
    """SDP of the competition's evaluation (Contrastive_Stage/ProspectiveCup/eval.py:78): the mean standard deviation of the generated
    motion as a percentage of the real motion's, mean(SD_fake) / mean(SD_real) * 100.  `sd_gen`, `sd_real`: the per-clip standard
    deviations (arrays or tensors), or their means - evaluate_dataset's "sd_gen" and "sd_real"."""
    g = np.asarray(sd_gen.detach().cpu() if hasattr(sd_gen, "detach") else sd_gen, np.float64).reshape(-1)
    r = np.asarray(sd_real.detach().cpu() if hasattr(sd_real, "detach") else sd_real, np.float64).reshape(-1)
    if not g.size or not r.size:
        raise ValueError(f"standard_deviation_percentage: {g.size} generated and {r.size} real standard deviations")
    if not r.mean() > 0:
        raise ValueError(f"standard_deviation_percentage: the real motion's mean standard deviation is {r.mean()}, not positive")
    return float(g.mean() / r.mean() * 100.0)


BEAT_ORDER, BEAT_SIGMA = 10, 3.0      # argrelextrema's order (eval_new_metrics.py:301) and alignment_score's sigma (:315)
_BEAT_LANES = 256                     # threads of csrc/dc_rhythm.hip's k_beat_scores: the partial sums of its summation order


def _motion_clips(motion):
    x = np.asarray(motion.detach().cpu() if hasattr(motion, "detach") else motion, np.float32)
    if x.ndim == 3 and x.shape[-1] == 2:              # one clip [T, 13, 2]
        x = x[None]
    if x.ndim not in (3, 4) or x.size != x.shape[0] * x.shape[1] * 26:
        raise ValueError(f"motion must be [T, 13, 2], [B, T, 26] or [B, T, 13, 2], got {x.shape}")
    return x.reshape(x.shape[0], x.shape[1], 13, 2)


def motion_beats_host(motion, length=None, order=BEAT_ORDER):
    """motion_peak_onehot (eval_new_metrics.py:285-309) as the device computes it (dc_rhythm_motion_beats), in numpy float32:
    -> (beats bool [B, T], envelope float32 [B, T]).  The envelope is e[0] = 0, e[t] = the sum over the 13 joints of
    sqrt(dx dx + dy dy), every operation rounded on its own and the 13 norms added as numpy's float32 reduction over 13 contiguous
    values adds them - ((n0+n1)+(n2+n3)) + ((n4+n5)+(n6+n7)), then n8 .. n12 one by one -, written out so that it does not depend
    on the numpy it runs under.  A beat is a strict minimum over +-`order` frames, the index clamped to the clip
    (scipy.signal.argrelextrema's mode='clip').  `length`: None or the clips' frame counts; frames behind one are 0."""
    x = _motion_clips(motion)
    B, T = x.shape[:2]
    if not 1 <= int(order) <= 64:
        raise ValueError(f"order {order} is outside 1 .. 64")
    ln = np.full(B, T, np.int64) if length is None else np.asarray(length, np.int64).reshape(-1)
    if ln.shape != (B,) or ln.min() < 1 or ln.max() > T:
        raise ValueError(f"length must hold {B} values in [1, {T}], got {ln.tolist()}")
    env, beats = np.zeros((B, T), np.float32), np.zeros((B, T), bool)
    for b in range(B):
        L = int(ln[b])
        v = x[b, 1:L] - x[b, :L - 1]
        n = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])                   # [L - 1, 13] float32
        s = ((n[:, 0] + n[:, 1]) + (n[:, 2] + n[:, 3])) + ((n[:, 4] + n[:, 5]) + (n[:, 6] + n[:, 7]))
        for j in range(8, 13):
            s = s + n[:, j]
        e = env[b, :L]
        e[1:] = s
        t = np.arange(L)
        ok = np.ones(L, bool)
        for k in range(1, int(order) + 1):
            ok &= (e < e[np.clip(t - k, 0, L - 1)]) & (e < e[np.clip(t + k, 0, L - 1)])
        beats[b, :L] = ok
    return beats, env


def _onehots(a, what):
    a = np.asarray(a.detach().cpu() if hasattr(a, "detach") else a)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] < 1:
        raise ValueError(f"{what}: expected one-hots [B, L], got {a.shape}")
    return a != 0


def _ordered_sum(terms):
    """The float32 sum of `terms` (one per position, 0 where there is no beat) in k_beat_scores' order: partial j adds the positions
    j, j + 256, ... in increasing order, then the partials are added as a binary tree (j with j + 128, then + 64, ...)."""
    pad = np.zeros(-len(terms) % _BEAT_LANES, np.float32)
    rows = np.concatenate([terms.astype(np.float32), pad]).reshape(-1, _BEAT_LANES)
    acc = np.zeros(_BEAT_LANES, np.float32)
    for r in rows:
        acc = acc + r
    while acc.size > 1:
        acc = acc[:acc.size // 2] + acc[acc.size // 2:]
    return acc[0]


def _nearest_terms(query, keys, stride, sigma):
    """float32 exp(-d^2 / (2 sigma^2)), d = (float)min |query - keys| / (float)stride, for every query; integers in music frames."""
    j = np.searchsorted(keys, query)
    above = np.abs(keys[np.minimum(j, len(keys) - 1)] - query)
    below = np.abs(query - keys[np.maximum(j - 1, 0)])
    d = np.minimum(above, below).astype(np.float32) / np.float32(stride)
    return np.exp(-(d * d) / (np.float32(2) * np.float32(sigma) * np.float32(sigma)))


def beat_alignment_host(music_onehot, motion_onehot, sigma=BEAT_SIGMA, music_stride=1):
    """alignment_score (eval_new_metrics.py:253-275) as the device computes it (dc_rhythm_beat_scores), in numpy float32: one-hots
    [Lm] and [T], or [B, Lm] and [B, T] (nonzero = a beat) -> float32 [2] or [B, 2]: BC - the mean over the music beats of
    exp(-d^2 / (2 sigma^2)), d the distance to the nearest motion beat; 0 without motion beats, NaN with motion beats and no music
    beat - and Beat Align, the other direction (0 without music beats, NaN with music beats and no motion beat).  Music beat i sits
    at i / music_stride motion frames: 1 is the reference (the index lists compared as they are), 3 puts 90-fps music frames and
    30-fps motion frames on one clock."""
    single = np.ndim(music_onehot) == 1
    mus, mot = _onehots(music_onehot, "music_onehot"), _onehots(motion_onehot, "motion_onehot")
    if mus.shape[0] != mot.shape[0]:
        raise ValueError(f"{mus.shape[0]} clips of music beats and {mot.shape[0]} of motion beats")
    if int(music_stride) < 1 or not (np.isfinite(sigma) and sigma > 0):
        raise ValueError(f"music_stride {music_stride} must be >= 1 and sigma {sigma} finite and > 0")
    s = int(music_stride)
    out = np.zeros((mus.shape[0], 2), np.float32)
    for b in range(mus.shape[0]):
        i, m = np.flatnonzero(mus[b]).astype(np.int64), np.flatnonzero(mot[b]).astype(np.int64)
        bc, ba = np.zeros(mus.shape[1], np.float32), np.zeros(mot.shape[1], np.float32)
        if i.size and m.size:
            bc[i] = _nearest_terms(i, s * m, s, sigma)
            ba[m] = _nearest_terms(s * m, i, s, sigma)
        with np.errstate(invalid="ignore", divide="ignore"):
            out[b, 0] = 0 if not m.size else _ordered_sum(bc) / np.float32(i.size)
            out[b, 1] = 0 if not i.size else _ordered_sum(ba) / np.float32(m.size)
    return out[0] if single else out


def beat_consistency(scores, counts, ids, column=0):
    """The mean over the clips of the per-clip scores [n, 2] of dc_rhythm_beat_scores (`column` 0: BC, 1: Beat Align) and
    {clip id: score}.  `counts` [n, 2]: the clips' music and motion beat counts.  A clip without a music beat has no BC (the
    reference divides by zero there): ValueError naming those clips.  (Beat Align of a clip without a motion beat is NaN, and so is
    its mean: that is a finding about the motion, not about the input.)"""
    s = np.asarray(scores.detach().cpu() if hasattr(scores, "detach") else scores, np.float32).reshape(-1, 2)
    c = np.asarray(counts.detach().cpu() if hasattr(counts, "detach") else counts).reshape(-1, 2)
    ids = list(ids)
    if not (len(ids) == s.shape[0] == c.shape[0]) or not ids:
        raise ValueError(f"beat_consistency: {s.shape[0]} scores, {c.shape[0]} counts and {len(ids)} clip ids")
    silent = [cid for cid, n in zip(ids, c[:, 0]) if n == 0]
    if silent:
        raise ValueError(f"beat_consistency: no music beat in {len(silent)} clip(s): {silent[:8]}{' ...' if len(silent) > 8 else ''}")
    return float(s[:, column].astype(np.float64).mean()), {cid: float(v) for cid, v in zip(ids, s[:, column])}


def load_music_beats(path, ids):
    """{clip id: uint8 one-hot [Lm]} for `ids` from an .npz whose keys are clip ids and whose values are 1-D one-hots (bool, uint8 or
    float; nonzero = a beat) - the `beat_onehot` the reference's get_music_beat returns, one entry per mel frame
    (tools/music_beats_librosa.py writes it).  ValueError for a clip id the file lacks or an array that is not 1-D."""
    out = {}
    with np.load(path) as z:
        missing = [cid for cid in ids if cid not in z.files]
        if missing:
            raise ValueError(f"{path} has no music beats for {len(missing)} clip(s): {missing[:8]}{' ...' if len(missing) > 8 else ''}")
        for cid in ids:
            a = z[cid]
            if a.ndim != 1 or a.size < 1:
                raise ValueError(f"{path}: the music beats of clip {cid} have shape {a.shape}, expected a 1-D one-hot")
            out[cid] = (a != 0).astype(np.uint8)
    return out
