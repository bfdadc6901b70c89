"""Batched evaluation driver and pose post-processing.

Replaces the serial B=1 loops of the reference's evaluation scripts
(Diffusion_Stage/tools/eval_new.py:104-134, eval_old_metrics.py:175-191, eval_new_metrics.py:129-156):
walk a dataset directory of ``<clip id>/mel.npy`` (``[5400,128]``) + ``<clip id>/motion.npy`` (``[1800,13,2]``;
on-disk format of the reference's README.md:53-84), sample every clip and report the per-clip MSE the way
eval_new.py does (``np.mean((pred - gt) ** 2)``, summed in directory order, then divided by the clip count).

Here the clips go through the sampler ``batch_size`` at a time: mel files and noise are prepared by background
threads in pinned host buffers while the GPU samples the previous batch, the batch is sharded over the ranks of an
initialised ``torch.distributed`` group by ``DDPMTrainer.generate_music_motion``, the poses come back with one
copy behind an event and are scored on a third thread - the GPU's queue never runs dry (tools/time_evaluate.py).  ``smooth_motion`` is tools/visualization.py:20-26 (Savitzky-Golay, kernel 19, order 5 at
:126) on the GPU.

``validation_dataset`` (``--val_loss``) scores a checkpoint WITHOUT sampling it: the held-out value of the denoising objective it was
trained on (models/gaussian_diffusion.py:1002-1090, trainers/ddpm_trainer.py:223-268), per noise level.  ``bound_dataset``
(``--bpd``) scores it by its variational bound in bits per dimension (calc_bpd_loop, models/gaussian_diffusion.py:1110-1165): one
model evaluation per clip and timestep, as a per-timestep table.
"""
from __future__ import annotations

import functools
import os
import threading
import time
from os.path import join as pjoin

import numpy as np
import torch


def mse_loss(gt_motion, pred_motion):
    """eval_new.py:37-44."""
    return np.mean((pred_motion - gt_motion) ** 2)


def list_clips(root):
    """Clip ids (sub-directories holding mel.npy and motion.npy), sorted for a reproducible order
    (the reference iterates os.listdir order, eval_new.py:106-113)."""
    return sorted(d for d in os.listdir(root)
                  if os.path.isfile(pjoin(root, d, "mel.npy")) and os.path.isfile(pjoin(root, d, "motion.npy")))


def smooth_motion(kp_pred, kernel=11, order=5):
    """tools/visualization.py:20-26 for a pose tensor on the GPU: [T,13,2], [B,T,13,2] or [B,T,26]."""
    from .native import savgol_filter
    x = kp_pred if torch.is_tensor(kp_pred) else torch.as_tensor(np.asarray(kp_pred))
    single = x.dim() == 3 and x.shape[-1] == 2            # [T, J, 2]
    y = x.unsqueeze(0) if single else x
    if not y.is_cuda:
        raise RuntimeError("smooth_motion runs on the MI355X only (no CPU path); pass a device tensor")
    out = savgol_filter(y.float(), kernel, order).view(y.shape)
    return out[0] if single else out


def clip_noise(seed, index, T, dim_pose, out=None):
    """x_T of clip `index` (position in sorted order): its own generator, independent of batching.  `out`: a [T, dim_pose] fp32 CPU
    tensor to draw into (a row of the pinned batch buffer: a `copy_` between two CPU tensors goes through torch's thread pool and
    costs milliseconds per clip - it was what bound the evaluation driver's loader)."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(index)) & 0x7fffffffffff)
    return torch.randn(T, dim_pose, generator=g) if out is None else torch.randn(T, dim_pose, generator=g, out=out)


def _read_npy_into(path, dst):
    """One clip's mel.npy into a row of the pinned batch buffer with a single copy (np.load would allocate an array first and the
    batch of 32 x 2.8 MB would be copied twice per 40 ms of GPU work)."""
    m = np.load(path, mmap_mode="r")
    if m.shape != tuple(dst.shape):
        raise ValueError(f"{os.path.basename(os.path.dirname(path))}/mel.npy has shape {m.shape}, expected {tuple(dst.shape)}")
    np.copyto(dst.numpy(), m, casting="same_kind")


class _Prefetcher:
    """Prepares the next batch on background threads while the GPU samples the current one: the .npy files into a pinned buffer
    (a small pool reads the clips of a batch side by side), the ground-truth motions, and - `noise=(seed, T, dim_pose)` - every
    clip's x_T into a second pinned buffer.  Two slots; `start(k, after=event)` waits for `event` (the GPU is done with the slot's
    previous batch) before it overwrites the slot."""

    def __init__(self, root, ids, batch_size, mel_shape, noise=None, workers=None):
        self.root, self.ids, self.bs = root, ids, batch_size
        pin = torch.cuda.is_available()
        self.buf = [torch.empty((batch_size,) + tuple(mel_shape), dtype=torch.float32, pin_memory=pin) for _ in range(2)]
        self.noise_spec = noise
        self.nbuf = [torch.empty((batch_size, noise[1], noise[2]), dtype=torch.float32, pin_memory=pin) for _ in range(2)] if noise else None
        # (four threads: with 16 the loaders fight the enqueueing thread for the interpreter lock - 288 clips took 1.35 s instead of 0.40,
        # profiles/r05_time_evaluate.txt)
        self.workers = max(1, int(workers)) if workers else 4
        self.result = None
        self.noise = None
        self.error = None
        self.thread = None

    def _load(self, k, slot, after):
        try:
            if after is not None:
                after.synchronize()
            self._load_batch(k, slot)
        except BaseException as e:      # handed to the consumer: a dead loader thread must not leave the previous batch behind
            self.error = e

    def _load_batch(self, k, slot):
        ids = self.ids[k * self.bs:(k + 1) * self.bs]
        mel = self.buf[slot][:len(ids)]
        gts = [None] * len(ids)
        nz = self.nbuf[slot][:len(ids)] if self.nbuf else None

        def one(i):
            _read_npy_into(pjoin(self.root, ids[i], "mel.npy"), mel[i])
            gts[i] = np.load(pjoin(self.root, ids[i], "motion.npy"))
            if nz is not None:
                seed, T, dim_pose = self.noise_spec
                clip_noise(seed, k * self.bs + i, T, dim_pose, out=nz[i])

        if self.workers > 1 and len(ids) > 1:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(self.workers) as ex:
                list(ex.map(one, range(len(ids))))      # (re-raises a worker's exception)
        else:
            for i in range(len(ids)):
                one(i)
        self.noise = nz
        self.result = (ids, mel, gts)

    def start(self, k, after=None):
        self.result = None
        self.noise = None
        self.error = None
        self.thread = threading.Thread(target=self._load, args=(k, k & 1, after), daemon=True)
        self.thread.start()

    def take(self):
        self.thread.join()
        if self.error is not None:
            raise self.error
        return self.result


def _open_dataset(root, limit, batch_size):
    """(clip ids, a mel's shape, the frames T it gives, the number of batches) of the first `limit` clips under `root`."""
    ids = list_clips(root)
    if limit is not None:
        ids = ids[:int(limit)]
    if not ids:
        raise FileNotFoundError(f"no <id>/mel.npy + <id>/motion.npy pairs under {root}")
    mel_shape = tuple(np.load(pjoin(root, ids[0], "mel.npy"), mmap_mode="r").shape)
    return ids, mel_shape, (mel_shape[0] - 1) // 3 + 1, (len(ids) + batch_size - 1) // batch_size


def _clip_mses(ids, gts, pred, dim_pose):
    """[(clip id, mse)] of a batch's poses (numpy [B, T, dim_pose]) against its ground truths (eval_new.py:124-131)."""
    return [(cid, mse_loss(gts[i], pred[i].reshape([pred[i].shape[0], dim_pose // 2, 2]))) for i, cid in enumerate(ids)]


class _Batch:
    """One sampled batch on its way to the score families: its number `k`, the index `first` of its first clip, its `ids`, `mel`
    (host) and `gts` (the motions as loaded), the sampled `pred` [B, T, dim_pose] on its device, and `slot` - which of the two pinned
    host slots the pipelined loop gave it, None for a batch that is sampled again: later batches may still be queued on the scoring
    thread and read those slots, so nothing of such a batch may be written there."""

    def __init__(self, k, first, ids, mel, gts, pred, slot):
        self.k, self.first, self.ids, self.mel, self.gts, self.pred, self.slot = k, first, ids, mel, gts, pred, slot

    @functools.cached_property
    def _truth(self):
        gt = torch.from_numpy(np.ascontiguousarray(np.stack([np.reshape(g, -1) for g in self.gts]), np.float32))
        return gt.pin_memory().to(self.pred.device, non_blocking=True) if self.pred.is_cuda else gt

    def ground_truth(self, *shape):
        """The ground truth fp32 [B, *shape] on the poses' device: stacked, pinned and uploaded on the current stream by the first
        family that asks, and viewed by the others.  (Each family refuses the clips it cannot score before it asks.)"""
        return self._truth.view(len(self.gts), *shape)


class _LatentScores:
    """`motion_encoder` (a motion_encoder.MotionEncoder_STGCN, or anything with its `latent(x)` -> [B, 64, T]): the latent-space
    scores of the paper's table (metrics.py), added as "latent_mse" ({id: the clip's Sync Error term}, eval_old_metrics.py:90-100),
    "final_latent_mse" (SE), "fgd", "feat_dist" (eval_new_metrics.py:169-199), "diversity" (:159-166, permutation drawn with
    `diversity_seed`) and "metrics_s" (host seconds spent on FGD, feat_dist and diversity after the last batch).  The sampled poses
    and the ground truth are encoded on the device right after each batch's sampling, on the same stream, and the latents come back
    with the poses, into a pinned double buffer; the scoring thread takes them from there.  Every clip must have the poses' T frames
    (ValueError otherwise).  With `smooth` the latents are those of the SMOOTHED poses - the reference scores the unsmoothed output."""

    def __init__(self, motion_encoder, diversity_seed, ids, T, dim_pose, batch_size):
        self.encoder, self.diversity_seed, self.ids, self.dim_pose, self.batch_size = motion_encoder, diversity_seed, ids, dim_pose, batch_size
        self.slots = [None, None]        # pinned [2 (generated, real), batch_size, 64, T]
        self.clips = {}                  # batch -> [(latent_mse, generated latent [64, T], real latent [64, T])], filled once it has landed

    def enqueue(self, batch, pred):
        B, T, J = pred.shape[0], pred.shape[1], self.dim_pose // 2
        bad = [(cid, np.shape(g)) for cid, g in zip(batch.ids, batch.gts) if tuple(np.shape(g)) != (T, J, 2)]
        if bad:
            raise ValueError(f"the latent metrics compare clips of {T} frames ([T, {J}, 2] motions; the reference stacks the "
                             f"latents with np.vstack), but these ground truths differ: {bad[:4]}")
        gt = batch.ground_truth(T, J, 2)
        lats = self.encoder.latent(pred.reshape(B, T, J, 2)), self.encoder.latent(gt)
        s = batch.slot
        if s is None:                    # (a batch sampled again: pageable memory and blocking copies)
            host = torch.empty((2, B) + tuple(lats[0].shape[1:]), dtype=torch.float32)
        else:
            if self.slots[s] is None or self.slots[s].shape[1] < B or self.slots[s].shape[2:] != lats[0].shape[1:]:
                self.slots[s] = torch.empty((2, self.batch_size) + tuple(lats[0].shape[1:]), dtype=torch.float32, pin_memory=pred.is_cuda)
            host = self.slots[s][:, :B]
        host[0].copy_(lats[0], non_blocking=s is not None)
        host[1].copy_(lats[1], non_blocking=s is not None)
        k = batch.k                      # (the callable holds the host tensor, not the batch and its device tensors)
        return lambda: self._landed(k, host.numpy())

    def _landed(self, k, lats):
        from .metrics import latent_mse
        pairs = [(np.array(g), np.array(r)) for g, r in zip(lats[0], lats[1])]      # (copies: the pinned slot is reused two batches later)
        self.clips[k] = [(latent_mse(g, r), g, r) for g, r in pairs]

    def finish(self, out, verbose):
        from .metrics import diversity_score, frechet_gesture_distance, sync_error
        tm = time.perf_counter()
        clips = [c for k in sorted(self.clips) for c in self.clips[k]]
        out["latent_mse"] = {cid: float(c[0]) for cid, c in zip(self.ids, clips)}
        out["final_latent_mse"] = float(sync_error([c[0] for c in clips]))
        gen, real = [c[1] for c in clips], [c[2] for c in clips]
        fgd, feat_dist = frechet_gesture_distance(gen, real)
        out["fgd"], out["feat_dist"], out["diversity"] = float(fgd), float(feat_dist), float(diversity_score(gen, self.diversity_seed))
        out["metrics_s"] = time.perf_counter() - tm
        if verbose:
            print("final_latent_mse: ", out["final_latent_mse"])
            print(f"fgd: {out['fgd']}  feat_dist: {out['feat_dist']}  diversity: {out['diversity']}")


RETRIEVAL_TOP_K = (1, 2, 3)            # the reference's R-precision columns (Diffusion_Stage/utils/metrics.py calculate_R_precision, top_k = 3)


class _SyncScores:
    """`m2snet` (an m2snet.M2SNet, or anything with its `music_latent`, `motion_latent` and `fuse`): the learned synchronisation
    score - the one number here that looks at the music.  Each batch's music is encoded once and scored against the ground truth,
    the sampled poses and, as the mismatched control, the sampled poses of the next clip of the batch (rolled by one; left out for a
    batch of one clip, so the control depends on `batch_size`); the per-frame predictions [B, T] stay on the poses' device until the
    end.  Adds "m2s_sync_real", "m2s_sync_gen", "m2s_sync_mismatched" (mean per-frame predictions over all clips; nan when no batch had
    two clips) and "m2s_accuracy_gen" (metrics.sync_stats: matched = generated, mismatched = rolled).

    `retrieval` (needs `m2snet`, which must have `fuse_pairs`): the question the rolled control cannot ask - does a motion follow its
    own music better than it follows the other pieces of the set?  The music latents [B, T, 64] and the real and generated motion
    latents [B, 64, T] of ALL clips stay on the device (3 x 64 T floats per clip); after the last batch every music is scored against
    every real and every generated motion (two M2SNet.fuse_pairs, N^2 pairs each; a pair's score is the mean per-frame probability) and
    the N x N matrices are ranked on the host (metrics.retrieval_stats, the reference's calculate_R_precision / calculate_top_k of
    Diffusion_Stage/utils/metrics.py on scores instead of distances).  Adds "m2s_r_precision_real" / "_gen" (lists over top-1, 2, 3:
    the share of musics whose own motion is among the k best), "m2s_mean_rank_real" / "_gen" (1 = best), "m2s_margin_real" / "_gen"
    (mean matched score minus mean mismatched score), "m2s_sync_offdiag_gen" (the mean mismatched score: every other clip, not the
    next one of the batch), "m2s_pair_accuracy_real" / "_gen" (metrics.pair_accuracy: M2SNet_eval.py:65-68 with matched and
    mismatched frames weighted equally) and "m2s_retrieval_s".  None of them depends on `batch_size` or on the order of the clips
    (ties go to the lower clip index).  The clips must share one latent length (ValueError naming two that differ).  The other
    keys, the rolled control among them, are what they are without it.

    (Built before the dataset is opened - its refusal has always come first - so it takes none of the dataset's facts.)"""

    def __init__(self, m2snet, retrieval, dim_pose):
        if retrieval and (m2snet is None or not hasattr(m2snet, "fuse_pairs")):
            raise ValueError("retrieval=True ranks M2SNet's scores of every pair: pass m2snet= (an m2snet.M2SNet, with fuse_pairs)")
        self.net, self.dim_pose = m2snet, dim_pose
        self.preds = {}                  # batch -> (real, generated, mismatched | None) predictions [B, T] on the device
        self.kept = {} if retrieval else None      # batch -> (its first clip's id, music latent, real motion latent, generated motion latent)

    def enqueue(self, batch, pred):
        B, T, net = pred.shape[0], pred.shape[1], self.net
        gt = batch.ground_truth(-1, self.dim_pose // 2, 2)
        mel = torch.as_tensor(batch.mel)
        if pred.is_cuda:
            mel = mel.to(pred.device, non_blocking=True)
        mus = net.music_latent(mel)
        real_lat = net.motion_latent(gt)
        real = net.fuse(mus, real_lat)
        gen_lat = net.motion_latent(pred.reshape(B, T, self.dim_pose // 2, 2))
        gen = net.fuse(mus, gen_lat)
        mis = net.fuse(mus, torch.roll(gen_lat, -1, 0).contiguous()) if B > 1 else None
        self.preds[batch.k] = (real, gen, mis)
        if self.kept is not None:
            self.kept[batch.k] = (batch.ids[0], mus, real_lat, gen_lat)

    def finish(self, out, verbose):
        from .metrics import sync_stats
        real, gen, mis = ([torch.as_tensor(self.preds[k][i]).cpu().reshape(-1) for k in sorted(self.preds) if self.preds[k][i] is not None]
                          for i in range(3))
        st = sync_stats(torch.cat(gen), torch.cat(mis) if mis else None)
        out["m2s_sync_real"] = sync_stats(torch.cat(real))["sync"]
        out["m2s_sync_gen"], out["m2s_sync_mismatched"], out["m2s_accuracy_gen"] = st["sync"], st["non_sync"], st["accuracy"]
        if verbose:
            print(f"m2s_sync_real: {out['m2s_sync_real']}  m2s_sync_gen: {out['m2s_sync_gen']}  "
                  f"m2s_sync_mismatched: {out['m2s_sync_mismatched']}  m2s_accuracy_gen: {out['m2s_accuracy_gen']}")
        if self.kept is not None:
            tm = time.perf_counter()
            self._retrieval(out)
            out["m2s_retrieval_s"] = time.perf_counter() - tm
            if verbose:
                print("  ".join(f"{key}: {out[key]}" for key in sorted(out) if key.startswith(("m2s_r_", "m2s_mean_rank", "m2s_margin", "m2s_pair"))))

    def _retrieval(self, out, top_k=RETRIEVAL_TOP_K):
        """All clips' music against all clips' real and generated motion (M2SNet.fuse_pairs), ranked on the host."""
        from .metrics import pair_accuracy, retrieval_stats
        kept = [self.kept[k] for k in sorted(self.kept)]
        T = int(kept[0][1].shape[1])
        for cid, mus, real, gen in kept:
            if int(mus.shape[1]) != T or int(real.shape[2]) != T or int(gen.shape[2]) != T:
                raise ValueError(f"the retrieval scores pair every music with every motion and need one latent length: clip {kept[0][0]} has "
                                 f"{T} frames, clip {cid} has {int(mus.shape[1])}")
        mus, real, gen = (torch.cat([b[i] for b in kept]) for i in (1, 2, 3))
        for name, mot in (("real", real), ("gen", gen)):
            r = self.net.fuse_pairs(mus, mot)
            st = retrieval_stats(r["mean"].cpu().numpy(), top_k)
            out[f"m2s_r_precision_{name}"] = [float(v) for v in st["r_precision"]]
            out[f"m2s_mean_rank_{name}"] = st["mean_rank"]
            out[f"m2s_margin_{name}"] = st["margin"]
            out[f"m2s_pair_accuracy_{name}"] = pair_accuracy(r["above"].cpu().numpy(), r["below"].cpu().numpy(), r["count"].cpu().numpy())
            if name == "gen":
                out["m2s_sync_offdiag_gen"] = st["offdiag_mean"]


def _same_frames(batch, pred, dim_pose, what):
    """The batch's ground truth [B, T, dim_pose] on the poses' device; every clip must have the poses' T frames (ValueError naming
    `what` scores otherwise)."""
    T = pred.shape[1]
    bad = [(cid, np.shape(g)) for cid, g in zip(batch.ids, batch.gts) if int(np.prod(np.shape(g))) != T * dim_pose]
    if bad:
        raise ValueError(f"the {what} scores compare clips of {T} frames, but these ground truths differ: {bad[:4]}")
    return batch.ground_truth(T, dim_pose)


class _MovementScores:
    """`rhythm` (a rhythm.MotionRhythm, or anything with its `psd` and `contour_and_std`): the scores of the M2S-GAN evaluation that look
    at how the motion moves (Contrastive_Stage/M2SGAN_eval.py:100-133, metrics.py) - "rde" and "sce" (the means over the clips of
    "rde_per_clip" and "sce_per_clip", {id: value}; the reference evaluates clip by clip), "sd_gen" and "sd_real".  Needs clips of
    at least 256 frames.  `discriminator` (a discriminator.Discriminator_1DCNN, or anything with its `forward`): "w_distance", the
    mean of D(real) - D(generated); at least 41 frames.  Both run on the device right behind each batch's sampling, on the same
    stream; only the per-clip arrays come back, with the poses, into one pinned row per clip: [psd generated 32 | psd real 32 |
    contour generated W | contour real W | sd generated | sd real] with `rhythm`, then [D(generated) | D(real)] with `discriminator`.
    As with the latents, with `smooth` these are the scores of the SMOOTHED poses."""

    def __init__(self, rhythm, discriminator, ids, T, dim_pose, batch_size):
        if rhythm is not None and T < 256:
            raise ValueError(f"clips of {T} frames: the rhythm scores need at least 256 (Welch's segment)")
        if discriminator is not None and T < 41:
            raise ValueError(f"clips of {T} frames: the critic needs at least 41 (one pooled frame behind its third stage)")
        self.rhythm, self.critic, self.ids, self.dim_pose, self.W = rhythm, discriminator, ids, dim_pose, (T - 60) // 30 + 1
        self.rows = None                 # pinned [clips, columns]: every clip's row, read after the last batch's event

    def enqueue(self, batch, pred):
        B, T = pred.shape[0], pred.shape[1]
        gt = _same_frames(batch, pred, self.dim_pose, "rhythm")
        gen = pred.reshape(B, T, self.dim_pose).contiguous()
        cols = []
        if self.rhythm is not None:
            cg, sg = self.rhythm.contour_and_std(gen)
            cr, sr = self.rhythm.contour_and_std(gt)
            cols += [self.rhythm.psd(gen), self.rhythm.psd(gt), cg, cr, sg.reshape(B, 1), sr.reshape(B, 1)]
        if self.critic is not None:
            cols += [self.critic.forward(gen).reshape(B, 1), self.critic.forward(gt).reshape(B, 1)]
        rows = torch.cat(cols, dim=1)
        if self.rows is None:
            self.rows = torch.empty((len(self.ids), rows.shape[1]), dtype=torch.float32, pin_memory=pred.is_cuda)
        self.rows[batch.first:batch.first + B].copy_(rows, non_blocking=True)

    def finish(self, out, verbose):
        from .metrics import rhythm_density_error, standard_deviation_percentage, strength_contour_error, w_distance
        rows, ids, W, at = self.rows.numpy(), self.ids, self.W, 0
        if self.rhythm is not None:
            psd_g, psd_r, c_g, c_r = rows[:, 0:32], rows[:, 32:64], rows[:, 64:64 + W], rows[:, 64 + W:64 + 2 * W]
            at = 64 + 2 * W
            rde, out["rde"] = rhythm_density_error(psd_r, psd_g)
            sce, out["sce"] = strength_contour_error(c_r, c_g)
            out["rde_per_clip"] = {cid: float(v) for cid, v in zip(ids, rde)}
            out["sce_per_clip"] = {cid: float(v) for cid, v in zip(ids, sce)}
            out["sd_gen"], out["sd_real"] = float(rows[:, at].astype(np.float64).mean()), float(rows[:, at + 1].astype(np.float64).mean())
            at += 2
        if self.critic is not None:
            out["w_distance"] = w_distance(rows[:, at + 1], rows[:, at])
        if verbose:
            print("  ".join(f"{key}: {out[key]}" for key in ("rde", "sce", "sd_gen", "sd_real", "w_distance") if key in out))
            if "sd_gen" in out:
                print(f"sdp: {standard_deviation_percentage(out['sd_gen'], out['sd_real']):.2f}%")


BEAT_COLUMNS = 8      # floats per clip of _BeatScores' rows: [BC, Beat Align, music beats, motion beats] of the sampled poses, then of the ground truth


def _check_music_beats(music_beats, ids):
    """{clip id: 1-D one-hot} covers `ids`, every array 1-D with at least one beat (ValueError naming the clips otherwise) -> the
    arrays as uint8, by clip id."""
    missing = [cid for cid in ids if cid not in music_beats]
    if missing:
        raise ValueError(f"music_beats has no entry for {len(missing)} clip(s): {missing[:8]}{' ...' if len(missing) > 8 else ''}")
    out = {cid: np.asarray(music_beats[cid]) for cid in ids}
    bad = [(cid, a.shape) for cid, a in out.items() if a.ndim != 1 or a.size < 1]
    if bad:
        raise ValueError(f"music_beats holds one 1-D one-hot per clip, but these differ: {bad[:4]}")
    out = {cid: (a != 0).astype(np.uint8) for cid, a in out.items()}
    silent = [cid for cid, a in out.items() if not a.any()]
    if silent:
        raise ValueError(f"no music beat in {len(silent)} clip(s), beat consistency is undefined there: {silent[:8]}{' ...' if len(silent) > 8 else ''}")
    return out


class _BeatScores:
    """`music_beats` ({clip id: 1-D one-hot, nonzero = a beat}: metrics.load_music_beats): beat consistency, the BC column of the
    paper's table (eval_new_metrics.py:253-317) - from SUPPLIED music beats: the reference's get_music_beat is librosa's tracker on
    the clip's mel, a property of the dataset (tools/music_beats_librosa.py).  Each batch's one-hots are padded with zeros to its
    longest and uploaded with it (zeros behind a clip's last beat change nothing: csrc/dc_rhythm.hip, k_beat_scores); the motion's
    beats and their alignment (rhythm.MotionRhythm.motion_beats, .beat_scores) run on the sampled poses and on the ground truth right
    behind the sampling, on the same stream (on `rhythm` when it can, else on a MotionRhythm of the poses' device), and the [B, 2]
    scores and counts come back with the poses, into one pinned row of BEAT_COLUMNS per clip.  Adds "bc_gen", "bc_real" (the means
    over the clips of "bc_gen_per_clip", "bc_real_per_clip", {id: value}), "beat_align_gen" and "beat_align_real" (the other
    direction; nan when a clip has no motion beat).  `beat_stride`: 1 compares the index lists as they are, as the reference does
    (90-fps mel frames against 30-fps motion frames; the paper's numbers); 3 puts both on one clock.  A clip id without an entry, an
    entry that is not 1-D or has no beat: ValueError before anything is sampled.  With `smooth` the scores are those of the SMOOTHED
    poses."""

    def __init__(self, music_beats, beat_stride, rhythm, ids, T, dim_pose, batch_size):
        if int(beat_stride) < 1:
            raise ValueError(f"beat_stride must be >= 1, got {beat_stride}")
        self.beats, self.stride, self.ids, self.dim_pose = _check_music_beats(music_beats, ids), int(beat_stride), ids, dim_pose
        self.rhythm = rhythm if hasattr(rhythm, "motion_beats") and hasattr(rhythm, "beat_scores") else None
        self.rows = None                 # pinned [clips, BEAT_COLUMNS]: every clip's row, read after the last batch's event

    def enqueue(self, batch, pred):
        B, T = pred.shape[0], pred.shape[1]
        if self.rhythm is None:
            from .rhythm import MotionRhythm
            self.rhythm = MotionRhythm(pred.device)
        if self.rows is None:
            self.rows = torch.empty((len(self.ids), BEAT_COLUMNS), dtype=torch.float32, pin_memory=pred.is_cuda)
        gt = _same_frames(batch, pred, self.dim_pose, "beat")
        mus = np.zeros((B, max(self.beats[cid].size for cid in batch.ids)), np.uint8)
        for i, cid in enumerate(batch.ids):
            mus[i, :self.beats[cid].size] = self.beats[cid]
        mus = torch.from_numpy(mus)
        if pred.is_cuda:
            mus = mus.pin_memory().to(pred.device, non_blocking=True)
        cols = []
        for x in (pred.reshape(B, T, self.dim_pose).contiguous(), gt):
            scores, counts = self.rhythm.beat_scores(self.rhythm.motion_beats(x), mus, music_stride=self.stride, counts=True)
            cols += [scores, counts.to(torch.float32)]           # (counts are at most a clip's frames: exact in fp32)
        self.rows[batch.first:batch.first + B].copy_(torch.cat(cols, dim=1), non_blocking=True)

    def finish(self, out, verbose):
        from .metrics import beat_consistency
        rows = self.rows.numpy()
        for name, at in (("gen", 0), ("real", 4)):
            out[f"bc_{name}"], out[f"bc_{name}_per_clip"] = beat_consistency(rows[:, at:at + 2], rows[:, at + 2:at + 4], self.ids)
            out[f"beat_align_{name}"] = beat_consistency(rows[:, at:at + 2], rows[:, at + 2:at + 4], self.ids, column=1)[0]
        if verbose:
            print("  ".join(f"{key}: {out[key]}" for key in ("bc_gen", "bc_real", "beat_align_gen", "beat_align_real")))


def _enqueue_scores(families, batch):
    """Every active family's device work for `batch`, on the current stream and in the families' order -> what they left to do on
    the host once the batch has landed (zero-argument callables)."""
    return [fn for fn in [f.enqueue(batch, batch.pred) for f in families] if fn is not None]


class _Scorer:
    """Per-clip MSE of a batch (eval_new.py:124-131) on a background thread, behind the event that says the batch's poses have
    landed in the pinned buffer - the main thread is enqueueing the next batch meanwhile.  `landed`: what the score families left
    to do on the host once the batch is there (their `enqueue`'s return values), run behind the MSEs."""

    def __init__(self, dim_pose):
        import queue
        self.dim_pose = dim_pose
        self.q = queue.Queue()
        self.done = {}                  # batch -> [(clip id, mse)] | exception
        self.cv = threading.Condition()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            job = self.q.get()
            if job is None:
                return
            k, bid, gts, pred_h, event, _keep, landed = job
            try:
                if event is not None:
                    event.synchronize()
                pred = pred_h.numpy()
                if not np.isfinite(pred).all():
                    raise FloatingPointError(f"non-finite poses in batch {k}")
                res = _clip_mses(bid, gts, pred, self.dim_pose)
                for fn in landed:
                    fn()
            except BaseException as e:
                res = e
            with self.cv:
                self.done[k] = res
                self.cv.notify_all()

    def submit(self, k, bid, gts, pred_h, event, keep, landed=()):
        self.q.put((k, bid, gts, pred_h, event, keep, landed))

    def wait_for(self, k, reraise=True):
        """Blocks until batch k has been scored (k < 0: nothing to wait for); returns its [(clip id, mse)] or raises its error.
        reraise=False only waits (the sampling loop frees a pinned slot with it: a failed batch is dealt with when the results are
        collected, where a non-finite one is sampled again the checked way)."""
        if k < 0:
            return None
        with self.cv:
            self.cv.wait_for(lambda: k in self.done)
            res = self.done[k]
        if isinstance(res, BaseException):
            if reraise:
                raise res
            return None
        return res

    def close(self):
        self.q.put(None)


def evaluate_dataset(trainer, root, dim_pose=26, batch_size=32, limit=None, seed=0, smooth=False, verbose=True, motion_encoder=None,
                     diversity_seed=0, m2snet=None, guidance_scale=None, steps=None, spacing="uniform", solver="ddim", rhythm=None,
                     discriminator=None, music_beats=None, beat_stride=1, retrieval=False):
    """Samples every clip under `root` and returns {"per_clip": {id: mse}, "total_loss", "final_mse", "clips",
    "seconds", "frames_per_s"}.  Clip i (in sorted order) starts from noise seeded with (seed, i), so the result
    does not depend on batch_size or on the number of ranks.

    Each further score is a family of its own, switched on by its argument(s) and described at its class; without them the result
    and the work done are exactly what they were before the family existed, and each family refuses what it cannot score before
    anything is sampled:
    `motion_encoder`, `diversity_seed`: the latent scores SE, FGD, feat_dist and diversity (_LatentScores).
    `m2snet`, `retrieval`: M2SNet's synchronisation score, and every music ranked against every motion (_SyncScores).
    `rhythm`, `discriminator`: RDE, SCE, SD and the critic's W-distance (_MovementScores).
    `music_beats`, `beat_stride`: beat consistency and Beat Align from supplied music beats (_BeatScores).

    `guidance_scale`: None, or the classifier-free guidance scale every batch is sampled with (generate_music_motion).
    `steps`, `spacing`, `solver`: every batch is sampled on `steps` of the schedule's timesteps (generate_music_motion; the defaults
    walk every timestep, as before).

    The host stays out of the GPU's way: batch k + 1's files and noise are prepared, and batch k - 1's MSEs computed, on
    background threads while batch k is sampled; the active families enqueue their device work right behind the batch's sampling, in
    the order above, and the poses come back behind it through a pinned double buffer and an event, not a stream synchronisation;
    the sampler's per-loop numeric check (a status read that waits for the GPU) is replaced by a finiteness check of the poses on
    the scoring thread, and a batch that fails it is sampled again the checked way (which is where precision="auto" falls back to
    the bf16-range mode) and handed to the same families again, whose rows for it are overwritten.  At most two batches are in
    flight."""
    gkw = {} if guidance_scale is None else {"guidance_scale": float(guidance_scale)}      # (None: the trainer is called as before)
    if steps is not None or solver != "ddim":
        gkw.update(steps=steps, spacing=spacing, solver=solver)
    sync = _SyncScores(m2snet, retrieval, dim_pose) if m2snet is not None or retrieval else None
    ids, mel_shape, T, nb = _open_dataset(root, limit, batch_size)
    facts = (ids, T, dim_pose, batch_size)
    families = [f for f in (_LatentScores(motion_encoder, diversity_seed, *facts) if motion_encoder is not None else None, sync,
                            _MovementScores(rhythm, discriminator, *facts) if rhythm is not None or discriminator is not None else None,
                            _BeatScores(music_beats, beat_stride, rhythm, *facts) if music_beats is not None else None) if f is not None]
    pf = _Prefetcher(root, ids, batch_size, mel_shape, noise=(seed, T, dim_pose))
    pf.start(0)
    scorer = _Scorer(dim_pose)
    enc = getattr(trainer, "encoder", None)
    serial = bool(os.environ.get("DC_EVAL_SERIAL"))      # A/B switch (tools/time_evaluate.py): round 4's behaviour - the status read's stream
    checked = None if serial else getattr(enc, "check_numerics", None)      # synchronisation and the MSEs between two batches
    dev = getattr(trainer, "device", None)
    on_gpu = dev is not None and torch.device(dev).type == "cuda"
    out_h = [None, None]
    slot_free = [None, None]             # event: the GPU has consumed the slot's pinned mel / noise buffers
    results = {}
    exchange_before = getattr(enc, "combine_exchange", None)
    ev_first = ev_last = None            # completion events of the first and the last batch: the GPU's own steady-state period
    n_after_first = 0
    waits = {"loader": 0.0, "enqueue": 0.0, "scorer": 0.0}      # where the main thread spent its time (seconds): waiting for the next
    t0 = time.perf_counter()                                    # batch's files, inside generate_music_motion, waiting for batch k - 2's scores
    try:
        if checked:
            enc.check_numerics = False   # (see above: checked on the scoring thread instead)
            # ... which cannot see the one failure that leaves finite poses: a timed-out combine exchange of the small-batch layer kernel
            # (dc_ddim.h, DC_STATUS_TIMEOUT; possible only on a GPU shared with other work).  Unchecked loops run the form without it.
            enc.combine_exchange = False
        for k in range(nb):
            tw = time.perf_counter()
            bid, mel, gts = pf.take()
            waits["loader"] += time.perf_counter() - tw
            noise = pf.noise
            if k + 1 < nb:
                pf.start(k + 1, after=slot_free[(k + 1) & 1])
            if on_gpu:
                noise = noise.to(dev, non_blocking=True)      # (a blocking copy on the default stream would wait for the previous batch)
            # [B, T, dim_pose] on the device; smoothing (tools/visualization.py:126) happens in the sampling loop's final write
            tw = time.perf_counter()
            pred = trainer.generate_music_motion(mel, dim_pose, noise=noise, smooth=19 if smooth else None, **gkw)
            waits["enqueue"] += time.perf_counter() - tw
            tw = time.perf_counter()
            scorer.wait_for(k - 2, reraise=False)             # the pinned pose buffer of this slot has been scored (errors: collected below)
            waits["scorer"] += time.perf_counter() - tw
            s = k & 1
            if out_h[s] is None or out_h[s].shape[0] < pred.shape[0] or out_h[s].shape[1:] != pred.shape[1:]:
                out_h[s] = torch.empty((batch_size,) + tuple(pred.shape[1:]), dtype=pred.dtype, pin_memory=pred.is_cuda)     # pageable D2H costs ~3x the copy
            ph = out_h[s][:pred.shape[0]]
            landed = _enqueue_scores(families, _Batch(k, k * batch_size, bid, mel, gts, pred, s))
            ph.copy_(pred, non_blocking=True)
            ev = None
            if pred.is_cuda:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                slot_free[s] = ev
                ev_first = ev_first or ev
                ev_last, n_after_first = ev, (n_after_first + len(bid) if ev_first is not ev else 0)
            scorer.submit(k, bid, gts, ph, ev, pred, landed)
            if serial:
                scorer.wait_for(k, reraise=False)
        for k in range(nb):
            try:
                results[k] = scorer.wait_for(k)
            except FloatingPointError:
                if not checked:
                    raise
                # the checked path (status read, precision="auto" fallback) for this batch alone
                enc.check_numerics = True
                pf2 = _Prefetcher(root, ids, batch_size, mel_shape, noise=(seed, T, dim_pose))
                pf2._load_batch(k, 0)
                bid, mel, gts = pf2.result
                pred = trainer.generate_music_motion(mel, dim_pose, noise=pf2.noise, smooth=19 if smooth else None, **gkw)
                # no pinned slot for this batch: later ones may still be queued on the scoring thread and read both.  What the families
                # enqueue goes to their per-clip rows and per-batch entries, and the poses' blocking copy waits for all of it
                landed = _enqueue_scores(families, _Batch(k, k * batch_size, bid, mel, gts, pred, None))
                results[k] = _clip_mses(bid, gts, pred.cpu().numpy(), dim_pose)
                for fn in landed:
                    fn()
                enc.check_numerics = False
    finally:
        scorer.close()
        if checked:
            enc.check_numerics = checked
            enc.combine_exchange = exchange_before
    dt = time.perf_counter() - t0
    per_clip, total_loss = {}, 0.0
    for k in range(nb):
        for cid, cur in results[k]:
            per_clip[cid] = float(cur)
            total_loss += cur
            if verbose:
                print("cur_loss: ", cur)
                print("total_loss: ", total_loss)
    final_mse = total_loss / len(ids)
    if verbose:
        print("final total loss: ", total_loss)
        print("final_mse: ", final_mse)
    out = {"per_clip": per_clip, "total_loss": float(total_loss), "final_mse": float(final_mse), "clips": len(ids),
           "seconds": dt, "frames_per_s": len(ids) * T / dt, "main_thread_s": {k: round(v, 4) for k, v in waits.items()}}
    if ev_first is not None and ev_last is not ev_first:
        # clips of batches 2 .. n over the time between the completion of batch 1 and of batch n ON THE GPU: the pipeline's rate
        # without the two things nothing can hide (the first batch's load before any GPU work, the last batch's scoring after it)
        out["steady_frames_per_s"] = n_after_first * T / (ev_first.elapsed_time(ev_last) * 1e-3)
    for f in families:
        f.finish(out, verbose)
    return out


NEGATIVE_STRATEGIES = {"easy": 1, "hard": 2, "super_hard": 2}      # strategy -> uniform draws PairBuilder.build_pairs takes for it


def negative_windows(strategy, u, sample_length, clip_length):
    """The index ranges PairBuilder.build_pairs (Contrastive_Stage/utils/train_utils.py:27-89) cuts for `strategy` from the uniform
    draws `u` (its np.random.rand() values, in its order): {"music_1", "motion_1", "music_2", "motion_2"} -> (start, end), music at
    90 Hz, motion at 30 Hz, with the reference's float64 expressions and int() truncations.  `sample_length`, `clip_length`: seconds.
    For "easy" the second window is the first (the negative is the batch flipped)."""
    if strategy not in NEGATIVE_STRATEGIES:
        raise ValueError(f"strategy must be one of {sorted(NEGATIVE_STRATEGIES)}, got {strategy!r}")
    if clip_length > sample_length / 3:
        raise ValueError(f"clip_length {clip_length} must be at most sample_length / 3 = {sample_length / 3} (PairBuilder's condition)")
    u = [float(v) for v in np.atleast_1d(np.asarray(u, np.float64))]
    if len(u) != NEGATIVE_STRATEGIES[strategy]:
        raise ValueError(f"{strategy} takes {NEGATIVE_STRATEGIES[strategy]} uniform draw(s), got {len(u)}")
    L, c = sample_length, clip_length
    if strategy == "easy":
        start_1 = u[0] * (L - c)
        start_2 = start_1
    elif strategy == "hard":
        start_1 = u[0] * (L - c - 10)
        start_2 = start_1 + 10 + u[1] * (L - c - start_1 - 10)
    else:
        start_1 = u[0] * (L - c - 5)
        start_2 = u[1] * (5 - 0.5) + start_1
    end_1, end_2 = start_1 + c, start_2 + c
    return {"music_1": (int(start_1 * 90), int(end_1 * 90)), "motion_1": (int(start_1 * 30), int(end_1 * 30)),
            "music_2": (int(start_2 * 90), int(end_2 * 90)), "motion_2": (int(start_2 * 30), int(end_2 * 30))}


def sync_negatives(m2snet, mel, motion, sample_length, clip_length, draws):
    """The reference's own protocol for one batch (Contrastive_Stage/M2SNet_eval.py:58-92): for each of "easy", "hard" and
    "super_hard", PairBuilder's windows (negative_windows) from the caller's uniform draws, `m2snet(mel_1, motion_1)` as the matched and
    `m2snet(mel_1, motion_2)` as the mismatched predictions, and metrics.sync_stats of the two:
    {strategy: {"sync", "non_sync", "accuracy"}}.  mel [B, >= 90 sample_length, 128], motion [B, >= 30 sample_length, 13, 2] (or
    [.., 26]); `draws`: {strategy: its draws} (one for easy, two for the others; strategies left out are not scored).  For "easy" the
    negative is the batch flipped.  Where the windows' frame counts are ones the reference's torch.cat fails on (the music window's
    latent frames differ from the motion window's frames), ValueError.

        u = np.random.RandomState(0).rand(5)
        sync_negatives(net, mel, motion, 60, 20, {"easy": u[:1], "hard": u[1:3], "super_hard": u[3:]})
    """
    from .metrics import sync_stats
    mel, motion = torch.as_tensor(mel), torch.as_tensor(motion)
    out = {}
    for strategy in NEGATIVE_STRATEGIES:
        if strategy not in draws:
            continue
        w = negative_windows(strategy, draws[strategy], sample_length, clip_length)
        mel_1 = mel[:, w["music_1"][0]:w["music_1"][1]]
        motion_1 = motion[:, w["motion_1"][0]:w["motion_1"][1]]
        motion_2 = motion_1.flip(0) if strategy == "easy" else motion[:, w["motion_2"][0]:w["motion_2"][1]]
        Tm = int(mel_1.shape[1])
        for what, x in (("motion_1", motion_1), ("motion_2", motion_2)):
            if Tm < 1 or (Tm - 1) // 3 + 1 != int(x.shape[1]):
                raise ValueError(f"{strategy}: the music window {w['music_1']} has {Tm} mel frames = {(Tm - 1) // 3 + 1 if Tm else 0} latent "
                                 f"frames, {what} has {int(x.shape[1])} (the reference's torch.cat fails on this draw)")
        out[strategy] = sync_stats(m2snet(mel_1.contiguous(), motion_1.contiguous()), m2snet(mel_1.contiguous(), motion_2.contiguous()))
    return out


def _encoded_batches(trainer, root, ids, batch_size, mel_shape, T, nb):
    """The walk of the drivers that score without sampling: starts loading batch 0 at once and returns a generator of (k, the batch's
    clip ids, x0 [B, T, 26] on the trainer's device, xf_proj, xf_out) - the batch's music encoded once (encode_music) while batch
    k + 1's files are read into the other pinned slot, which is free once the GPU has consumed it."""
    pf = _Prefetcher(root, ids, batch_size, mel_shape)
    pf.start(0)
    dev = trainer.device

    def walk():
        slot_free = [None, None]
        for k in range(nb):
            bid, mel, gts = pf.take()
            if k + 1 < nb:
                pf.start(k + 1, after=slot_free[(k + 1) & 1])
            bad = [(cid, np.shape(g)) for cid, g in zip(bid, gts) if int(np.prod(np.shape(g))) != T * 26]
            if bad:
                raise ValueError(f"the music gives {T} frames, but these motions differ: {bad[:4]}")
            x0 = torch.from_numpy(np.ascontiguousarray(np.stack([np.reshape(g, (T, 26)) for g in gts]), np.float32)).to(dev)
            with torch.no_grad():
                xf_proj, xf_out = trainer.encoder.encode_music(mel, dev)
            if torch.device(dev).type == "cuda":
                slot_free[k & 1] = torch.cuda.Event()
                slot_free[k & 1].record()
            yield k, bid, x0, xf_proj, xf_out
    return walk()


def validation_grid(num_timesteps, k):
    """The noise levels of a `k`-point loss curve: unique(round(linspace(0, S - 1, k))), increasing."""
    S, k = int(num_timesteps), int(k)
    if not 1 <= k:
        raise ValueError(f"the grid needs at least one timestep, got {k}")
    return sorted({int(v) for v in np.floor(np.linspace(0, S - 1, k) + 0.5)})


_VAL_SCALARS = ("loss", "loss_mot_rec", "loss_mot_feat", "loss_velocity", "loss_velocity_elbow", "loss_velocity_head",
                "loss_velocity_body", "velocity_elbow", "mse")


def validation_dataset(trainer, root, timesteps=None, batch_size=32, seed=0, motion_encoder=None, limit=None):
    """Scores a checkpoint by its held-out DENOISING losses (DDPMTrainer.validation_losses) over every clip under `root` - one
    model evaluation per clip and noise level, no sampling loop.
    `timesteps`: an int K - the grid validation_grid(S, K), every clip evaluated at every grid timestep; a list - those timesteps;
    None - the training protocol, one uniform timestep per clip (drawn on the host from `seed`, by clip index).
    Each batch's music is encoded once and its conditioning pre-pass set once, then reused across the grid.  Noise comes from the
    library's device stream with iteration = grid index and first_element = clip_index * T * 26, so a clip's draw - and with it
    every number here - does not depend on batch_size or order.  The scalars are combined on the host from the per-clip terms of
    the WHOLE data set (metrics.denoising_loss_scalars).
    Returns {"clips", "timesteps" (the grid, or None), "per_timestep": [{"t": grid timestep or None, "loss", "loss_mot_rec",
    "loss_mot_feat" (None without `motion_encoder`), "loss_velocity", "loss_velocity_elbow", "loss_velocity_head",
    "loss_velocity_body", "velocity_elbow", "mse", "feat_included"}], "average": the same scalars averaged over the grid,
    "evaluations" (model evaluations per clip), "seconds"}."""
    from .metrics import denoising_loss_scalars
    ids, mel_shape, T, nb = _open_dataset(root, limit, batch_size)
    S = int(trainer.diffusion.num_timesteps)
    if timesteps is None:
        grid, drawn = None, np.random.RandomState(int(seed) & 0xffffffff).choice(S, size=(len(ids),), p=np.ones(S) / S)
    else:
        grid = validation_grid(S, timesteps) if np.ndim(timesteps) == 0 else [int(v) for v in timesteps]
        if not grid or any(not 0 <= v < S for v in grid):
            raise ValueError(f"timesteps must be inside [0, {S}), got {grid}")
    batches = _encoded_batches(trainer, root, ids, batch_size, mel_shape, T, nb)
    n_levels = 1 if grid is None else len(grid)
    terms = [[] for _ in range(n_levels)]
    feats = [[] for _ in range(n_levels)]
    t0 = time.perf_counter()
    for k, bid, x0, xf_proj, xf_out in batches:
        B, first = len(bid), k * batch_size
        for gi in range(n_levels):
            t = drawn[first:first + B] if grid is None else np.full(B, grid[gi], np.int64)
            r = trainer._validation_batch(xf_proj, xf_out, x0, np.full(B, T, np.int64), t, noise_seed=(seed, gi, first * T * 26),
                                          motion_encoder=motion_encoder)
            terms[gi].append(r["terms"])
            if motion_encoder is not None:
                feats[gi].append(r["latent_l1"])
    dt = time.perf_counter() - t0
    rows = []
    for gi in range(n_levels):
        sc = denoising_loss_scalars(np.concatenate(terms[gi]), np.full(len(ids), T), np.concatenate(feats[gi]) if feats[gi] else None)
        rows.append({"t": None if grid is None else grid[gi], **sc})
    avg = {key: (None if rows[0][key] is None else float(np.mean([r[key] for r in rows]))) for key in _VAL_SCALARS}
    avg["feat_included"] = rows[0]["feat_included"]
    return {"clips": len(ids), "timesteps": grid, "per_timestep": rows, "average": avg, "evaluations": n_levels, "seconds": dt}


def bound_grid(num_timesteps, k):
    """The `k` evenly spaced timesteps of a --bpd table, decreasing; 0 and S - 1 are always among them (k >= 2; k = 1 gives [S - 1])."""
    S, k = int(num_timesteps), int(k)
    if not 1 <= k:
        raise ValueError(f"the table needs at least one timestep, got {k}")
    if k == 1:
        return [S - 1]
    return sorted({int(v) for v in np.floor(np.linspace(0, S - 1, k) + 0.5)} | {0, S - 1}, reverse=True)


def bound_dataset(trainer, root, timesteps=None, batch_size=32, seed=0, limit=None):
    """Scores a checkpoint by its VARIATIONAL BOUND in bits per dimension (DDPMTrainer.bound_bpd, GaussianDiffusion.calc_bpd_loop) over
    every clip under `root`: one model evaluation per clip and timestep, no sampling loop.
    `timesteps`: an int K - the table bound_grid(S, K); a list - those timesteps; None - every timestep of the schedule, which is what
    the total needs.  Each batch's music is encoded once.  Step t's noise is the library's device draw (seed + batch index,
    iteration = t).
    Returns {"clips", "timesteps" (decreasing), "total_bpd" (mean over the clips; None for a subset), "prior_bpd",
    "per_timestep": [{"t", "vb", "xstart_mse", "mse"}] (means over the clips), "evaluations" (model evaluations per clip), "seconds"}."""
    ids, mel_shape, T, nb = _open_dataset(root, limit, batch_size)
    S = int(trainer.diffusion.num_timesteps)
    grid = None
    if timesteps is not None:
        grid = bound_grid(S, timesteps) if np.ndim(timesteps) == 0 else sorted({int(v) for v in timesteps}, reverse=True)
        if not grid or any(not 0 <= v < S for v in grid):
            raise ValueError(f"timesteps must be inside [0, {S}), got {grid}")
    batches = _encoded_batches(trainer, root, ids, batch_size, mel_shape, T, nb)
    rows = []
    t0 = time.perf_counter()
    for k, bid, x0, xf_proj, xf_out in batches:
        rows.append(trainer._bound_batch(xf_proj, xf_out, x0, np.full(len(bid), T, np.int64), grid, int(seed) + k))
    dt = time.perf_counter() - t0
    ts = rows[0]["timesteps"]
    cat = {key: np.concatenate([r[key] for r in rows]) for key in ("vb", "xstart_mse", "mse", "prior_bpd")}
    total = None if grid is not None else float(np.concatenate([r["total_bpd"] for r in rows]).mean())
    return {"clips": len(ids), "timesteps": ts, "total_bpd": total, "prior_bpd": float(cat["prior_bpd"].mean()),
            "per_timestep": [{"t": t, "vb": float(cat["vb"][:, i].mean()), "xstart_mse": float(cat["xstart_mse"][:, i].mean()),
                              "mse": float(cat["mse"][:, i].mean())} for i, t in enumerate(ts)],
            "evaluations": len(ts), "seconds": dt}


def _evaluation_encoders(args, dev):
    """(motion encoder for --metrics | None, M2SNet for --sync | None) as main's flags ask for them."""
    menc = None
    if args.metrics or args.m2snet:
        from .motion_encoder import MotionEncoder_STGCN, load_m2snet
        if args.m2snet:
            menc = load_m2snet(args.m2snet, dev)
        else:
            from .synthetic import synthetic_motion_encoder_state_dict
            menc = MotionEncoder_STGCN(dev).load_state_dict(synthetic_motion_encoder_state_dict())
            print("--metrics without --m2snet: the motion encoder has seeded synthetic weights, so SE / FGD / feat_dist / diversity "
                  "only check the pipeline, they say nothing about the motions")
    m2s = None
    if args.sync:
        from .m2snet import M2SNet, load_m2snet_full
        if args.m2snet:
            m2s = load_m2snet_full(args.m2snet, dev)
        else:
            from .synthetic import synthetic_m2snet_state_dict
            m2s = M2SNet(dev).load_state_dict(synthetic_m2snet_state_dict())
            print("--sync without --m2snet: M2SNet has seeded synthetic weights, so the m2s_* scores only check the pipeline")
    return menc, m2s


def _movement_scorers(args, dev):
    """(MotionRhythm for --rhythm | None, the critic for --discriminator | None) as main's flags ask for them."""
    rh = disc = None
    if args.rhythm:
        from .rhythm import MotionRhythm
        rh = MotionRhythm(dev)
    if args.discriminator:
        from .discriminator import load_m2sgan_discriminator
        disc = load_m2sgan_discriminator(args.discriminator, dev)
    return rh, disc


def _music_beats(args):
    """{clip id: one-hot} of --beats for the clips main is about to evaluate | None."""
    if not args.beats:
        return None
    from .metrics import load_music_beats
    ids = list_clips(args.data_root)
    return load_music_beats(args.beats, ids if args.limit is None else ids[:int(args.limit)])


def _baseline_main(args, dev):
    """--baseline_generator: evaluate_dataset on the M2S-GAN generator (generator.GeneratorBaseline), one JSON line.  The loader picks
    the decoder - the TCN or the CNN-LSTM baseline's BiLSTM - from the checkpoint's keys."""
    import json
    from .generator import GeneratorBaseline, load_m2sgan_generator
    gen = load_m2sgan_generator(args.baseline_generator, dev)
    menc, m2s = _evaluation_encoders(args, dev)
    rh, disc = _movement_scorers(args, dev)
    r = evaluate_dataset(GeneratorBaseline(gen), args.data_root, 26, args.batch_size, args.limit, args.seed, args.smooth, verbose=False,
                         motion_encoder=menc, diversity_seed=args.diversity_seed, m2snet=m2s, rhythm=rh, discriminator=disc,
                         music_beats=_music_beats(args), beat_stride=args.beat_stride, retrieval=args.retrieval)
    print(json.dumps({"model": "m2sgan", **r}))
    return 0


def main(argv=None):
    """python -m diffusion_conductor_amd.evaluate --data_root <dir> [--model latest.tar] [--batch_size 32]"""
    import argparse
    import types
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_root", required=True, help="directory of <id>/mel.npy + <id>/motion.npy (the reference's split dirs)")
    ap.add_argument("--model", default=None, help="checkpoint (.tar with an 'encoder' state_dict, ddpm_trainer.py:303-319); "
                                                  "omitted = seeded synthetic weights")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--diffusion_steps", type=int, default=1000, help="reference default train_options.py:10")
    ap.add_argument("--gpu_id", type=int, default=0)
    ap.add_argument("--limit", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--smooth", action="store_true", help="Savitzky-Golay smoothing as tools/visualization.py:126")
    ap.add_argument("--no_eff", action="store_true")
    ap.add_argument("--metrics", action="store_true", help="also SE, FGD, feat_dist and diversity on the ST-GCN latents (metrics.py)")
    ap.add_argument("--m2snet", default=None, help="M2SNet checkpoint for --metrics (DataParallel state_dict, keys "
                                                   "module.motion_encoder.*) and --sync (every key); omitted = seeded synthetic weights")
    ap.add_argument("--diversity_seed", type=int, default=0)
    ap.add_argument("--guidance_scale", type=float, default=None, help="classifier-free guidance scale of the sampling loops (omitted: no guidance)")
    ap.add_argument("--steps", type=int, default=None, help="sample on this many of the schedule's timesteps (omitted: all of them)")
    ap.add_argument("--spacing", default="uniform", choices=["uniform", "logsnr"], help="how --steps picks them (use logsnr with dpmpp2m)")
    ap.add_argument("--solver", default="ddim", choices=["ddim", "dpmpp2m"], help="first-order DDIM or the second-order multistep update")
    ap.add_argument("--sync", action="store_true", help="also M2SNet's synchronisation score of the sampled poses against the music "
                                                        "(m2snet.py; every entry of --m2snet, or seeded synthetic weights)")
    ap.add_argument("--retrieval", action="store_true", help="also rank every clip's music against every clip's real and generated motion "
                                                             "with M2SNet: R-precision, mean rank, margin and pair accuracy (implies --sync)")
    ap.add_argument("--val_loss", action="store_true", help="score the checkpoint by its held-out denoising losses instead of sampling it: "
                                                            "one JSON line, no sampling loop (validation_dataset)")
    ap.add_argument("--val_timesteps", type=int, default=None, help="--val_loss on a grid of this many noise levels (omitted: one uniform "
                                                                    "timestep per clip, the training protocol)")
    ap.add_argument("--bpd", action="store_true", help="score the checkpoint by its variational bound in bits per dimension instead of "
                                                       "sampling it: one JSON line, one model evaluation per clip and timestep (bound_dataset)")
    ap.add_argument("--bpd_timesteps", type=int, default=None, help="--bpd on this many evenly spaced timesteps, 0 and S - 1 among them "
                                                                    "(omitted: every timestep, which the total needs)")
    ap.add_argument("--rhythm", action="store_true", help="also RDE, SCE and the standard deviations of the sampled and the real motion "
                                                          "(M2SGAN_eval.py:100-133; rhythm.py, metrics.py)")
    ap.add_argument("--discriminator", default=None, help="M2S-GAN critic checkpoint (a plain state_dict, M2SGAN_eval.py:453): also the "
                                                          "W-distance D(real) - D(generated) (discriminator.py)")
    ap.add_argument("--baseline_generator", default=None, help="score the M2S-GAN generator of this checkpoint (a plain state_dict, "
                                                               "M2SGAN_eval.py:451) instead of the denoiser: the same evaluation, one JSON "
                                                               "line with \"model\": \"m2sgan\" (generator.py).  Either flavour loads: the "
                                                               "TCN decoder (tcn.TCN.* keys) or the CNN-LSTM baseline's BiLSTM decoder "
                                                               "(tcn.LSTM.* keys)")
    ap.add_argument("--beats", default=None, help=".npz of music beats, one 1-D one-hot per clip id (tools/music_beats_librosa.py): also "
                                                  "beat consistency and Beat Align of the sampled and the real motion (rhythm.py, metrics.py)")
    ap.add_argument("--beat_stride", type=int, default=1, help="music frames per motion frame for --beats: 1 compares the beat indices as "
                                                               "they are, as the reference does; 3 puts 90-fps mel frames and 30-fps poses "
                                                               "on one clock")
    args = ap.parse_args(argv)
    if args.retrieval:
        args.sync = True
    if args.baseline_generator:
        clash = [f for f, on in (("--model", args.model), ("--val_loss", args.val_loss), ("--guidance_scale", args.guidance_scale is not None),
                                 ("--steps", args.steps is not None), ("--solver", args.solver != "ddim"), ("--spacing", args.spacing != "uniform"),
                                 ("--no_eff", args.no_eff), ("--diffusion_steps", args.diffusion_steps != 1000)) if on]
        if clash:
            ap.error(f"--baseline_generator scores the M2S-GAN generator, one forward pass per clip: {', '.join(clash)} belong"
                     f"{'s' if len(clash) == 1 else ''} to the diffusion denoiser and cannot be combined with it")
    if args.val_loss and (args.rhythm or args.discriminator):
        ap.error("--val_loss scores the checkpoint without sampling it: --rhythm and --discriminator score sampled motion and cannot be "
                 "combined with it")
    if args.val_loss and (args.beats or args.beat_stride != 1):
        ap.error("--val_loss scores the checkpoint without sampling it: --beats and --beat_stride score sampled motion and cannot be "
                 "combined with it")
    if args.bpd_timesteps is not None and not args.bpd:
        ap.error("--bpd_timesteps picks the timesteps of --bpd and says nothing without it")
    if args.bpd:
        clash = [f for f, on in (("--val_loss", args.val_loss), ("--baseline_generator", args.baseline_generator), ("--rhythm", args.rhythm),
                                 ("--discriminator", args.discriminator), ("--beats", args.beats), ("--beat_stride", args.beat_stride != 1),
                                 ("--metrics", args.metrics), ("--sync", args.sync), ("--smooth", args.smooth),
                                 ("--guidance_scale", args.guidance_scale is not None), ("--steps", args.steps is not None),
                                 ("--solver", args.solver != "ddim"), ("--spacing", args.spacing != "uniform")) if on]
        if clash:
            ap.error(f"--bpd scores the checkpoint without sampling it: {', '.join(clash)} cannot be combined with it")
        if args.bpd_timesteps is not None and args.bpd_timesteps < 1:
            ap.error("--bpd_timesteps must be >= 1")
    if args.beat_stride != 1 and not args.beats:
        ap.error("--beat_stride places the music beats of --beats and says nothing without it")
    if args.beat_stride < 1:
        ap.error("--beat_stride must be >= 1")
    from . import DDPMTrainer, MotionTransformer
    dev = torch.device("cuda", args.gpu_id)
    torch.cuda.set_device(dev)
    if args.baseline_generator:
        return _baseline_main(args, dev)
    enc = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, no_clip=True, no_eff=args.no_eff,
                            device=dev, music_model_path=None)
    opt = types.SimpleNamespace(device=dev, diffusion_steps=args.diffusion_steps, is_train=False)
    tr = DDPMTrainer(opt, enc)
    if args.model:
        tr.load(args.model)
    else:
        from .synthetic import synthetic_state_dict
        enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict().items()}, strict=True)
    tr.eval_mode()
    if args.bpd:
        import json
        print(json.dumps(bound_dataset(tr, args.data_root, args.bpd_timesteps, args.batch_size, args.seed, limit=args.limit)))
        return 0
    menc, m2s = _evaluation_encoders(args, dev)
    if args.val_loss:
        import json
        r = validation_dataset(tr, args.data_root, args.val_timesteps, args.batch_size, args.seed, motion_encoder=menc, limit=args.limit)
        print(json.dumps(r))
        return 0
    rh, disc = _movement_scorers(args, dev)
    r = evaluate_dataset(tr, args.data_root, 26, args.batch_size, args.limit, args.seed, args.smooth, motion_encoder=menc,
                         diversity_seed=args.diversity_seed, m2snet=m2s, guidance_scale=args.guidance_scale,
                         steps=args.steps, spacing=args.spacing, solver=args.solver, rhythm=rh, discriminator=disc,
                         music_beats=_music_beats(args), beat_stride=args.beat_stride, retrieval=args.retrieval)
    print(f"{r['clips']} clips in {r['seconds']:.2f} s = {r['frames_per_s']:.0f} frames/s")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
