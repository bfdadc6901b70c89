"""Shared pieces of the retrieval tests (test_host_retrieval.py, test_gpu_retrieval.py): the order in which csrc/dc_m2snet.hip's
k_m2s_pairs / k_m2s_pairs_reduce sum a pair's probabilities, restated in numpy fp32; the retrieval keys of evaluate_dataset from
plain matrices; a sampler stand-in whose poses depend on the clip's music alone."""
import numpy as np
import torch

from helpers_m2snet import fixture_inputs

from diffusion_conductor_amd import metrics

TILE = 32


def reduction_depth(T):
    """Additions a probability passes through at most: the five levels of the tile's 32-lane tree, then one per further tile."""
    return 5 + (T + TILE - 1) // TILE - 1


def ordered_sum(prob, n):
    """fp32 sum of prob[:n] (one pair's frames, fp32 [T]) in the library's order: per 32-frame tile a stride-halving tree over the
    lanes (lane l takes l + 16, then l + 8, ..., l + 1; a frame >= n is a literal 0), then the tiles ascending."""
    prob = np.asarray(prob, np.float32)
    T = prob.shape[0]
    nt = (T + TILE - 1) // TILE
    v = np.zeros(nt * TILE, np.float32)
    v[:n] = prob[:n]
    v = v.reshape(nt, TILE)
    for half in (16, 8, 4, 2, 1):
        v = v[:, :half] + v[:, half:2 * half]
    total = v[0, 0]
    for k in range(1, nt):
        total = np.float32(total + v[k, 0])
    return np.float32(total)


def numbers_from_frames(prob, len_music=None, len_motion=None):
    """(sum fp32, above, below, count) [Bm, Bn] from per-frame probabilities [Bm, Bn, T]: ordered_sum and the two strict comparisons
    of M2SNet_eval.py:65-66 over the frames t < min(len_music[i], len_motion[j])."""
    prob = np.asarray(prob, np.float32)
    Bm, Bn, T = prob.shape
    lm = np.full(Bm, T) if len_music is None else np.asarray(len_music)
    ln = np.full(Bn, T) if len_motion is None else np.asarray(len_motion)
    count = np.minimum(lm[:, None], ln[None, :]).astype(np.int32)
    total = np.zeros((Bm, Bn), np.float32)
    above, below = np.zeros((Bm, Bn), np.int32), np.zeros((Bm, Bn), np.int32)
    for i in range(Bm):
        for j in range(Bn):
            n = int(count[i, j])
            total[i, j] = ordered_sum(prob[i, j], n)
            above[i, j], below[i, j] = int((prob[i, j, :n] > 0.5).sum()), int((prob[i, j, :n] < 0.5).sum())
    return total, above, below, count


def fuse_every_pair(net, mus, mot):
    """prob [Bm, Bn, T] (numpy fp32) from `net.fuse` alone: motion j against every music, one call per motion."""
    Bm = mus.shape[0]
    return np.stack([net.fuse(mus, mot[j:j + 1].expand(Bm, -1, -1).contiguous()).cpu().numpy() for j in range(mot.shape[0])], axis=1)


def latents(net, B, T):
    """(music latent [B, T, 64], motion latent [B, 64, T]) on the device: M2SNet's encoders on B fixture clips (fixture_inputs at
    max(T, 2) frames - the music encoder needs four mel frames), the first T frames."""
    mel, motion = fixture_inputs(max(T, 2), B=B)
    return net.music_latent(mel)[:, :T].contiguous(), net.motion_latent(motion)[:, :, :T].contiguous()


def retrieval_keys(mean_real, mean_gen, counts_real, counts_gen, top_k=(1, 2, 3)):
    """evaluate_dataset's retrieval keys from the two [N, N] mean matrices and their (above, below, count) triples."""
    out = {}
    for name, mean, cnt in (("real", mean_real, counts_real), ("gen", mean_gen, counts_gen)):
        st = metrics.retrieval_stats(mean, top_k)
        out[f"m2s_r_precision_{name}"] = [float(v) for v in st["r_precision"]]
        out[f"m2s_mean_rank_{name}"] = st["mean_rank"]
        out[f"m2s_margin_{name}"] = st["margin"]
        out[f"m2s_pair_accuracy_{name}"] = metrics.pair_accuracy(*cnt)
    out["m2s_sync_offdiag_gen"] = metrics.retrieval_stats(mean_gen, top_k)["offdiag_mean"]
    return out


class MusicOnlySampler:
    """Stands in for a DDPMTrainer in evaluate_dataset: a clip's poses are an element-wise function of that clip's mel (every third
    mel frame, the first `dim_pose` bins), so they depend neither on the batch around the clip nor on its position or noise."""
    encoder = None

    def __init__(self, device):
        self.device = torch.device(device)

    def generate_music_motion(self, mel, dim_pose, noise=None, smooth=None, **kw):
        mel = torch.as_tensor(np.asarray(mel) if not torch.is_tensor(mel) else mel).to(self.device, torch.float32)
        return (0.5 + 0.2 * torch.tanh(0.25 * mel[:, ::3, :dim_pose])).contiguous()
