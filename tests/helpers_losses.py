"""Shared by tests/test_host_losses.py and tests/test_gpu_losses.py: the inputs of tests/golden/g14_training_losses.npz regenerated
from their seeds (tools/make_golden_losses.py, case_inputs - pinned by the fixture's digests), and the fp64 definitions of the
per-clip loss terms (include/dc_ddim.h, dc_motion_loss_terms / dc_latent_l1)."""
import numpy as np

from helpers import golden

from diffusion_conductor_amd.synthetic import array_digest, batch_mel, batch_noise, synthetic_motion

S = 1000
CASES_A = ((1, 2), (3, 5), (3, 33), (2, 65))
CASES_B = ((3, 64), (2, 1800))
MEAN_TYPES = ("START_X", "EPSILON")
SCALAR_KEYS = ("loss_mot_rec", "loss_mot_feat", "loss_velocity", "loss_velocity_elbow", "loss_velocity_head", "loss")
BODY, ELBOW, HEAD = [10, 11, 12, 13, 22, 23, 24, 25], list(range(14, 22)), list(range(10))
_cache = {}


def g14():
    if "g14" not in _cache:
        _cache["g14"] = dict(golden("g14_training_losses.npz"))
    return _cache["g14"]


def case_inputs(B, T, mel=False):
    """x0 [B, T, 13, 2], noise [B, T, 13, 2], the stub model's unit-scale output [B, T, 26] (and the mel [B, 3 T, 128])."""
    g = g14()
    first = 100 * T + B
    seeds = [int(v) for v in g["seeds"]]
    x0 = synthetic_motion(B, T, seed=seeds[0], first=first)
    noise = batch_noise(B, T, 26, seed=seeds[1], first=first).reshape(B, T, 13, 2)
    stub = batch_noise(B, T, 26, seed=seeds[2], first=first)
    return (x0, noise, stub, batch_mel(B, 3 * T, 128, seed=seeds[3], first=first)) if mel else (x0, noise, stub)


def check_digests(tag, *arrays):
    want = g14()[f"{tag}_digest"]
    for i, a in enumerate(arrays):
        assert np.allclose(array_digest(a), want[i], rtol=1e-12, atol=1e-9), (tag, i)


def terms_fp64(pred, target, length):
    """[B, 8] float64: the definitions of dc_motion_loss_terms on the fp32 inputs, every operation in float64."""
    p, g = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    B, T = p.shape[:2]
    p, g = p.reshape(B, T, 26), g.reshape(B, T, 26)
    d2 = (g - p) ** 2
    mask = np.arange(T)[None, :] < np.asarray(length).reshape(B, 1)
    vp, vt = p[:, 1:] - p[:, :-1], g[:, 1:] - g[:, :-1]
    out = np.zeros((B, 8))
    out[:, 0] = d2.mean(axis=(1, 2))
    out[:, 1] = (d2.mean(axis=2) * mask).sum(axis=1)
    out[:, 2] = (vp[:, :, BODY] ** 2).mean(axis=(1, 2))
    out[:, 3] = (vp[:, :, ELBOW] ** 2).mean(axis=(1, 2))
    out[:, 4] = (vp[:, :, HEAD] ** 2).mean(axis=(1, 2))
    out[:, 5] = ((vt - vp) ** 2).mean(axis=(1, 2))
    return out


def latent_l1_fp64(a, b):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).mean(axis=(1, 2))


def rel(a, b):
    """Largest relative difference of two arrays of positive numbers (b the reference)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.abs(b)))
