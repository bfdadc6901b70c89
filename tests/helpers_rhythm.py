"""numpy-fp64 restatements of what csrc/dc_rhythm.hip computes - the Welch PSD behind RDE, the speed contour behind SCE, the standard
deviation, and the M2S-GAN critic - and the seeded inputs of tests/golden/g16_rhythm.npz (tools/make_golden_rhythm.py).  numpy only:
the GPU tests need neither scipy nor the reference."""
import numpy as np

from diffusion_conductor_amd.synthetic import synthetic_generated_motion, synthetic_motion

FIXTURE = "g16_rhythm.npz"
REAL_SEED, GEN_SEED, OFFSET = 31, 37, 0.5
# every length a test scores: the critic's shortest (L3 = 1, 1, 2), the contour's one / one + tail / two windows, Welch's one
# segment / one + tail / two segments, a half clip and a full one
FIXTURE_T = (41, 44, 53, 60, 89, 90, 256, 383, 384, 900, 1800)
MIN_CRITIC_T, MIN_CONTOUR_T, MIN_PSD_T = 41, 60, 256
NSEG, HOP, BINS, FS = 256, 128, 32, 30.0
BAND = (6, 26)


def fixture_pair(T, n=2):
    """(real, generated) fp32 [n, T, 13, 2]: synthetic_motion around OFFSET (pose-like values in [0, 1]-ish units; the offset is what
    the detrend has to remove) and its perturbed companion."""
    real = (synthetic_motion(n, T, seed=REAL_SEED, first=100 * T) + np.float32(OFFSET)).astype(np.float32)
    return real, synthetic_generated_motion(real, seed=GEN_SEED + T)


# (T, frames) of the critic's non-finite cases: one value of clip 1 overwritten at channel POISON_CHANNEL of one frame.  Around the
# middle of a clip in each alignment of the stride-3 pool (a window of 5 holds nothing but NaN frames only when it starts at t - 2),
# at both ends (Conv1d's zero padding) and at T = 44 on frame 43, the last frame of the last pool window.
CRITIC_NAN_CASES = ((41, (20, 21, 22)), (125, (62, 63, 64)), (209, (104, 105, 106)), (900, (450, 451, 452)), (900, (0, 899)), (44, (43,)))
POISON_CLIP, POISON_CHANNEL = 1, 5


def poisoned(x, frame, value=np.nan, clip=POISON_CLIP):
    """A copy of the motions x [B, T, 13, 2] with `value` at (clip, frame, channel POISON_CHANNEL)."""
    bad = np.array(x, np.float32).reshape(x.shape[0], x.shape[1], 26)
    bad[clip, frame, POISON_CHANNEL] = value
    return bad.reshape(x.shape)


def value_class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, element by element."""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0))).astype(np.int8)


def _clips(x):
    x = np.asarray(x, np.float64)
    return x.reshape(x.shape[0], x.shape[1], 26)


def welch_psd(x):
    """scipy.signal.welch(x, fs=30) with its defaults, summed over the 26 channels and / 26: [B, T, 26] -> bins 0 .. 31, [B, 32]."""
    x = _clips(x)
    B, T, _ = x.shape
    assert T >= NSEG
    n = np.arange(NSEG)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / NSEG)                        # periodic Hann
    scale = 1.0 / (FS * (w * w).sum())
    nseg = (T - HOP) // HOP
    out = np.zeros((B, NSEG // 2 + 1))
    for s in range(nseg):
        seg = x[:, s * HOP:s * HOP + NSEG]                              # [B, 256, 26]
        seg = (seg - seg.mean(axis=1, keepdims=True)) * w[None, :, None]
        p = np.abs(np.fft.rfft(seg, axis=1)) ** 2 * scale
        p[:, 1:-1] *= 2                                                 # one-sided: every bin but 0 and Nyquist
        out += p.sum(axis=2)
    return (out / nseg / 26.0)[:, :BINS]


def psd_error(psd, ref):
    """The PSD tests' error: max |delta| over bins 0 .. 31 over the clip's largest in-band value of `ref`; the worst clip."""
    psd, ref = np.asarray(psd, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(psd - ref).max(axis=1) / ref[:, BAND[0]:BAND[1]].max(axis=1)).max())


def rde(psd_real, psd_gen):
    """per clip log(mean((r[6:26] - g[6:26])^2) 1e7 + 1), fp64."""
    r, g = np.asarray(psd_real, np.float64), np.asarray(psd_gen, np.float64)
    return np.log(((r[:, BAND[0]:BAND[1]] - g[:, BAND[0]:BAND[1]]) ** 2).mean(axis=1) * 1e7 + 1)


def contour(x):
    """loss.py:129-142 per clip: [B, T, 26] -> [B, (T - 60) // 30 + 1]."""
    x = _clips(x)
    B, T, _ = x.shape
    v = np.zeros((B, T))
    v[:, 1:] = np.abs((x[:, :-1] - x[:, 1:]).mean(axis=2))
    W = (T - 60) // 30 + 1
    return np.stack([v[:, 30 * w:30 * w + 60].mean(axis=1) for w in range(W)], axis=1)


def sce(c_real, c_gen):
    r, g = np.asarray(c_real, np.float64), np.asarray(c_gen, np.float64)
    return np.log(((g - r) ** 2).mean(axis=1) * 1e7 + 1)


def sd(x):
    """mean over the channels of the unbiased standard deviation over time: [B, T, 26] -> [B]."""
    return _clips(x).std(axis=1, ddof=1).mean(axis=1)


def pooled_frames(T):
    L1 = (T - 5) // 3 + 1
    L2 = (L1 - 5) // 2 + 1
    return L1, L2, (L2 - 5) // 2 + 1


def critic_features(weights, x):
    """Discriminator_1DCNN.features in fp64: [B, T, 26] -> [B, 64, L3]."""
    h = _clips(x)                                                       # channel-last
    for i, stride in ((0, 3), (3, 2), (6, 2)):
        W, b = np.asarray(weights[f"motion_encoder.{i}.weight"], np.float64), np.asarray(weights[f"motion_encoder.{i}.bias"], np.float64)
        L = h.shape[1]
        hp = np.pad(h, ((0, 0), (2, 2), (0, 0)))
        with np.errstate(invalid="ignore"):                             # (inf - inf of a poisoned input is the NaN the tests look for)
            y = sum(hp[:, tap:tap + L] @ W[:, :, tap].T for tap in range(5)) + b
        y = np.maximum(y, 0.0)
        Lo = (L - 5) // stride + 1
        h = np.stack([y[:, stride * p:stride * p + 5].max(axis=1) for p in range(Lo)], axis=1)
    return h.transpose(0, 2, 1)


def critic_score(weights, x=None, features=None):
    """Discriminator_1DCNN.forward in fp64 -> [B]."""
    f = critic_features(weights, x) if features is None else np.asarray(features, np.float64)
    h = f.transpose(0, 2, 1)
    for i in (0, 2, 4):
        h = h @ np.asarray(weights[f"fc.{i}.weight"], np.float64).T + np.asarray(weights[f"fc.{i}.bias"], np.float64)
        if i != 4:
            h = np.maximum(h, 0.0)
    return h[..., 0].mean(axis=1)
