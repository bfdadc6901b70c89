"""Seeded inputs, an fp64 oracle and a float32 restatement for the beat scores of csrc/dc_rhythm.hip (dc_rhythm_motion_beats,
dc_rhythm_beat_scores), and the inputs of tests/golden/g18_beats.npz (tools/make_golden_beats.py).  numpy only: the GPU tests need
neither scipy nor the reference.  Written apart from metrics.motion_beats_host / beat_alignment_host (loops where those are
vectorised), so that the two check each other."""
import numpy as np

from diffusion_conductor_amd.synthetic import synthetic_generated_motion, synthetic_motion

FIXTURE = "g18_beats.npz"
REAL_SEED, GEN_SEED, OFFSET = 41, 43, 0.5
ORDER, SIGMA = 10, 3
# no frame (1), the longest clip without a possible beat (11: frames <= order and the last one are never beats), the first lengths
# where frame 11 could be one (12: it is the last; 13), 21 / 22 (the first length with a full +-10 window inside the clip), one tile
# of the kernel's 256 threads less one / exact / plus one, a short clip, a full one
FIXTURE_T = (1, 11, 12, 13, 21, 22, 255, 256, 257, 300, 1800)
SCORED_T = (300, 1800)                # the lengths whose reference scores the fixture stores
CLIPS = 3
MUSIC_EVERY, MUSIC_FIRST = 37, 5      # the fixture's music beats: one every 37 mel frames from frame 5, Lm = 3 T
EPS = 2.0 ** -24                      # float32's unit roundoff


def fixture_pair(T, n=CLIPS):
    """(real, generated) fp32 [n, T, 13, 2]: synthetic_motion around OFFSET and its perturbed companion."""
    real = (synthetic_motion(n, T, seed=REAL_SEED, first=100 * T) + np.float32(OFFSET)).astype(np.float32)
    return real, synthetic_generated_motion(real, seed=GEN_SEED + T)


def fixture_music(T):
    """uint8 [3 T]: the fixture's music beats for a clip of T frames."""
    m = np.zeros(3 * T, np.uint8)
    m[MUSIC_FIRST::MUSIC_EVERY] = 1
    return m


def envelope_f32(x):
    """[T, 13, 2] float32 -> the summed joint speed [T] in float32: every operation rounded on its own, the 13 norms added as
    ((n0+n1)+(n2+n3)) + ((n4+n5)+(n6+n7)), then + n8 .. + n12 one after the other."""
    x = np.asarray(x, np.float32).reshape(-1, 13, 2)
    e = np.zeros(x.shape[0], np.float32)
    for t in range(1, x.shape[0]):
        n = []
        for j in range(13):
            dx, dy = np.float32(x[t, j, 0] - x[t - 1, j, 0]), np.float32(x[t, j, 1] - x[t - 1, j, 1])
            n.append(np.sqrt(np.float32(np.float32(dx * dx) + np.float32(dy * dy))))
        s = np.float32(np.float32(np.float32(n[0] + n[1]) + np.float32(n[2] + n[3])) + np.float32(np.float32(n[4] + n[5]) + np.float32(n[6] + n[7])))
        for j in range(8, 13):
            s = np.float32(s + n[j])
        e[t] = s
    return e


def minima(e, order=ORDER):
    """bool [L]: e[t] < e[clip(t - s)] and e[t] < e[clip(t + s)] for every s = 1 .. order, clip to [0, L - 1]."""
    L = len(e)
    out = np.zeros(L, bool)
    for t in range(L):
        out[t] = all(e[t] < e[max(t - s, 0)] and e[t] < e[min(t + s, L - 1)] for s in range(1, order + 1))
    return out


def beats_f32(x, length=None, order=ORDER):
    """[B, T, 13, 2] -> (beats bool [B, T], envelope float32 [B, T]); frames behind a clip's length are 0 and are not looked at."""
    x = np.asarray(x, np.float32)
    x = x.reshape(x.shape[0], x.shape[1], 13, 2)
    B, T = x.shape[:2]
    beats, env = np.zeros((B, T), bool), np.zeros((B, T), np.float32)
    for b in range(B):
        L = T if length is None else int(length[b])
        env[b, :L] = envelope_f32(x[b, :L])
        beats[b, :L] = minima(env[b, :L], order)
    return beats, env


def scores_f64(music, motion, music_stride=1, sigma=SIGMA):
    """One clip's (BC, Beat Align, music beats, motion beats) in float64 with music beat i at exactly i / music_stride motion
    frames.  BC: 0 without motion beats, else the mean over the music beats (nan without one); Beat Align: 0 without music beats,
    else the mean over the motion beats (nan without one)."""
    i = np.flatnonzero(np.asarray(music)).astype(np.float64) / float(music_stride)
    m = np.flatnonzero(np.asarray(motion)).astype(np.float64)
    if not i.size or not m.size:
        return (float("nan") if m.size else 0.0), (float("nan") if i.size else 0.0), int(i.size), int(m.size)
    d = np.abs(i[:, None] - m[None, :])                             # every music beat against every motion beat
    g = lambda d: np.exp(-d * d / (2.0 * float(sigma) ** 2))      # noqa: E731
    return float(g(d.min(axis=1)).mean()), float(g(d.min(axis=0)).mean()), int(i.size), int(m.size)


def score_bound(n):
    """|device - fp64| of a score that is a mean of n terms in [0, 1], each an fp32 expf, summed in fp32 in some fixed order:
    (n + 4) 2^-24 absolute."""
    return (n + 4) * EPS


def exact_case():
    """(motion fp32 [1, 100, 13, 2], envelope fp32 [100], beats bool [100]) where every float32 operation is exact, so that nothing
    depends on a summation order: y is constant, x moves on a 2^-10 grid.  The envelope is 1000 grid steps everywhere but
      frames 20, 21 = 100   a two-frame plateau minimum: no beat;
      frame 40 = 200 and frame 51 = 150   a strict minimum exactly 11 frames from a lower value: both are beats;
      frame 70 = 200 and frame 80 = 150   a strict minimum exactly 10 frames from a lower value: 70 is no beat, 80 is one."""
    T, grid = 100, 2.0 ** -10
    steps = np.full(T, 1000, np.int64)
    steps[0] = 0
    steps[[20, 21]] = 100
    steps[[40, 70]] = 200
    steps[[51, 80]] = 150
    x = np.zeros((T, 13, 2), np.float64)
    x[:, :, 1] = 0.25
    for t in range(1, T):
        k = steps[t] // 13 + (np.arange(13) < steps[t] % 13)           # the frame's steps dealt over the 13 joints
        x[t, :, 0] = x[t - 1, :, 0] + (1 if t % 2 else -1) * k * grid
    beats = np.zeros(T, bool)
    beats[[40, 51, 80]] = True
    motion = x.astype(np.float32)[None]
    assert np.array_equal(motion.astype(np.float64)[0], x)
    return motion, (steps * grid).astype(np.float32), beats
