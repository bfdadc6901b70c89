"""The rhythm and critic kernels (csrc/dc_rhythm.hip) against the fp64 oracle of tests/helpers_rhythm.py where test_gpu_rhythm.py does
not look: pooled lengths on every wave and workgroup edge of the three critic stages and of the head, Welch column counts on the
edges of k_psd_cols' waves, contour windows on the edges of k_contour's 7-window workgroups, pixel-scale motion, a workspace that
grows, shrinks and runs on another stream, and non-finite inputs.

Bounds.  Those of test_gpu_rhythm.py, imported, in its units: the operations are the same, only the lengths differ, and no kernel
here has a recurrence.  The non-finite checks have no tolerance: the GPU's NaN mask (for infinities: the class NaN / +inf / -inf /
finite of every element) is the oracle's, which test_host_rhythm.py ties to torch's own conv1d, max_pool1d and avg_pool1d; every
finite element of the poisoned clip and every element of the other clips is bit-identical to the clean run.  torch's max_pool1d keeps
a NaN; a pool written with fmaxf returns the finite operand, and one NaN pose value then survives the first stage only where a
stride-3 window starts exactly two frames before it.
"""
import numpy as np
import pytest
import torch

import helpers_rhythm as H
from test_gpu_rhythm import CONTOUR_TOL, FEAT_TOL, PSD01_TOL, PSD_TOL, SCORE_TOL, SD_TOL

from diffusion_conductor_amd import metrics
from diffusion_conductor_amd.discriminator import Discriminator_1DCNN
from diffusion_conductor_amd.rhythm import MotionRhythm
from diffusion_conductor_amd.synthetic import synthetic_discriminator_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 3)


@pytest.fixture(scope="module")
def weights():
    return synthetic_discriminator_state_dict(0)


@pytest.fixture(scope="module")
def rhythm():
    return MotionRhythm(DEV)


@pytest.fixture(scope="module")
def critic(weights):
    return Discriminator_1DCNN(DEV).load_state_dict(weights, strict=True)


@pytest.fixture(scope="module")
def motions():
    """T -> real fp32 [3, T, 13, 2], the seeded clips of the fixture and a third."""
    cache = {}

    def get(T):
        if T not in cache:
            cache[T] = H.fixture_pair(T, n=3)[0]
        return cache[T]
    return get


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


def _critic_errors(critic, weights, x, B, what):
    """The checks of test_gpu_rhythm.py's critic test on x[:B]: -> (features, first frame, last frame, score) errors."""
    f_ref = H.critic_features(weights, x)
    s_ref = H.critic_score(weights, features=f_ref)
    scale = np.abs(f_ref).max()
    f = critic.features(x[:B])
    assert isinstance(f, list) and len(f) == 1 and tuple(f[0].shape) == (B, 64, H.pooled_frames(x.shape[1])[2])
    d = critic(x[:B])
    assert tuple(d.shape) == (B, 1) and d.dtype == torch.float32
    err = np.abs(_np(f[0]) - f_ref[:B]) / scale
    es = float(np.abs(_np(d)[:, 0] - s_ref[:B]).max() / max(np.abs(s_ref).max(), 1.0))
    e = (float(err.max()), float(err[..., 0].max()), float(err[..., -1].max()), es)
    print(f"critic {what} B={B}: features {e[0]:.2e} first frame {e[1]:.2e} last {e[2]:.2e} (max |f| {scale:.2f})  score {e[3]:.2e}")
    assert max(e[:3]) <= FEAT_TOL and e[3] <= SCORE_TOL, (what, B, e)
    return e


# (stage, frames a wave covers, the pooled lengths on its wave and workgroup edges, the clip lengths that give them); 0: the head
CRITIC_EDGES = {
    "stage 1": (1, (20, 21, 40, 41), (62, 65, 122, 125)),
    "stage 2": (2, (14, 15, 28, 29, 56, 57), (95, 101, 179, 185, 347, 353)),
    "stage 3": (3, (14, 15, 56, 57), (197, 209, 701, 713)),
    "head": (3, (32, 33), (413, 425)),
}


@pytest.mark.parametrize("edge", list(CRITIC_EDGES), ids=[k.replace(" ", "_") for k in CRITIC_EDGES])
def test_critic_pooled_lengths_on_every_tile_edge(critic, weights, motions, edge):
    """A wave of k_disc_conv writes 10 pooled frames in stage 1 and 14 in stages 2 and 3, four waves a workgroup; a wave of
    k_disc_head takes 32 frames.  Each edge length L and L + 1, and behind the first of a pair the two lengths T + 1, T + 2 whose
    extra frames the pools drop."""
    stage, pooled, lengths = CRITIC_EDGES[edge]
    errs = []
    for k, (L, T) in enumerate(zip(pooled, lengths)):
        assert H.pooled_frames(T)[stage - 1] == L, (edge, T, H.pooled_frames(T))
        for Tx in (T, T + 1, T + 2) if k % 2 == 0 else (T,):
            assert H.pooled_frames(Tx)[stage - 1] == L, (edge, Tx, H.pooled_frames(Tx))
            for B in BATCHES:
                errs.append(_critic_errors(critic, weights, motions(Tx), B, f"{edge} L{stage}={L} T={Tx}"))
    print(f"== critic {edge}: worst features {max(e[0] for e in errs):.2e}, first frame {max(e[1] for e in errs):.2e}, last frame "
          f"{max(e[2] for e in errs):.2e}, score {max(e[3] for e in errs):.2e}")


def _psd_errors(rhythm, x, B, what):
    ref = H.welch_psd(x)
    psd = rhythm.psd(x[:B])
    assert tuple(psd.shape) == (B, 32) and psd.dtype == torch.float32
    e = H.psd_error(_np(psd), ref[:B])
    e01 = float((np.abs(_np(psd) - ref[:B])[:, :2] / ref[:B, :2]).max())
    print(f"PSD {what} B={B}: error {e:.2e} (bins 0, 1 relative to themselves {e01:.2e})")
    assert e <= PSD_TOL and e01 <= PSD01_TOL, (what, B, e, e01)
    return e, e01


def test_psd_columns_on_every_wave_edge(rhythm, motions):
    """A wave of k_psd_cols takes 32 of a clip's segments x 26 columns, four waves a workgroup: 4 segments = 104 columns = 4 waves
    (one workgroup), 5 = 130 = 5 waves (a second workgroup), 16 = 416 = 13 full waves with no idle column, and 15 segments behind
    which 127 frames - the longest tail - are dropped."""
    errs = []
    for T, nseg, waves in ((640, 4, 4), (768, 5, 5), (2176, 16, 13), (2175, 15, 13)):
        assert (T - H.HOP) // H.HOP == nseg and -(-nseg * 26 // 32) == waves and (T != 2176 or nseg * 26 == 32 * waves)
        for B in BATCHES:
            errs.append(_psd_errors(rhythm, motions(T), B, f"T={T}"))
    print(f"== PSD wave edges: worst {max(e[0] for e in errs):.2e}, bins 0 and 1 {max(e[1] for e in errs):.2e}")


def _contour_errors(rhythm, x, B, what):
    T = x.shape[1]
    c_ref, s_ref = H.contour(x), H.sd(x)
    c, s = rhythm.contour_and_std(x[:B])
    assert tuple(c.shape) == (B, (T - 60) // 30 + 1) and tuple(s.shape) == (B,)
    ec = max(float(np.abs(_np(c)[b] - c_ref[b]).max() / np.abs(c_ref[b]).max()) for b in range(B))
    es = float((np.abs(_np(s) - s_ref[:B]) / s_ref[:B]).max())
    print(f"contour {what} B={B}: error {ec:.2e}   SD: {es:.2e}")
    assert ec <= CONTOUR_TOL and es <= SD_TOL, (what, B, ec, es)
    return ec, es


def test_contour_windows_on_every_workgroup_edge(rhythm, motions):
    """A workgroup of k_contour takes 7 windows: W = 7 (one full workgroup), 7 and 29 dropped frames, 8 (one window in a second
    workgroup), 14 and 15."""
    errs = []
    for T, W in ((240, 7), (269, 7), (270, 8), (450, 14), (480, 15)):
        assert (T - 60) // 30 + 1 == W
        for B in BATCHES:
            errs.append(_contour_errors(rhythm, motions(T), B, f"T={T} W={W}"))
    print(f"== contour workgroup edges: worst {max(e[0] for e in errs):.2e}, SD {max(e[1] for e in errs):.2e}")


def test_pixel_coordinates(rhythm, critic, weights, motions):
    """The same clips as x 1000 + 500: every unit is relative, so the bounds are the same.  The offset is 500 times the motion's own
    size in front of the Welch detrend and of k_sd's pivot."""
    px = lambda T: (motions(T) * np.float32(1000) + np.float32(500)).astype(np.float32)      # noqa: E731
    errs = []
    for B in BATCHES:
        errs.append(_psd_errors(rhythm, px(768), B, "x 1000 + 500 T=768") + _contour_errors(rhythm, px(450), B, "x 1000 + 500 T=450")
                    + _critic_errors(critic, weights, px(353), B, "x 1000 + 500 T=353"))
    print("== x 1000 + 500: worst PSD {:.2e} bins 0 and 1 {:.2e} contour {:.2e} SD {:.2e} features {:.2e} first {:.2e} last {:.2e} "
          "score {:.2e}".format(*(max(e[i] for e in errs) for i in range(8))))


def test_workspace_shrinks_and_grows_on_two_streams(weights, motions):
    """One MotionRhythm and one critic through a long clip, the shortest one and the long one again, on the current stream and on a
    second one: every result is bit-identical to a fresh handle's (the workspace is reallocated only when it grows; a stale plane,
    partial or length would show here)."""
    rh, cr = MotionRhythm(DEV), Discriminator_1DCNN(DEV).load_state_dict(weights, strict=True)
    calls = (("psd", lambda r, c, x: r.psd(x), (2176, H.MIN_PSD_T, 2176)),
             ("contour", lambda r, c, x: r.contour_and_std(x)[0], (2176, H.MIN_CONTOUR_T, 2176)),
             ("sd", lambda r, c, x: r.contour_and_std(x)[1], (2176, H.MIN_CONTOUR_T, 2176)),
             ("features", lambda r, c, x: c.features(x)[0], (713, H.MIN_CRITIC_T, 713)),
             ("score", lambda r, c, x: c.forward(x), (713, H.MIN_CRITIC_T, 713)))
    fresh = {}
    for name, f, lengths in calls:
        for T in set(lengths):
            x = torch.from_numpy(motions(T)).to(DEV)
            fresh[name, T] = f(MotionRhythm(DEV), Discriminator_1DCNN(DEV).load_state_dict(weights, strict=True), x).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for stream in (torch.cuda.current_stream(), side):
        for name, f, lengths in calls:
            for T in lengths:
                x = torch.from_numpy(motions(T)).to(DEV)
                stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(stream):
                    got = f(rh, cr, x)
                stream.synchronize()
                assert torch.equal(got, fresh[name, T]), (name, T, stream is side)


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------------
def _same_bits(got, clean, what):
    assert np.array_equal(_bits(got), _bits(clean)), what


def _nan_check(what, got, clean, ref):
    """got, clean: the GPU's [3, ...] of the poisoned and of the clean clips; ref: the oracle's of the poisoned clips.  -> the number
    of NaN elements of clip 1."""
    g, c, ref = got.cpu().numpy(), clean.cpu().numpy(), np.asarray(ref)
    assert g.shape == c.shape == ref.shape, (what, g.shape, ref.shape)
    mask, want = np.isnan(g[1]), np.isnan(ref[1])
    print(f"{what}: NaN elements of clip 1: GPU {int(mask.sum())} oracle {int(want.sum())} of {want.size}")
    assert np.isfinite(ref[[0, 2]]).all() and np.isfinite(ref[1][~want]).all(), what
    assert np.array_equal(mask, want), (what, int(mask.sum()), int(want.sum()))                     # (a)
    _same_bits(g[1][~mask], c[1][~mask], what)                                                      # (b)
    _same_bits(g[[0, 2]], c[[0, 2]], what)                                                          # (c)
    return int(want.sum())


@pytest.mark.parametrize("T,frames", H.CRITIC_NAN_CASES, ids=[f"T{T}_f{'_'.join(map(str, fr))}" for T, fr in H.CRITIC_NAN_CASES])
def test_critic_keeps_a_nan_as_the_reference(critic, weights, motions, T, frames):
    """One NaN at (clip 1, frame t, channel 5) of three clips: the features that are NaN are exactly the oracle's, the score of clip 1
    is NaN, and nothing else changes by a bit.  Frames t - 2 .. t + 2 of the first convolution are NaN; in two of the three alignments
    of t against the stride-3 pool every window that holds them holds a finite frame too."""
    real = motions(T)
    clean_f, clean_d = critic.features(real)[0].clone(), critic(real).clone()
    assert bool(torch.isfinite(clean_f).all()) and bool(torch.isfinite(clean_d).all())
    for t in frames:
        bad = H.poisoned(real, t)
        f_ref = H.critic_features(weights, bad)
        n = _nan_check(f"critic features T={T} NaN at frame {t}", critic.features(bad)[0], clean_f, f_ref)
        assert n > 0 and n % 64 == 0, (T, t, n)                  # whole pooled frames: the convolution mixes every channel
        _nan_check(f"critic score T={T} NaN at frame {t}", critic(bad), clean_d, H.critic_score(weights, features=f_ref)[:, None])
        assert bool(torch.isnan(critic(bad)[1]).all())


@pytest.mark.parametrize("value", (np.inf, -np.inf), ids=("+inf", "-inf"))
def test_critic_infinities_as_the_reference(critic, weights, motions, value):
    """One infinity in place of the NaN at T = 125: an infinite conv output is +inf or 0 behind the ReLU, and NaN one stage on where
    weights of both signs meet it.  Every element's class is the oracle's; the other clips are the clean run's."""
    T = 125
    real = motions(T)
    clean_f, clean_d = critic.features(real)[0].clone(), critic(real).clone()
    for t in (62, 63, 64):
        bad = H.poisoned(real, t, value)
        f_ref = H.critic_features(weights, bad)
        f, d = critic.features(bad)[0], critic(bad)
        cf, cd = H.value_class(_np(f)), H.value_class(_np(d)[:, 0])
        wf, wd = H.value_class(f_ref), H.value_class(H.critic_score(weights, features=f_ref))
        print(f"critic T={T} {value} at frame {t}: features of clip 1 NaN {int((wf[1] == 3).sum())} +inf {int((wf[1] == 1).sum())} "
              f"finite {int((wf[1] == 0).sum())} (GPU {int((cf[1] == 3).sum())} / {int((cf[1] == 1).sum())} / {int((cf[1] == 0).sum())}); "
              f"score class {wd[1]} (GPU {cd[1]})")
        assert wf[1].any() and not (wf == 2).any()
        assert np.array_equal(cf, wf) and np.array_equal(cd, wd), (value, t)
        _same_bits(f[[0, 2]], clean_f[[0, 2]], (value, t))
        _same_bits(d[[0, 2]], clean_d[[0, 2]], (value, t))


def test_psd_contour_and_sd_keep_a_nan_as_the_reference(rhythm, motions):
    """PSD at T = 383 (one segment and a dropped tail): a NaN inside the segment is in its column's mean, so in all 32 bins of the
    clip; one in the tail is never read.  Contour at T = 270: speed frames t and t + 1 are NaN, and so is every window that holds
    one of them; SD is NaN for the clip whatever the frame."""
    T = 383
    real = motions(T)
    clean = rhythm.psd(real).clone()
    bad = H.poisoned(real, 100)
    assert _nan_check(f"PSD T={T} NaN at frame 100", rhythm.psd(bad), clean, H.welch_psd(bad)) == 32
    bad = H.poisoned(real, 300)
    assert _nan_check(f"PSD T={T} NaN at frame 300 (the dropped tail)", rhythm.psd(bad), clean, H.welch_psd(bad)) == 0
    T = 270
    real = motions(T)
    clean_c, clean_s = (a.clone() for a in rhythm.contour_and_std(real))
    for t, windows in ((95, (2, 3)), (0, (0,)), (T - 1, (7,))):
        bad = H.poisoned(real, t)
        c, s = rhythm.contour_and_std(bad)
        c_ref = H.contour(bad)
        assert list(np.nonzero(np.isnan(c_ref[1]))[0]) == list(windows), (t, windows)
        assert _nan_check(f"contour T={T} NaN at frame {t}", c, clean_c, c_ref) == len(windows)
        assert _nan_check(f"SD T={T} NaN at frame {t}", s, clean_s, H.sd(bad)) == 1


def test_w_distance_is_nan_with_one_nan_in_the_real_motion(critic, weights):
    T = 900
    real, gen = H.fixture_pair(T, n=3)
    assert np.isfinite(metrics.w_distance(critic(real), critic(gen)))
    bad = H.poisoned(real, 450)
    wd = metrics.w_distance(critic(bad), critic(gen))
    wd64 = float((H.critic_score(weights, bad) - H.critic_score(weights, gen)).mean())
    print(f"W-distance with one NaN in the real motion: {wd} (oracle {wd64})")
    assert np.isnan(wd64) and np.isnan(wd)


def test_a_nan_in_the_ground_truth_reaches_every_score_of_the_evaluator(rhythm, critic, tmp_path):
    """The setup of test_gpu_rhythm.py's test_through_the_evaluator with three clips.  evaluate_dataset checks the poses it generates,
    not the motion.npy it reads: one NaN in clip 001's ground truth (frame 100: inside Welch's one segment, in contour windows 2 and
    3, and in no first-stage pool window alone) makes w_distance, rde, sce and sd_real NaN, as the reference's evaluation would
    report, and leaves the other clips' entries as they were."""
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.generator import Generator, GeneratorBaseline
    from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_m2sgan_state_dict, synthetic_motion
    T, n, seed = 270, 3, 6
    gts = synthetic_motion(n, T, seed=24) + np.float32(0.5)
    base = GeneratorBaseline(Generator(DEV).load_state_dict(synthetic_m2sgan_state_dict(0), strict=True))
    runs = []
    for name, motion in (("clean", gts), ("poisoned", H.poisoned(gts, 100))):
        root = tmp_path / name
        for i in range(n):
            d = root / f"{i:03d}"
            d.mkdir(parents=True)
            np.save(d / "mel.npy", smooth_mel(700 + i, 3 * T - 2, seed=7))
            np.save(d / "motion.npy", motion[i])
        runs.append(ev.evaluate_dataset(base, str(root), 26, batch_size=2, seed=seed, verbose=False, rhythm=rhythm, discriminator=critic))
    clean, bad = runs
    ids = sorted(clean["per_clip"])
    assert len(ids) == n
    print("evaluate_dataset with one NaN in a ground truth: " + "  ".join(f"{k} {clean[k]:.6g} -> {bad[k]}" for k in ("w_distance", "rde", "sce", "sd_real")))
    for k in ("w_distance", "rde", "sce", "sd_real"):
        assert np.isfinite(clean[k]) and np.isnan(bad[k]), (k, clean[k], bad[k])
    assert bad["sd_gen"] == clean["sd_gen"]
    for k in ("rde_per_clip", "sce_per_clip"):
        assert np.isnan(bad[k][ids[1]]) and np.isfinite(clean[k][ids[1]]), k
        assert all(bad[k][c] == clean[k][c] for c in (ids[0], ids[2])), k
