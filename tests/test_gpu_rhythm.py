"""The rhythm and realism scores on the MI355X (csrc/dc_rhythm.hip; rhythm.py, discriminator.py, metrics.py) against the fp64 oracle
of tests/helpers_rhythm.py and the reference's fp32 values of tests/golden/g16_rhythm.npz (tools/make_golden_rhythm.py).

Bounds.  Each is four times the largest error measured on the MI355X against the fp64 oracle over the cases it covers, rounded up to
one significant digit; against the reference's fp32 fixture it is that bound plus the fixture's
`ref_vs_fp64_*` for the quantity.  Units: the PSD's error is max |delta| over bins 0 .. 31 over the clip's largest in-band (bins
6 .. 25) value; the contour's and the features' are max |delta| over the case's largest |value|, the scores' over max(1, largest
|score|); SD's is relative; RDE, SCE and the W-distance are absolute (RDE and SCE are logarithms, the W-distance a difference of
scores of order 5).
  PSD, T = 256 .. 900 at B = 1 .. 3, 1800 at B = 2   measured 7.20e-6   bound 3e-5
  PSD bins 0 and 1, relative to themselves    measured 9.17e-7   bound 4e-6   (the detrend in front of the window)
  contour, T = 60 .. 1800, B = 1 .. 3 each    measured 3.03e-7   bound 2e-6
  SD                                          measured 1.21e-7   bound 5e-7
  critic features, T = 41 .. 1800, B = 1 .. 3 measured 6.30e-7   bound 3e-6   (first and last pooled frame, 5.0e-7: the same bound)
  critic score                                measured 7.18e-7   bound 3e-6
  RDE, at 2 x 900 and through the evaluator   measured 1.55e-7   bound 7e-7
  SCE                                         measured 4.47e-7   bound 2e-6
  W-distance                                  measured 1.71e-7   bound 7e-7
tests/test_gpu_rhythm_edges.py holds further lengths - pooled lengths, Welch columns and contour windows on the kernels' wave and
workgroup edges, pixel-scale motion - to the same bounds, imported from here.  Measured there: features 7.38e-7, score 3.50e-7,
contour 2.81e-7, SD 1.56e-7, PSD bins 0 and 1 1.48e-6, and the PSD 1.46e-5 (bin 1 at T = 640, 2.9e-7 of itself: the unit's price,
DESIGN.md section 13), which leaves PSD_TOL at twice the largest measurement over all cases instead of four times.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_rhythm as H
from helpers import golden

from diffusion_conductor_amd import metrics
from diffusion_conductor_amd.discriminator import Discriminator_1DCNN
from diffusion_conductor_amd.native import DcError, NativeDiscriminator, NativeRhythm, lib
from diffusion_conductor_amd.rhythm import MotionRhythm
from diffusion_conductor_amd.synthetic import synthetic_discriminator_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PSD_TOL, PSD01_TOL, CONTOUR_TOL, SD_TOL, FEAT_TOL, SCORE_TOL = 3e-5, 4e-6, 2e-6, 5e-7, 3e-6, 3e-6
RDE_TOL, SCE_TOL, WD_TOL = 7e-7, 2e-6, 7e-7


@pytest.fixture(scope="module")
def g16():
    return golden(H.FIXTURE)


@pytest.fixture(scope="module")
def weights():
    return synthetic_discriminator_state_dict(0)            # pinned by the fixture's digests (test_host_rhythm.py)


@pytest.fixture(scope="module")
def rhythm():
    return MotionRhythm(DEV)


@pytest.fixture(scope="module")
def critic(weights):
    return Discriminator_1DCNN(DEV).load_state_dict(weights, strict=True)


@pytest.fixture(scope="module")
def motions():
    """T -> (real, generated) fp32 [3, T, 13, 2]; the first two real clips are the fixture's."""
    cache = {}

    def get(T):
        if T not in cache:
            cache[T] = H.fixture_pair(T, n=3)
        return cache[T]
    return get


BATCHES = (1, 2, 3)


def _np(t):
    return t.cpu().numpy().astype(np.float64)


def _rel(a, ref):
    return float(np.abs(a - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("T", (256, 383, 384, 900, 1800))
def test_psd_against_the_fp64_oracle(rhythm, motions, g16, T):
    """One segment, one segment and a dropped tail, two segments, seven, thirteen (eleven waves per clip)."""
    real = motions(T)[0]
    ref = H.welch_psd(real)
    assert real.mean() > 0.3 and ref[:, 0].min() > 0             # (an offset the detrend removes; bin 0 is the window's leak, not 0)
    for B in ((2,) if T == 1800 else BATCHES):          # (T = 1800 is the one case the batch is fixed for: B = 2)
        psd = rhythm.psd(real[:B])
        assert tuple(psd.shape) == (B, 32) and psd.dtype == torch.float32
        e = H.psd_error(_np(psd), ref[:B])
        e01 = float((np.abs(_np(psd) - ref[:B])[:, :2] / ref[:B, :2]).max())
        print(f"PSD T={T} B={B}: error {e:.2e} (bins 0, 1 relative to themselves {e01:.2e})")
        assert e <= PSD_TOL and e01 <= PSD01_TOL, (T, B, e, e01)
    e_ref = H.psd_error(_np(rhythm.psd(real[:2])), g16[f"psd_real_T{T}"])
    print(f"PSD T={T}: against scipy's fp32 {e_ref:.2e}")
    assert e_ref <= PSD_TOL + float(g16["ref_vs_fp64_psd"])


@pytest.mark.parametrize("T", (60, 89, 90, 1800))
def test_contour_and_sd_against_the_fp64_oracle(rhythm, motions, T):
    """One window, one window and a dropped tail, two windows, 59."""
    real, gen = motions(T)
    for x in (real, gen):
        c_ref, s_ref = H.contour(x), H.sd(x)
        for B in BATCHES:
            c, s = rhythm.contour_and_std(x[:B])
            assert tuple(c.shape) == (B, (T - 60) // 30 + 1) and tuple(s.shape) == (B,)
            ec = max(_rel(_np(c)[b], c_ref[b]) for b in range(B))
            es = float((np.abs(_np(s) - s_ref[:B]) / s_ref[:B]).max())
            print(f"contour T={T} B={B}: error {ec:.2e}   SD: {es:.2e}")
            assert ec <= CONTOUR_TOL and es <= SD_TOL, (T, B, ec, es)
            assert torch.equal(rhythm.contour(x[:B]), c) and torch.equal(rhythm.std(x[:B]), s)      # either output alone


def test_constant_motion_has_no_contour_and_no_deviation(rhythm):
    x = torch.tensor(np.random.default_rng(0).uniform(0.1, 0.9, (2, 1, 26)).astype(np.float32)).expand(2, 95, 26).contiguous()
    c, s = rhythm.contour_and_std(x)
    assert tuple(c.shape) == (2, 2) and bool((c == 0).all()) and bool((s == 0).all())


@pytest.mark.parametrize("T", (41, 44, 53, 900, 1800))
def test_critic_against_the_fp64_oracle(critic, weights, motions, g16, T):
    """L3 = 1 (T = 41, 44: the pools' dropped tails), 2, 72, 147.  The first and the last pooled frame separately: Conv1d's zero
    padding at both ends and the frames a pool drops."""
    real, gen = motions(T)
    for name, x in (("real", real), ("gen", gen)):
        f_ref = H.critic_features(weights, x)
        s_ref = H.critic_score(weights, features=f_ref)
        scale = np.abs(f_ref).max()
        for B in BATCHES:
            f = critic.features(x[:B])
            assert isinstance(f, list) and len(f) == 1 and tuple(f[0].shape) == (B, 64, H.pooled_frames(T)[2])
            f = _np(f[0])
            d = critic(x[:B])
            assert tuple(d.shape) == (B, 1) and d.dtype == torch.float32
            err = np.abs(f - f_ref[:B]) / scale
            es = float(np.abs(_np(d)[:, 0] - s_ref[:B]).max() / max(np.abs(s_ref).max(), 1.0))
            print(f"critic {name} T={T} B={B}: features {err.max():.2e} first frame {err[..., 0].max():.2e} last {err[..., -1].max():.2e} "
                  f"(max |f| {scale:.2f})  score {es:.2e} (scores {s_ref[:B]})")
            assert err[..., 0].max() <= FEAT_TOL and err[..., -1].max() <= FEAT_TOL and err.max() <= FEAT_TOL, (T, B, err.max())
            assert es <= SCORE_TOL, (T, B, es)
    # the fixture's fp32: the reference's own features of the real clips and scores of both
    f = _np(critic.features(real[:2])[0])
    ef = float(np.abs(f - g16[f"features_T{T}"]).max())
    ed = max(float(np.abs(_np(critic(x[:2]))[:, 0] - g16[f"d_{n}_T{T}"]).max()) for n, x in (("real", real), ("gen", H.fixture_pair(T)[1])))
    print(f"critic T={T}: against the reference's fp32 features {ef:.2e} scores {ed:.2e}")
    assert ef <= FEAT_TOL * np.abs(g16[f"features_T{T}"]).max() + float(g16["ref_vs_fp64_features"])
    assert ed <= SCORE_TOL * max(np.abs(g16[f"d_real_T{T}"]).max(), np.abs(g16[f"d_gen_T{T}"]).max(), 1.0) + float(g16["ref_vs_fp64_score"])


def test_scores_end_to_end_at_two_half_clips(rhythm, critic, weights, g16):
    """RDE, SCE and the W-distance of metrics.py on the GPU's arrays at 2 x 900 against the reference's logged values."""
    T = 900
    real, gen = H.fixture_pair(T)
    rde, rde_mean = metrics.rhythm_density_error(rhythm.psd(real), rhythm.psd(gen))
    sce, sce_mean = metrics.strength_contour_error(rhythm.contour(real), rhythm.contour(gen))
    wd = metrics.w_distance(critic(real), critic(gen))
    rde64, sce64 = H.rde(H.welch_psd(real), H.welch_psd(gen)), H.sce(H.contour(real), H.contour(gen))
    wd64 = float((H.critic_score(weights, real) - H.critic_score(weights, gen)).mean())
    e = (float(np.abs(rde - rde64).max()), float(np.abs(sce - sce64).max()), abs(wd - wd64))
    print(f"end to end 2 x {T}: RDE {rde} error {e[0]:.2e}  SCE {sce} error {e[1]:.2e}  W-distance {wd:.6f} error {e[2]:.2e}")
    assert e[0] <= RDE_TOL and e[1] <= SCE_TOL and e[2] <= WD_TOL, e
    assert np.abs(rde - g16[f"rde_T{T}"]).max() <= RDE_TOL + float(g16["ref_vs_fp64_rde"])
    assert np.abs(sce - g16[f"sce_T{T}"]).max() <= SCE_TOL + float(g16["ref_vs_fp64_sce"])
    assert abs(wd - float((g16[f"d_real_T{T}"] - g16[f"d_gen_T{T}"]).astype(np.float64).mean())) <= WD_TOL + 2 * float(g16["ref_vs_fp64_score"])
    assert rde_mean == float(rde.mean()) and abs(sce_mean - float(sce.astype(np.float64).mean())) == 0
    for m in (rhythm.std(real), rhythm.std(gen)):
        assert tuple(m.shape) == (2,)
    assert np.abs(_np(rhythm.std(real)) - g16[f"sd_real_T{T}"]).max() <= SD_TOL * g16[f"sd_real_T{T}"].max() + float(g16["ref_vs_fp64_sd"])
    assert np.abs(_np(rhythm.std(gen)) - g16[f"sd_gen_T{T}"]).max() <= SD_TOL * g16[f"sd_gen_T{T}"].max() + float(g16["ref_vs_fp64_sd"])


def test_bit_identical_in_any_batch_and_on_a_rerun(rhythm, critic, motions):
    for T, calls in ((384, (rhythm.psd, rhythm.contour, rhythm.std, critic.forward, lambda x: critic.features(x)[0])),
                     (53, (critic.forward, lambda x: critic.features(x)[0]))):
        x = torch.from_numpy(motions(T)[0]).to(DEV)
        for f in calls:
            alone, batch = f(x[1:2]).clone(), f(x).clone()
            assert torch.equal(batch[1], alone[0])
            assert torch.equal(f(x.flip(0))[1], alone[0]) and torch.equal(f(x.flip(0))[0], batch[2])
            assert torch.equal(f(x), batch)
    # a batch larger than one pass (64 clips for the rhythm kernels, 32 for the critic) against the same clips one by one
    for T, n, calls in ((256, 66, (rhythm.psd,)), (60, 66, (rhythm.contour, rhythm.std)), (41, 34, (critic.forward, lambda x: critic.features(x)[0]))):
        x = torch.from_numpy(H.fixture_pair(T, n=n)[0]).to(DEV)
        for f in calls:
            big = f(x).clone()
            for b in (0, n // 2 - 1, n // 2, n - 2, n - 1):
                assert torch.equal(big[b], f(x[b:b + 1])[0]), (T, b)


def test_refusals_come_before_any_launch(weights):
    L, stream = lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr()      # noqa: E731
    sentinel = 7.0
    x = torch.zeros(1, 300, 26, device=DEV)
    out = torch.full((1, 64 * 32), sentinel, device=DEV)
    r = NativeRhythm(0)
    assert L.dc_rhythm_psd(r._h, ptr(x), 1, 255, ptr(out), stream) == -1
    assert L.dc_rhythm_contour(r._h, ptr(x), 1, 59, ptr(out), ptr(out), stream) == -1
    assert L.dc_rhythm_psd(r._h, ptr(x), 0, 300, ptr(out), stream) == -1 and L.dc_rhythm_psd(r._h, None, 1, 300, ptr(out), stream) == -1
    assert L.dc_rhythm_psd(r._h, ptr(x), 1, 300, None, stream) == -1 and L.dc_rhythm_contour(r._h, None, 1, 300, ptr(out), None, stream) == -1
    with pytest.raises(ValueError, match="256"):
        r.psd(x[:, :255].contiguous())
    with pytest.raises(ValueError, match="60"):
        r.contour(x[:, :59].contiguous())
    d = NativeDiscriminator(0)
    with pytest.raises(DcError, match="error -4.*unknown"):
        d.set_param("fc.6.weight", np.zeros(32, np.float32))
    with pytest.raises(DcError, match="error -4.*unknown"):
        d.set_param("module.fc.0.weight", np.zeros(32 * 64, np.float32))      # the prefix is the Python loaders' to strip
    with pytest.raises(DcError, match="error -4.*elements"):
        d.set_param("motion_encoder.0.weight", np.zeros(64 * 64 * 5, np.float32))
    # score and features before finalize: DC_ERR_INVALID
    assert L.dc_discriminator_score(d._h, ptr(x), 1, 300, ptr(out), stream) == -1
    assert L.dc_discriminator_features(d._h, ptr(x), 1, 300, ptr(out), stream) == -1
    with pytest.raises(DcError, match="error -1.*finalize"):
        d.score(x)
    last = "fc.4.bias"
    for k, v in weights.items():
        if k != last:
            d.set_param(k, v)
    with pytest.raises(DcError, match="error -4.*fc.4.bias"):
        d.finalize()
    assert L.dc_discriminator_score(d._h, ptr(x), 1, 300, ptr(out), stream) == -1
    d.set_param(last, weights[last])
    d.finalize()
    for B, T in ((1, 40), (0, 300)):
        assert L.dc_discriminator_score(d._h, ptr(x), B, T, ptr(out), stream) == -1
        assert L.dc_discriminator_features(d._h, ptr(x), B, T, ptr(out), stream) == -1
    assert L.dc_discriminator_score(d._h, None, 1, 300, ptr(out), stream) == -1
    with pytest.raises(ValueError, match="41"):
        d.score(x[:, :40].contiguous())
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        Discriminator_1DCNN(DEV).forward(x)
    assert tuple(d.score(x).shape) == (1,) and tuple(r.psd(x).shape) == (1, 32)
    torch.cuda.synchronize()
    d.close()
    r.close()


def test_through_the_evaluator(rhythm, critic, weights, tmp_path):
    """evaluate_dataset(rhythm=, discriminator=) on the M2S-GAN generator as the trainer: the new keys are the oracle's values on the
    poses the run itself made, and everything else is what a run without the two arguments returns."""
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.generator import Generator, GeneratorBaseline
    from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_m2sgan_state_dict, synthetic_motion
    T, n, seed = 270, 2, 6
    gts = synthetic_motion(n, T, seed=24) + np.float32(0.5)
    for i in range(n):
        d = tmp_path / f"{i:03d}"
        d.mkdir()
        np.save(d / "mel.npy", smooth_mel(700 + i, 3 * T - 2, seed=7))
        np.save(d / "motion.npy", gts[i])
    gen = Generator(DEV).load_state_dict(synthetic_m2sgan_state_dict(0), strict=True)
    made = []

    class Recording(GeneratorBaseline):
        def generate_music_motion(self, *a, **kw):
            made.append(super().generate_music_motion(*a, **kw).clone())
            return made[-1]
    base = Recording(gen)
    plain = ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=2, seed=seed, verbose=False)
    del made[:]
    r = ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=2, seed=seed, verbose=False, rhythm=rhythm, discriminator=critic)
    new = {"rde", "sce", "sd_gen", "sd_real", "w_distance", "rde_per_clip", "sce_per_clip"}
    timing = {"seconds", "frames_per_s", "main_thread_s", "steady_frames_per_s"}
    assert set(r) - timing == (set(plain) - timing) | new
    for k in set(plain) - timing:
        assert r[k] == plain[k], k
    one = ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=1, seed=seed, verbose=False, rhythm=rhythm, discriminator=critic)
    for k in new:
        assert one[k] == r[k], k
    poses = made[0].cpu().numpy().reshape(n, T, 26)
    ids = sorted(r["per_clip"])
    rde64, sce64 = H.rde(H.welch_psd(gts), H.welch_psd(poses)), H.sce(H.contour(gts), H.contour(poses))
    wd64 = float((H.critic_score(weights, gts) - H.critic_score(weights, poses)).mean())
    e = {"rde": abs(r["rde"] - rde64.mean()), "sce": abs(r["sce"] - sce64.mean()), "w_distance": abs(r["w_distance"] - wd64),
         "sd_gen": abs(r["sd_gen"] / H.sd(poses).mean() - 1), "sd_real": abs(r["sd_real"] / H.sd(gts).mean() - 1),
         "rde_per_clip": float(np.abs(np.array([r["rde_per_clip"][c] for c in ids]) - rde64).max()),
         "sce_per_clip": float(np.abs(np.array([r["sce_per_clip"][c] for c in ids]) - sce64).max())}
    print(f"evaluate_dataset 2 x {T}: " + "  ".join(f"{k} {r[k] if not isinstance(r[k], dict) else ''} error {v:.2e}" for k, v in e.items()))
    assert max(e["rde"], e["rde_per_clip"]) <= RDE_TOL and max(e["sce"], e["sce_per_clip"]) <= SCE_TOL and e["w_distance"] <= WD_TOL, e
    assert e["sd_gen"] <= SD_TOL and e["sd_real"] <= SD_TOL, e


def test_a_resampled_batch_scores_as_the_clean_run_with_every_family_on(rhythm, critic, tmp_path):
    """evaluate_dataset with the ST-GCN encoder, M2SNet (+ retrieval), MotionRhythm, the critic and beats on the M2S-GAN generator,
    4 clips at T = 270 in batches of 2: batch 0's poses come back with one inf from the unchecked pass, the batch is generated again
    the checked way and scored by the same per-family code - every key but the timings is exactly the clean run's (deterministic
    kernels on the same noise and mel)."""
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.generator import Generator, GeneratorBaseline
    from diffusion_conductor_amd.m2snet import M2SNet
    from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN
    from diffusion_conductor_amd.synthetic import (smooth_mel, synthetic_m2sgan_state_dict, synthetic_m2snet_state_dict, synthetic_motion,
                                                   synthetic_motion_encoder_state_dict)
    T, n, seed = 270, 4, 6
    gts = synthetic_motion(n, T, seed=24) + np.float32(0.5)
    beats = {}
    for i in range(n):
        d = tmp_path / f"{i:03d}"
        d.mkdir()
        np.save(d / "mel.npy", smooth_mel(700 + i, 3 * T - 2, seed=7))
        np.save(d / "motion.npy", gts[i])
        beats[f"{i:03d}"] = (np.arange(3 * T - 2 - 5 * i) % (44 + i) == 7).astype(np.uint8)
    gen = Generator(DEV).load_state_dict(synthetic_m2sgan_state_dict(0), strict=True)
    menc = MotionEncoder_STGCN(DEV).load_state_dict(synthetic_motion_encoder_state_dict())
    m2s = M2SNet(DEV).load_state_dict(synthetic_m2snet_state_dict())

    class Checks:                                                    # a stub of the denoiser's switches: what evaluate_dataset saves and restores
        check_numerics = True
        combine_exchange = True

    class Poisoned(GeneratorBaseline):
        def __init__(self, generator, poison):
            super().__init__(generator)
            self.encoder, self.poison, self.calls, self.checked_calls = Checks(), poison, 0, 0

        def generate_music_motion(self, *a, **kw):
            k = self.calls
            self.calls += 1
            out = super().generate_music_motion(*a, **kw)
            if self.encoder.check_numerics:
                self.checked_calls += 1
            elif k == self.poison:
                out = out.clone()
                out[0, 5, 3] = float("inf")                           # (one overwritten element of the result: the kernels ran as always)
            return out

    def run(poison):
        tr = Poisoned(gen, poison)
        r = ev.evaluate_dataset(tr, str(tmp_path), 26, batch_size=2, seed=seed, verbose=False, motion_encoder=menc, m2snet=m2s,
                                retrieval=True, rhythm=rhythm, discriminator=critic, music_beats=beats, beat_stride=3)
        return tr, r

    timing = {"seconds", "frames_per_s", "steady_frames_per_s", "main_thread_s", "metrics_s", "m2s_retrieval_s"}
    _, clean = run(-1)
    assert {"fgd", "m2s_sync_gen", "m2s_mean_rank_gen", "rde", "w_distance", "bc_gen", "beat_align_real"} <= set(clean)
    tr, got = run(0)
    assert tr.checked_calls == 1 and tr.calls == 3 and tr.encoder.check_numerics is True and tr.encoder.combine_exchange is True
    assert list(got) == list(clean)
    for key in clean:
        if key not in timing:
            same = got[key] == clean[key] or (isinstance(clean[key], float) and np.isnan(clean[key]) and np.isnan(got[key]))
            assert same, (key, got[key], clean[key])


def test_evaluate_main_takes_the_new_flags_beside_the_generator(weights, tmp_path, capsys):
    """--rhythm and --discriminator PATH (a checkpoint with DataParallel keys) under --baseline_generator: one JSON line with the new
    keys beside the old ones; without the flags the line has none of them."""
    import json
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_m2sgan_state_dict, synthetic_motion
    T, n = 270, 2
    data = tmp_path / "data"
    for i in range(n):
        d = data / f"{i:03d}"
        d.mkdir(parents=True)
        np.save(d / "mel.npy", smooth_mel(800 + i, 3 * T - 2, seed=7))
        np.save(d / "motion.npy", synthetic_motion(1, T, seed=25, first=i)[0] + np.float32(0.5))
    gen_ckpt, disc_ckpt = str(tmp_path / "generator.pt"), str(tmp_path / "critic.pt")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_m2sgan_state_dict(0).items()}, gen_ckpt)
    torch.save({"module." + k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}, disc_ckpt)
    new = {"rde", "sce", "sd_gen", "sd_real", "w_distance", "rde_per_clip", "sce_per_clip"}
    lines = []
    for extra in ([], ["--rhythm", "--discriminator", disc_ckpt]):
        assert ev.main(["--data_root", str(data), "--baseline_generator", gen_ckpt, "--batch_size", "2", "--seed", "6", *extra]) == 0
        out = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    plain, r = lines
    assert not new & set(plain) and new <= set(r) and r["model"] == "m2sgan" and r["per_clip"] == plain["per_clip"]
    assert sorted(r["rde_per_clip"]) == sorted(r["per_clip"]) and all(np.isfinite(r[k]) for k in new if not k.endswith("per_clip"))
    assert r["rde"] > 0 and r["sce"] > 0 and r["sd_real"] > r["sd_gen"] > 0
