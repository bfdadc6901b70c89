"""Beat consistency on the MI355X (csrc/dc_rhythm.hip: dc_rhythm_motion_beats, dc_rhythm_beat_scores; rhythm.py, metrics.py,
evaluate.py) against the reference's one-hots, envelopes and scores of tests/golden/g18_beats.npz (tools/make_golden_beats.py), the
float32 restatement and the fp64 oracle of tests/helpers_beats.py.

Beats and envelopes are compared BIT FOR BIT, no frame excluded.

Bound of the scores (derived, not measured): a score is a mean of n terms in [0, 1], each an fp32 expf, summed in fp32 in some fixed
order, so |device - fp64| <= (n + 4) 2^-24 absolute (helpers_beats.score_bound), n the clip's term count - its music beats for BC,
its motion beats for Beat Align.  Against the reference's own float32 value in the fixture: twice that.  The oracle places music
beat i at exactly i / music_stride; the device divides the integer distance |i - music_stride m| once, so the placement costs one
rounding of d and is covered by the same bound.

Measured on the MI355X (profiles/beats_gpu_tests.txt): every frame of every case equal; largest score error against the fp64 oracle
3.35e-8 beside its bound of 2.98e-7, against the reference's float32 BC 3.7e-8 beside 1.8e-5."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_beats as H
from helpers import golden

from diffusion_conductor_amd import metrics
from diffusion_conductor_amd.native import NativeRhythm, lib
from diffusion_conductor_amd.rhythm import MotionRhythm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCHES = (1, 2, 3)


@pytest.fixture(scope="module")
def g18():
    return golden(H.FIXTURE)


@pytest.fixture(scope="module")
def rhythm():
    return MotionRhythm(DEV)


def _bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


@pytest.mark.parametrize("T", H.FIXTURE_T)
def test_beats_and_envelope_are_the_references_bit_for_bit(rhythm, g18, T):
    real, gen = H.fixture_pair(T)
    for name, m in (("real", real), ("gen", gen)):
        want_b, want_e = g18[f"beats_{name}_T{T}"], g18[f"envelope_{name}_T{T}"]
        # the float32 restatement: the loop version up to 300 frames, metrics' vectorised one (bit-equal to it: test_host_beats.py) at 1800
        rest_b, rest_e = H.beats_f32(m) if T <= 300 and name == "real" else metrics.motion_beats_host(m)
        for B in BATCHES:
            beats, env = rhythm.motion_beats(m[:B], envelope=True)
            assert tuple(beats.shape) == tuple(env.shape) == (B, T) and beats.dtype == torch.uint8 and env.dtype == torch.float32
            assert np.array_equal(_bits(env), _bits(want_e[:B])) and np.array_equal(_bits(env), _bits(rest_e[:B])), (name, T, B)
            assert np.array_equal(_np(beats), want_b[:B].astype(np.uint8)) and np.array_equal(_np(beats).astype(bool), rest_b[:B]), (name, T, B)
            assert torch.equal(rhythm.motion_beats(m[:B]), beats)               # the envelope in the workspace
        print(f"T={T} {name}: {int(want_b.sum())} beats, every frame of {H.CLIPS} clips equal at B = 1, 2, 3")


def test_a_clip_alone_in_a_batch_and_on_a_rerun(rhythm):
    for T in (257, 1800):
        x = torch.from_numpy(H.fixture_pair(T)[0]).to(DEV)
        alone = [t.clone() for t in rhythm.motion_beats(x[1:2], envelope=True)]
        batch = [t.clone() for t in rhythm.motion_beats(x, envelope=True)]
        flipped = rhythm.motion_beats(x.flip(0).contiguous(), envelope=True)
        again = rhythm.motion_beats(x, envelope=True)
        for i in range(2):
            assert torch.equal(batch[i][1], alone[i][0]) and torch.equal(flipped[i][1], alone[i][0]) and torch.equal(flipped[i][0], batch[i][2])
            assert torch.equal(again[i], batch[i])
    # more clips than one pass of 64, both calls, against the same clips one by one
    T, n = 40, 66
    x = torch.from_numpy(H.fixture_pair(T, n=n)[0]).to(DEV)
    mus = torch.from_numpy(np.stack([np.roll(H.fixture_music(T), 3 * b) for b in range(n)])).to(DEV)
    beats, env = rhythm.motion_beats(x, envelope=True)
    scores, counts = rhythm.beat_scores(beats, mus, counts=True)
    assert int(beats.sum()) >= 20
    for b in (0, 32, 63, 64, 65):
        b1, e1 = rhythm.motion_beats(x[b:b + 1], envelope=True)
        s1, c1 = rhythm.beat_scores(b1, mus[b:b + 1], counts=True)
        assert torch.equal(b1[0], beats[b]) and torch.equal(e1[0], env[b]) and torch.equal(c1[0], counts[b])
        assert np.array_equal(_bits(s1[0]), _bits(scores[b])), b


def test_lengths_shorter_than_the_clip_with_junk_behind(rhythm):
    T = 300
    real = H.fixture_pair(T)[0].copy()
    length = [200, 300, 12]
    real[0, 200:] = np.nan
    real[2, 12:] = 1e30
    beats, env = rhythm.motion_beats(real, length=length, envelope=True)
    rest_b, rest_e = metrics.motion_beats_host(real, length=length)
    assert np.array_equal(_np(beats).astype(bool), rest_b) and np.array_equal(_bits(env), _bits(rest_e))
    for b, L in enumerate(length):
        b1, e1 = rhythm.motion_beats(np.ascontiguousarray(real[b:b + 1, :L]), envelope=True)
        assert torch.equal(b1[0], beats[b, :L]) and torch.equal(e1[0], env[b, :L])
        assert not bool(beats[b, L:].any()) and not bool(env[b, L:].any()) and not bool(beats[b, L - 1])
    assert int(beats[0].sum()) >= 5 and int(beats[2].sum()) == 0
    with pytest.raises(ValueError):
        rhythm.motion_beats(real, length=[200, 301, 12])
    with pytest.raises(ValueError):
        rhythm.motion_beats(real, length=[200, 300])


def test_strict_minima_where_every_operation_is_exact(rhythm):
    """y constant, x on a 2^-10 grid: no result can depend on a summation order (helpers_beats.exact_case)."""
    motion, env_exact, want = H.exact_case()
    beats, env = rhythm.motion_beats(motion, envelope=True)
    assert np.array_equal(_bits(env[0]), _bits(env_exact))
    got = list(np.flatnonzero(_np(beats[0])))
    assert got == [40, 51, 80] and np.array_equal(_np(beats[0]).astype(bool), want), got      # no plateau (20, 21), not 70 (80 is 10 away)
    assert list(np.flatnonzero(_np(rhythm.motion_beats(motion, order=11)[0]))) == [51, 80]       # 40 now sees frame 51
    for order in (1, 9, 64):
        assert np.array_equal(_np(rhythm.motion_beats(motion, order=order)[0]).astype(bool), H.minima(env_exact, order)), order
    for order in (0, 65):
        with pytest.raises(ValueError):
            rhythm.motion_beats(motion, order=order)


def _music_kinds(Lm):
    sparse, dense, absent, single = np.zeros(Lm, np.uint8), np.ones(Lm, np.uint8), np.zeros(Lm, np.uint8), np.zeros(Lm, np.uint8)
    sparse[::37] = 1
    single[Lm // 2] = 1
    return np.stack([sparse, dense, absent, single])


def _check_scores(scores, counts, mus, mot, stride, sigma, worst):
    for b in range(mus.shape[0]):
        bc, ba, n_mus, n_mot = H.scores_f64(mus[b], mot[b], stride, sigma)
        assert tuple(counts[b]) == (n_mus, n_mot)
        for got, want, n, what in ((scores[b, 0], bc, n_mus, "BC"), (scores[b, 1], ba, n_mot, "Beat Align")):
            where = (what, b, n_mus, n_mot, stride, sigma, mus.shape[1], mot.shape[1])
            if np.isnan(want):
                assert np.isnan(got), where
            elif n_mus == 0 or n_mot == 0:
                assert got == 0 and want == 0, where
            else:
                err = abs(float(got) - want)
                if err / H.score_bound(n) > worst["ratio"]:
                    worst.update(ratio=err / H.score_bound(n), err=err, bound=H.score_bound(n), where=where)
                assert err <= H.score_bound(n), (err, H.score_bound(n), where)


def test_scores_against_the_fp64_oracle(rhythm, g18):
    """Lm in {1, 37, 256, 257, 3 T, 5400}; music beats sparse (one every 37 frames), dense (Lm terms), absent, single; motion beats the
    fixture's and absent; music_stride in {1, 3}, sigma in {1, 3}; and both one-hots dense (every tile of the compaction full)."""
    worst = {"ratio": -1.0}
    for T, name, clip in ((300, "real", 0), (1800, "gen", 1)):
        beats = g18[f"beats_{name}_T{T}"][clip].astype(np.uint8)
        mot = np.stack([beats] * 4 + [np.zeros(T, np.uint8)] * 4)
        for Lm in sorted({1, 37, 256, 257, 3 * T, 5400}):
            mus = np.concatenate([_music_kinds(Lm)] * 2)
            for stride in (1, 3):
                for sigma in (1, 3):
                    scores, counts = rhythm.beat_scores(mot, mus, music_stride=stride, sigma=sigma, counts=True)
                    assert tuple(scores.shape) == tuple(counts.shape) == (8, 2) and scores.dtype == torch.float32 and counts.dtype == torch.int32
                    _check_scores(_np(scores), _np(counts), mus, mot, stride, sigma, worst)
    for T, Lm in ((257, 257), (257, 5400), (1, 1), (22, 66)):
        mot, mus = np.ones((1, T), np.uint8), np.ones((1, Lm), np.uint8)
        for stride in (1, 3):
            scores, counts = rhythm.beat_scores(mot, mus, music_stride=stride, sigma=1, counts=True)
            _check_scores(_np(scores), _np(counts), mus, mot, stride, 1, worst)
    print(f"largest score error {worst['err']:.3e} beside its derived bound {worst['bound']:.3e} ({worst['ratio']:.3f} of it) at "
          f"(score, row, music beats, motion beats, stride, sigma, Lm, T) = {worst['where']}")


@pytest.mark.parametrize("T", H.SCORED_T)
def test_scores_of_the_device_beats_against_the_references(rhythm, g18, T):
    real, gen = H.fixture_pair(T)
    mus = np.tile(H.fixture_music(T), (H.CLIPS, 1))
    n_mus = int(mus[0].sum())
    for name, m in (("real", real), ("gen", gen)):
        beats = rhythm.motion_beats(m)
        scores = _np(rhythm.beat_scores(beats, mus))
        ref32 = g18[f"bc_{name}_T{T}"]
        ref64 = np.array([H.scores_f64(mus[i], g18[f"beats_{name}_T{T}"][i])[0] for i in range(H.CLIPS)])
        e32, e64 = np.abs(scores[:, 0] - ref32).max(), np.abs(scores[:, 0] - ref64).max()
        print(f"T={T} {name}: BC {scores[:, 0]}  against the reference's float32 {e32:.2e} (bound {2 * H.score_bound(n_mus):.2e})  "
              f"against fp64 {e64:.2e} (bound {H.score_bound(n_mus):.2e})")
        assert e32 <= 2 * H.score_bound(n_mus) and e64 <= H.score_bound(n_mus)
        assert 0.02 < scores[:, 0].min() and scores[:, 0].max() < 0.98
        # zeros behind the last music beat change nothing, bit for bit; the host restatement keeps the same order
        padded = np.concatenate([mus, np.zeros((H.CLIPS, 777), np.uint8)], axis=1)
        assert np.array_equal(_bits(rhythm.beat_scores(beats, padded)), _bits(scores))
        host = metrics.beat_alignment_host(mus, _np(beats))
        assert np.abs(host - scores).max() <= 2 * H.score_bound(n_mus)


def test_refusals_come_before_any_launch():
    L, stream = lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: t.data_ptr()      # noqa: E731
    x = torch.zeros(2, 50, 26, device=DEV)
    env = torch.full((2, 50), 7.0, device=DEV)
    beats = torch.full((2, 50), 7, dtype=torch.uint8, device=DEV)
    mus = torch.ones((2, 150), dtype=torch.uint8, device=DEV)
    scores = torch.full((2, 2), 7.0, device=DEV)
    counts = torch.full((2, 2), 7, dtype=torch.int32, device=DEV)
    r = NativeRhythm(0)
    lens = lambda *v: (C.c_int32 * len(v))(*v)      # noqa: E731
    mb = lambda h, m, ln, B, T, order, e, b: L.dc_rhythm_motion_beats(h, m, ln, B, T, order, e, b, stream)      # noqa: E731
    assert mb(r._h, ptr(x), None, 0, 50, 10, ptr(env), ptr(beats)) == -1 and mb(r._h, ptr(x), None, 2, 0, 10, ptr(env), ptr(beats)) == -1
    assert mb(r._h, ptr(x), None, 2, 50, 0, ptr(env), ptr(beats)) == -1 and mb(r._h, ptr(x), None, 2, 50, 65, ptr(env), ptr(beats)) == -1
    assert mb(r._h, ptr(x), lens(50, 0), 2, 50, 10, ptr(env), ptr(beats)) == -1 and mb(r._h, ptr(x), lens(51, 50), 2, 50, 10, ptr(env), ptr(beats)) == -1
    assert mb(None, ptr(x), None, 2, 50, 10, ptr(env), ptr(beats)) == -1 and mb(r._h, None, None, 2, 50, 10, ptr(env), ptr(beats)) == -1
    assert mb(r._h, ptr(x), None, 2, 50, 10, ptr(env), None) == -1
    assert b"length" in L.dc_last_error() or b"NULL" in L.dc_last_error()
    bs = lambda h, m, B, T, u, Lm, s, sg, sc, c: L.dc_rhythm_beat_scores(h, m, B, T, u, Lm, s, C.c_float(sg), sc, c, stream)      # noqa: E731
    ok = (r._h, ptr(beats), 2, 50, ptr(mus), 150, 1, 3.0, ptr(scores), ptr(counts))
    for at, bad in ((2, 0), (3, 0), (5, 0), (6, 0), (7, 0.0), (7, -1.0), (7, float("nan")), (7, float("inf")), (0, None), (1, None), (4, None), (8, None)):
        args = list(ok)
        args[at] = bad
        assert bs(*args) == -1, (at, bad)
    torch.cuda.synchronize()
    assert bool((env == 7).all()) and bool((beats == 7).all()) and bool((scores == 7).all()) and bool((counts == 7).all())
    # the accepted edges: one clip of one frame, order 64, NULL envelope, NULL counts, lengths at both ends
    assert mb(r._h, ptr(x), lens(1, 50), 2, 50, 64, None, ptr(beats)) == 0
    assert bs(r._h, ptr(beats), 2, 50, ptr(mus), 150, 3, 1.0, ptr(scores), None) == 0
    assert mb(r._h, ptr(x), None, 1, 1, 1, ptr(env), ptr(beats)) == 0
    torch.cuda.synchronize()
    assert not bool(beats.any()) and bool((scores[:, 0] == 0).all()) and bool(torch.isnan(scores[:, 1]).all()) and bool((counts == 7).all())
    r.close()


def _dataset(root, n, T):
    from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_motion
    gts = synthetic_motion(n, T, seed=26) + np.float32(0.5)
    for i in range(n):
        d = root / f"{i:03d}"
        d.mkdir(parents=True)
        np.save(d / "mel.npy", smooth_mel(900 + i, 3 * T - 2, seed=7))
        np.save(d / "motion.npy", gts[i])
    # music beats of different lengths (a batch pads to its longest), a beat every 23 / 29 / 31 mel frames
    music = {f"{i:03d}": np.zeros(3 * T - 2 - 40 * i, np.float32) for i in range(n)}
    for i, m in enumerate(music.values()):
        m[4 + i::(23, 29, 31)[i % 3]] = 1.0
    return gts, music


def test_through_the_evaluator(rhythm, tmp_path):
    """evaluate_dataset(music_beats=) on the M2S-GAN generator as the trainer: bc_* are the two calls made by hand on the poses the run
    itself made, and without the argument the result has exactly the keys it had."""
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.generator import Generator, GeneratorBaseline
    from diffusion_conductor_amd.synthetic import synthetic_m2sgan_state_dict
    T, n, seed = 270, 3, 6
    gts, music = _dataset(tmp_path, n, T)
    gen = Generator(DEV).load_state_dict(synthetic_m2sgan_state_dict(0), strict=True)
    made = []

    class Recording(GeneratorBaseline):
        def generate_music_motion(self, *a, **kw):
            made.append(super().generate_music_motion(*a, **kw).clone())
            return made[-1]
    base = Recording(gen)
    plain = ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=2, seed=seed, verbose=False)
    timing = {"seconds", "frames_per_s", "main_thread_s", "steady_frames_per_s"}
    assert set(plain) - timing == {"per_clip", "total_loss", "final_mse", "clips"}
    del made[:]
    r = ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=2, seed=seed, verbose=False, music_beats=music)
    new = {"bc_gen", "bc_real", "bc_gen_per_clip", "bc_real_per_clip", "beat_align_gen", "beat_align_real"}
    assert set(r) - timing == (set(plain) - timing) | new
    for k in set(plain) - timing:
        assert r[k] == plain[k], k
    poses = torch.cat(made).reshape(n, T, 26)
    ids = sorted(r["per_clip"])
    mus = np.zeros((n, max(m.size for m in music.values())), np.uint8)
    for i, cid in enumerate(ids):
        mus[i, :music[cid].size] = music[cid] != 0
    for stride, res in ((1, r), (3, ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=1, seed=seed, verbose=False, music_beats=music,
                                                        beat_stride=3, rhythm=None))):
        for name, x in (("gen", poses), ("real", gts)):
            beats = rhythm.motion_beats(x)
            s, c = rhythm.beat_scores(beats, mus, music_stride=stride, counts=True)
            s = _np(s)
            print(f"evaluate_dataset stride {stride} {name}: motion beats {_np(c)[:, 1]}  BC {s[:, 0]}  Beat Align {s[:, 1]}")
            assert res[f"bc_{name}_per_clip"] == {cid: float(s[i, 0]) for i, cid in enumerate(ids)}, (stride, name)
            assert res[f"bc_{name}"] == float(s[:, 0].astype(np.float64).mean())
            assert _same(res[f"beat_align_{name}"], float(s[:, 1].astype(np.float64).mean()))
            assert 0 <= res[f"bc_{name}"] < 1 and [int(v) for v in _np(c)[:, 0]] == [int((music[cid] != 0).sum()) for cid in ids]
            if name == "real":                                         # (how many beats the seeded generator's poses have is not this test's to say)
                assert int(beats.sum(dim=1).min()) >= 3 and res["bc_real"] > 0
            for i in range(n):                                         # and the oracle, on the device's beats
                bc64 = H.scores_f64(mus[i], _np(beats[i]), stride)
                assert abs(s[i, 0] - bc64[0]) <= H.score_bound(bc64[2]) and abs(s[i, 1] - bc64[1]) <= H.score_bound(bc64[3])
    assert r["bc_gen_per_clip"] != r["bc_real_per_clip"]
    # the same scores beside the other movement scores, on the caller's MotionRhythm
    both = ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=2, seed=seed, verbose=False, music_beats=music, rhythm=rhythm)
    assert all(both[k] == r[k] or _same(both[k], r[k]) for k in new) and "rde" in both


def test_evaluate_main_takes_beats_beside_the_generator(tmp_path, capsys):
    import json
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.synthetic import synthetic_m2sgan_state_dict
    T, n = 270, 2
    _, music = _dataset(tmp_path / "data", n, T)
    np.savez(tmp_path / "beats.npz", **music)
    ckpt = str(tmp_path / "generator.pt")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_m2sgan_state_dict(0).items()}, ckpt)
    lines = []
    for extra in ([], ["--beats", str(tmp_path / "beats.npz")], ["--beats", str(tmp_path / "beats.npz"), "--beat_stride", "3"]):
        assert ev.main(["--data_root", str(tmp_path / "data"), "--baseline_generator", ckpt, "--batch_size", "2", "--seed", "6", *extra]) == 0
        out = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    plain, r, r3 = lines
    new = {"bc_gen", "bc_real", "bc_gen_per_clip", "bc_real_per_clip", "beat_align_gen", "beat_align_real"}
    assert not new & set(plain) and new <= set(r) and r["per_clip"] == plain["per_clip"] and sorted(r["bc_gen_per_clip"]) == sorted(r["per_clip"])
    assert 0 <= r["bc_gen"] < 1 and 0 < r["bc_real"] < 1 and r3["bc_real"] != r["bc_real"]
