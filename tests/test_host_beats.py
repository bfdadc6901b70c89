"""Beat consistency's host surface on a CPU-only box: metrics.motion_beats_host and beat_alignment_host against the reference's
one-hots, envelopes and scores in tests/golden/g18_beats.npz (tools/make_golden_beats.py: the reference's motion_peak_onehot and
alignment_score on seeded inputs) and against tests/helpers_beats.py, the .npz loader, beat_consistency, and evaluate.main's
argument rules.

Bound of the scores (derived, not measured): a score is a mean of n terms in [0, 1], each an fp32 exp, summed in fp32 in some fixed
order, so |fp32 value - fp64 oracle| <= (n + 4) 2^-24 absolute (helpers_beats.score_bound), n the clip's term count; against the
reference's own float32 value - the same kind of number - twice that."""
import numpy as np
import pytest

import helpers_beats as H
from helpers import golden

from diffusion_conductor_amd import metrics
from diffusion_conductor_amd.synthetic import array_digest


@pytest.fixture(scope="module")
def g18():
    return golden(H.FIXTURE)


def test_fixture_inputs_regenerate_from_their_seeds(g18):
    assert tuple(g18["lengths"]) == H.FIXTURE_T and tuple(g18["scored_lengths"]) == H.SCORED_T
    assert (int(g18["real_seed"]), int(g18["gen_seed"])) == (H.REAL_SEED, H.GEN_SEED)
    for T in H.FIXTURE_T:
        real, gen = H.fixture_pair(T)
        assert real.shape == gen.shape == (H.CLIPS, T, 13, 2) and real.dtype == gen.dtype == np.float32
        assert np.array_equal(array_digest(real), g18[f"real_digest_T{T}"]) and np.array_equal(array_digest(gen), g18[f"gen_digest_T{T}"])
    for T in H.SCORED_T:
        assert np.array_equal(array_digest(H.fixture_music(T)), g18[f"music_digest_T{T}"])


@pytest.mark.parametrize("T", H.FIXTURE_T)
def test_host_beats_and_envelope_are_the_references_bit_for_bit(g18, T):
    real, gen = H.fixture_pair(T)
    for name, m in (("real", real), ("gen", gen)):
        beats, env = metrics.motion_beats_host(m)
        assert beats.dtype == bool and env.dtype == np.float32 and beats.shape == env.shape == (H.CLIPS, T)
        assert np.array_equal(beats, g18[f"beats_{name}_T{T}"])
        assert np.array_equal(env.view(np.uint32), g18[f"envelope_{name}_T{T}"].view(np.uint32))
        if T <= 300:                                                    # (the loop restatement is slow at 1800: the GPU test's)
            b2, e2 = H.beats_f32(m)
            assert np.array_equal(b2, beats) and np.array_equal(e2.view(np.uint32), env.view(np.uint32))
        one, e1 = metrics.motion_beats_host(m[1])                       # a clip alone, [T, 13, 2]
        assert np.array_equal(one[0], beats[1]) and np.array_equal(e1[0], env[1])
    if T >= 300:
        assert g18[f"beats_real_T{T}"].sum(axis=1).min() >= 5 and not np.array_equal(g18[f"beats_real_T{T}"], g18[f"beats_gen_T{T}"])
    if T <= 12:
        assert not g18[f"beats_real_T{T}"].any() and not g18[f"beats_gen_T{T}"].any()


def test_host_beats_respect_a_length_and_the_strict_rules():
    real = H.fixture_pair(300)[0].copy()
    real[0, 200:] = np.nan                                              # junk behind the length
    beats, env = metrics.motion_beats_host(real, length=[200, 300, 257])
    alone, e_alone = metrics.motion_beats_host(real[0, :200])
    assert np.array_equal(beats[0, :200], alone[0]) and np.array_equal(env[0, :200], e_alone[0])
    assert not beats[0, 200:].any() and not env[0, 200:].any() and not beats[2, 257:].any() and not beats[:, 0].any()
    assert not beats[0, 199] and not beats[1, 299] and not beats[2, 256] and not beats[:, :11].any()
    motion, env_exact, want = H.exact_case()
    beats, env = metrics.motion_beats_host(motion)
    assert np.array_equal(env[0], env_exact) and np.array_equal(beats[0], want) and list(np.flatnonzero(want)) == [40, 51, 80]
    assert np.array_equal(H.beats_f32(motion)[0][0], want)
    assert list(np.flatnonzero(metrics.motion_beats_host(motion, order=11)[0][0])) == [51, 80]      # 40 now sees the lower 51
    for bad in ({"order": 0}, {"order": 65}, {"length": [0]}, {"length": [101]}, {"length": [50, 50]}):
        with pytest.raises(ValueError):
            metrics.motion_beats_host(motion, **bad)
    with pytest.raises(ValueError):
        metrics.motion_beats_host(np.zeros((2, 30, 25), np.float32))


@pytest.mark.parametrize("T", H.SCORED_T)
def test_host_scores_against_the_reference_and_the_fp64_oracle(g18, T):
    mus = H.fixture_music(T)
    for name in ("real", "gen"):
        beats = g18[f"beats_{name}_T{T}"]
        got = metrics.beat_alignment_host(np.tile(mus, (H.CLIPS, 1)), beats)
        assert got.dtype == np.float32 and got.shape == (H.CLIPS, 2)
        for i in range(H.CLIPS):
            bc, ba, n_mus, n_mot = H.scores_f64(mus, beats[i])
            assert abs(got[i, 0] - bc) <= H.score_bound(n_mus) and abs(got[i, 1] - ba) <= H.score_bound(n_mot)
            assert abs(got[i, 0] - g18[f"bc_{name}_T{T}"][i]) <= 2 * H.score_bound(n_mus)
            assert np.array_equal(metrics.beat_alignment_host(mus, beats[i]), got[i])
            for stride, sigma in ((3, 3), (1, 1), (3, 1)):
                g2 = metrics.beat_alignment_host(mus, beats[i], sigma=sigma, music_stride=stride)
                r2 = H.scores_f64(mus, beats[i], stride, sigma)
                assert abs(g2[0] - r2[0]) <= H.score_bound(n_mus) and abs(g2[1] - r2[1]) <= H.score_bound(n_mot), (stride, sigma)
        assert 0.02 < g18[f"bc_{name}_T{T}"].min() and g18[f"bc_{name}_T{T}"].max() < 0.98


def test_empty_cases_and_beat_consistency():
    mot = np.zeros(60, np.uint8)
    mot[[15, 40]] = 1
    mus = np.zeros(180, np.uint8)
    mus[[14, 44, 100]] = 1
    none_t, none_m = np.zeros(60, np.uint8), np.zeros(180, np.uint8)
    full = metrics.beat_alignment_host(mus, mot)
    assert 0 < full[0] < 1 and 0 < full[1] < 1
    assert abs(full[0] - H.scores_f64(mus, mot)[0]) <= H.score_bound(3) and abs(full[1] - H.scores_f64(mus, mot)[1]) <= H.score_bound(2)
    no_motion = metrics.beat_alignment_host(mus, none_t)                # the reference returns 0.0 before it looks at the music
    assert no_motion[0] == 0 and np.isnan(no_motion[1])
    no_music = metrics.beat_alignment_host(none_m, mot)                 # the reference divides by zero
    assert np.isnan(no_music[0]) and no_music[1] == 0
    assert np.array_equal(metrics.beat_alignment_host(none_m, none_t), [0, 0])
    assert np.isnan(H.scores_f64(none_m, mot)[0]) and H.scores_f64(mus, none_t)[0] == 0
    # zeros behind the last music beat change nothing, bit for bit; one-hots may be bool or float
    assert np.array_equal(metrics.beat_alignment_host(np.concatenate([mus, np.zeros(700, np.uint8)]), mot), full)
    assert np.array_equal(metrics.beat_alignment_host(mus.astype(bool), mot.astype(np.float32) * 0.5), full)
    scores = np.stack([full, no_motion, full])
    counts = np.array([[3, 2], [3, 0], [3, 2]])
    mean, per = metrics.beat_consistency(scores, counts, ["a", "b", "c"])
    assert per == {"a": float(full[0]), "b": 0.0, "c": float(full[0])} and mean == float(np.float64(full[0]) * 2 / 3)
    assert np.isnan(metrics.beat_consistency(scores, counts, ["a", "b", "c"], column=1)[0])
    with pytest.raises(ValueError, match="no music beat.*'b'"):
        metrics.beat_consistency(np.stack([full, no_music]), np.array([[3, 2], [0, 2]]), ["a", "b"])
    with pytest.raises(ValueError):
        metrics.beat_consistency(scores, counts, ["a", "b"])
    for bad in ({"music_stride": 0}, {"sigma": 0}, {"sigma": float("inf")}):
        with pytest.raises(ValueError):
            metrics.beat_alignment_host(mus, mot, **bad)


def test_load_music_beats_and_its_refusals(tmp_path):
    path = str(tmp_path / "beats.npz")
    a = np.zeros(30, np.float32)
    a[[3, 9]] = 1.0
    np.savez(path, clip0=a, clip1=a.astype(bool), clip2=(a * 7).astype(np.uint8), flat=np.zeros((2, 15)), scalar=np.float32(1))
    got = metrics.load_music_beats(path, ["clip0", "clip1", "clip2"])
    assert list(got) == ["clip0", "clip1", "clip2"]
    for v in got.values():
        assert v.dtype == np.uint8 and v.shape == (30,) and list(np.flatnonzero(v)) == [3, 9] and v.max() == 1
    with pytest.raises(ValueError, match="no music beats for 1 clip.*clip9"):
        metrics.load_music_beats(path, ["clip0", "clip9"])
    with pytest.raises(ValueError, match="flat.*1-D"):
        metrics.load_music_beats(path, ["clip0", "flat"])
    with pytest.raises(ValueError, match="scalar.*1-D"):
        metrics.load_music_beats(path, ["scalar"])


def test_evaluate_main_argument_clashes(capsys):
    from diffusion_conductor_amd import evaluate
    for flags, word in ((["--val_loss", "--beats", "b.npz"], "--val_loss"), (["--val_loss", "--beat_stride", "3"], "--val_loss"),
                        (["--beat_stride", "3"], "--beats"), (["--beats", "b.npz", "--beat_stride", "0"], ">= 1")):
        with pytest.raises(SystemExit) as e:
            evaluate.main(["--data_root", "nowhere", *flags])
        assert e.value.code == 2 and word in capsys.readouterr().err, flags
    # under --baseline_generator both flags parse: the refusal is still the denoiser's flag, not the beats
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--data_root", "nowhere", "--baseline_generator", "g.pt", "--beats", "b.npz", "--beat_stride", "3", "--steps", "5"])
    err = capsys.readouterr().err
    assert e.value.code == 2 and "--steps" in err and "--beats" not in err.split("error:")[1]


def test_evaluate_dataset_refuses_bad_music_beats_before_sampling(tmp_path):
    from diffusion_conductor_amd.evaluate import evaluate_dataset
    rng = np.random.default_rng(3)
    for i in range(2):
        d = tmp_path / f"clip{i}"
        d.mkdir()
        np.save(d / "mel.npy", rng.random((70, 128), dtype=np.float32))
        np.save(d / "motion.npy", rng.standard_normal((24, 13, 2)).astype(np.float32))

    class Never:
        device = encoder = None

        def generate_music_motion(self, *a, **kw):
            raise AssertionError("sampled before the music beats were checked")
    beat = np.zeros(70, np.uint8)
    beat[5] = 1
    for beats, match in (({"clip0": beat}, "no entry for 1 clip.*clip1"), ({"clip0": beat, "clip1": np.zeros((2, 35))}, "1-D"),
                         ({"clip0": beat, "clip1": np.zeros(70)}, "no music beat in 1 clip.*clip1")):
        with pytest.raises(ValueError, match=match):
            evaluate_dataset(Never(), str(tmp_path), batch_size=2, verbose=False, music_beats=beats)
    with pytest.raises(ValueError, match="beat_stride"):
        evaluate_dataset(Never(), str(tmp_path), batch_size=2, verbose=False, music_beats={"clip0": beat, "clip1": beat}, beat_stride=0)
