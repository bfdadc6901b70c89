"""The rhythm and realism scores' host surface on a CPU-only box: the fp64 restatements of tests/helpers_rhythm.py against the
reference's values in tests/golden/g16_rhythm.npz (tools/make_golden_rhythm.py: the reference's rhythm_density_error,
strengh_contour_error, torch.std and Discriminator_1DCNN on seeded inputs), metrics.py's three functions on the fixture's arrays,
the critic's image and the Welch table (csrc/dc_pack.h through tests/disc_pack_probe.cpp), and evaluate_dataset's unchanged result
without the new arguments."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import helpers_rhythm as H
from helpers import ROOT, golden

from diffusion_conductor_amd import metrics, native
from diffusion_conductor_amd.discriminator import Discriminator_1DCNN, discriminator_shapes
from diffusion_conductor_amd.synthetic import array_digest, synthetic_discriminator_state_dict

PSD_T = [T for T in H.FIXTURE_T if T >= H.MIN_PSD_T]
CONTOUR_T = [T for T in H.FIXTURE_T if T >= H.MIN_CONTOUR_T]


@pytest.fixture(scope="module")
def g16():
    return golden(H.FIXTURE)


@pytest.fixture(scope="module")
def weights():
    return synthetic_discriminator_state_dict(0)


def test_param_spec_and_seeded_weights_match_the_reference(g16, weights):
    spec = discriminator_shapes()
    assert len(spec) == 12 and list(spec) == [str(k) for k in g16["keys"]]
    assert [str(tuple(s)) for s in spec.values()] == [str(s) for s in g16["shapes"]]
    assert sum(int(np.prod(s)) for s in spec.values()) == 52641
    assert list(weights) == list(spec) and all(tuple(np.shape(v)) == spec[k] for k, v in weights.items())
    assert np.array_equal(np.stack([array_digest(v) for v in weights.values()]), g16["weight_digest"])


def test_fixture_motions_regenerate_from_their_seeds(g16):
    assert tuple(g16["lengths"]) == H.FIXTURE_T and (int(g16["real_seed"]), int(g16["gen_seed"])) == (H.REAL_SEED, H.GEN_SEED)
    for T in H.FIXTURE_T:
        real, gen = H.fixture_pair(T)
        assert real.shape == gen.shape == (2, T, 13, 2) and real.dtype == gen.dtype == np.float32
        assert np.array_equal(array_digest(real), g16[f"real_digest_T{T}"]) and np.array_equal(array_digest(gen), g16[f"gen_digest_T{T}"])
        assert 0.3 < abs(float(real.mean())) < 0.7            # the offset the detrend has to remove


@pytest.mark.parametrize("T", PSD_T)
def test_welch_restatement_reproduces_scipy_and_rde(g16, T):
    """Within the reference's own fp32 rounding (`ref_vs_fp64_*`, the maximum over all lengths) plus 1e-9."""
    real, gen = H.fixture_pair(T)
    p_real, p_gen = H.welch_psd(real), H.welch_psd(gen)
    assert p_real.shape == (2, 32)
    assert H.psd_error(g16[f"psd_real_T{T}"], p_real) <= float(g16["ref_vs_fp64_psd"]) + 1e-9
    assert H.psd_error(g16[f"psd_gen_T{T}"], p_gen) <= float(g16["ref_vs_fp64_psd"]) + 1e-9
    assert np.abs(H.rde(p_real, p_gen) - g16[f"rde_T{T}"]).max() <= float(g16["ref_vs_fp64_rde"]) + 1e-9


def test_welch_restatement_on_a_known_spectrum():
    """A sine at bin 10 of the 256-point segment on an offset: the Hann window spreads it over bins 9 .. 11 and nowhere else, the
    offset is gone, and with density scaling the spectrum sums to the sine's power: sum(PSD) fs / 256 = A^2 / 2."""
    n = np.arange(1800)
    x = np.zeros((1, 1800, 26))
    x[0, :, 3] = 0.7 + 0.2 * np.sin(2 * np.pi * 10 * n / 256)
    p = H.welch_psd(x)[0] * 26                                  # undo the channel average: one live channel
    assert p.argmax() == 10 and p[:8].max() < 1e-20 * p[10] + 1e-25 and p[13:].max() < 1e-20 * p[10] + 1e-25
    assert abs(p.sum() * H.FS / 256 - 0.2 ** 2 / 2) < 1e-12


@pytest.mark.parametrize("T", CONTOUR_T)
def test_contour_and_sd_restatements_reproduce_the_reference(g16, T):
    real, gen = H.fixture_pair(T)
    c_real, c_gen = H.contour(real), H.contour(gen)
    assert c_real.shape == (2, (T - 60) // 30 + 1)
    assert np.abs(H.sce(c_real, c_gen) - g16[f"sce_T{T}"]).max() <= float(g16["ref_vs_fp64_sce"]) + 1e-9
    assert np.abs(H.sd(real) - g16[f"sd_real_T{T}"]).max() <= float(g16["ref_vs_fp64_sd"]) + 1e-9
    assert np.abs(H.sd(gen) - g16[f"sd_gen_T{T}"]).max() <= float(g16["ref_vs_fp64_sd"]) + 1e-9


@pytest.mark.parametrize("T", H.FIXTURE_T)
def test_critic_restatement_reproduces_the_reference(g16, weights, T):
    real, gen = H.fixture_pair(T)
    f = H.critic_features(weights, real)
    assert f.shape == (2, 64, H.pooled_frames(T)[2]) == g16[f"features_T{T}"].shape
    assert np.abs(f - g16[f"features_T{T}"]).max() <= float(g16["ref_vs_fp64_features"])
    assert np.abs(H.critic_score(weights, features=f) - g16[f"d_real_T{T}"]).max() <= float(g16["ref_vs_fp64_score"])
    assert np.abs(H.critic_score(weights, gen) - g16[f"d_gen_T{T}"]).max() <= float(g16["ref_vs_fp64_score"])


def _torch_critic_features(weights, x):
    """Discriminator_1DCNN.motion_encoder with torch's own operators on the CPU in fp32: [B, T, 13, 2] -> [B, 64, L3]."""
    F = torch.nn.functional
    h = torch.from_numpy(np.asarray(x, np.float32)).flatten(start_dim=2).transpose(1, 2)
    for i, stride in ((0, 3), (3, 2), (6, 2)):
        w, b = (torch.from_numpy(np.asarray(weights[f"motion_encoder.{i}.{leaf}"], np.float32)) for leaf in ("weight", "bias"))
        h = F.max_pool1d(torch.relu(F.conv1d(h, w, b, padding=2)), kernel_size=5, stride=stride)
    return h.numpy()


def _torch_contour(x):
    """strengh_contour_error's contour of one batch (loss.py:129-141) with torch on the CPU in fp32: [B, T, 13, 2] -> [B, W]."""
    m = torch.from_numpy(np.asarray(x, np.float32))
    v = torch.zeros_like(m)
    v[:, 1:] = m[:, :-1] - m[:, 1:]
    v = torch.abs(v.flatten(start_dim=2).mean(dim=2))
    return torch.nn.functional.avg_pool1d(v.unsqueeze(0), kernel_size=60, stride=30).squeeze(0).numpy()


def test_the_oracles_non_finite_values_are_torchs(weights):
    """What the GPU tests of non-finite inputs compare against is torch's: on every poisoned input of tests/test_gpu_rhythm_edges.py the
    fp64 restatement's NaN / +inf / -inf / finite classes are, element by element, those of conv1d + relu + max_pool1d (the critic) and
    of avg_pool1d (the contour) on the CPU in fp32.  A maximum that returns its non-NaN operand (np.fmax, fmaxf) loses the NaN
    wherever a pool window also holds a finite frame: shown once, at T = 41 with the NaN on frame 21."""
    for T, frames in H.CRITIC_NAN_CASES:
        real = H.fixture_pair(T, n=3)[0]
        for t in frames:
            for value in (np.nan,) + ((np.inf, -np.inf) if T == 125 else ()):
                bad = H.poisoned(real, t, value)
                ref, got = H.critic_features(weights, bad), _torch_critic_features(weights, bad)
                assert got.shape == ref.shape
                assert np.array_equal(H.value_class(got), H.value_class(ref)), (T, t, value)
                assert not H.value_class(ref[[0, 2]]).any() and H.value_class(ref[1]).any(), (T, t, value)
                assert np.isnan(H.critic_score(weights, features=ref)[1]) and np.isfinite(H.critic_score(weights, features=ref)[[0, 2]]).all()
    y = np.maximum(np.asarray(H.poisoned(H.fixture_pair(41, n=3)[0], 21), np.float64).reshape(3, 41, 26)[1, :, H.POISON_CHANNEL], 0)
    assert np.isnan(y[3 * 6:3 * 6 + 5].max()) and np.isfinite(np.fmax.reduce(y[3 * 6:3 * 6 + 5]))
    T = 270
    real = H.fixture_pair(T, n=3)[0]
    for t, windows in ((95, (2, 3)), (0, (0,)), (T - 1, (7,))):
        bad = H.poisoned(real, t)
        ref, got = H.contour(bad), _torch_contour(bad)
        assert got.shape == ref.shape == (3, 8)
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and list(np.nonzero(np.isnan(ref[1]))[0]) == list(windows), (t, windows)
        assert not np.isnan(ref[[0, 2]]).any() and np.isnan(H.sd(bad)[1]) and np.isfinite(H.sd(bad)[[0, 2]]).all()
        assert np.isnan(torch.std(torch.from_numpy(bad).flatten(start_dim=2), dim=1).mean(dim=1).numpy()).tolist() == [False, True, False]


# SCE is a float32 logarithm of size <= 16 in the reference and in metrics.py alike, so neither can be closer to the exact value than
# the spacing of float32 there (9.5e-7 in [8, 16)).  Each chain - a float32 mean of at most 59 squares (torch's reduction order there,
# numpy's here: a few 6e-8 relative, which is the same absolute size in the logarithm), times 1e7, plus 1, log, each rounded once -
# is granted two spacings; the fixture's contours are the fp64 restatement's rounded to float32, which `ref_vs_fp64_sce` covers.
SCE_FP32_CHAINS = 4 * float(np.spacing(np.float32(8.0)))


def test_metrics_reproduce_the_fixtures_logged_values(g16):
    """metrics.py on the fixture's fp32 spectra and contours: the reference's arithmetic in the reference's dtypes.  RDE is numpy in
    both, on scipy's own spectra (bit-equal).  SCE is checked on contours that come from tests/helpers_rhythm.py, not from the
    reference (which never returns them), so it is the less independent of the two: within `ref_vs_fp64_sce` + SCE_FP32_CHAINS."""
    for T in PSD_T:
        per, mean = metrics.rhythm_density_error(g16[f"psd_real_T{T}"], g16[f"psd_gen_T{T}"])
        assert per.dtype == np.float64 and np.array_equal(per, g16[f"rde_T{T}"]) and mean == float(per.mean())
    for T in CONTOUR_T:
        per, mean = metrics.strength_contour_error(g16[f"contour_real_T{T}"], g16[f"contour_gen_T{T}"])
        assert per.dtype == np.float32 and per.shape == (2,)
        assert np.abs(per - g16[f"sce_T{T}"]).max() <= float(g16["ref_vs_fp64_sce"]) + SCE_FP32_CHAINS and mean == float(per.astype(np.float64).mean())
    T = 900
    w = metrics.w_distance(g16[f"d_real_T{T}"], g16[f"d_gen_T{T}"].reshape(2, 1))
    assert w == float((g16[f"d_real_T{T}"] - g16[f"d_gen_T{T}"]).astype(np.float64).mean()) and abs(w) > 1e-3
    with pytest.raises(ValueError):
        metrics.rhythm_density_error(np.zeros((2, 32)), np.zeros((3, 32)))
    with pytest.raises(ValueError):
        metrics.rhythm_density_error(np.zeros((2, 20)), np.zeros((2, 20)))
    with pytest.raises(ValueError):
        metrics.strength_contour_error(np.zeros((2, 5)), np.zeros((2, 6)))
    with pytest.raises(ValueError):
        metrics.w_distance(np.zeros(2), np.zeros(3))


# ---- the critic's image and the Welch table (csrc/dc_pack.h) through a host probe ------------------------------------------------
@pytest.fixture(scope="module")
def pack_probe(tmp_path_factory):
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"      # (dc_pack.h converts through _Float16: clang, the ROCm host compiler)
    if not os.path.exists(cxx):
        pytest.skip("no clang++")
    exe = str(tmp_path_factory.mktemp("disc_probe") / "probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", native.CSRC, os.path.join(ROOT, "tests", "disc_pack_probe.cpp"), "-o", exe], check=True)
    return exe


def test_disc_required_is_the_reference_state_dict(pack_probe, g16):
    rows = [l.split() for l in subprocess.run([pack_probe, "list"], check=True, capture_output=True, text=True).stdout.splitlines()]
    spec = discriminator_shapes()
    assert [r[0] for r in rows] == [str(k) for k in g16["keys"]]
    assert [int(r[1]) for r in rows] == [int(np.prod(s)) for s in spec.values()]


def _frags(W, mt_count):
    """lane-major A fragments of W [n][k]: out[mt][ks][l] = W[32 mt + (l & 31)][2 ks + (l >> 5)], 0 past n."""
    n, k = W.shape
    Wp = np.zeros((32 * mt_count, k))
    Wp[:n] = W
    lane = np.arange(64)
    return np.stack([np.stack([Wp[32 * mt + (lane & 31), 2 * ks + (lane >> 5)] for ks in range(k // 2)]) for mt in range(mt_count)])


def test_critic_image_is_the_permuted_weights(pack_probe, weights, tmp_path):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.concatenate([np.asarray(v, np.float32).ravel() for v in weights.values()]).tofile(src)
    off = [int(v) for v in subprocess.run([pack_probe, src, dst], check=True, capture_output=True, text=True).stdout.split()]
    img = np.fromfile(dst, np.float32)
    assert len(off) == 13 and img.size == off[12] and all(o % 64 == 0 for o in off[:12]) and sorted(off[:12]) == off[:12]
    covered = np.zeros(img.size, bool)

    def check(o, want):
        want = np.asarray(want, np.float64).ravel()
        assert not covered[o:o + want.size].any()
        covered[o:o + want.size] = True
        assert np.array_equal(img[o:o + want.size], want.astype(np.float32))      # a permutation: nothing is rounded
    for i in range(3):
        w = np.asarray(weights[f"motion_encoder.{3 * i}.weight"], np.float64)       # [64][cin][5]
        Wm = w.transpose(0, 2, 1).reshape(64, -1)                                   # column tap cin + ci
        check(off[2 * i], _frags(Wm, 2).transpose(1, 2, 0))                         # [ks][lane][tile]
        check(off[2 * i + 1], weights[f"motion_encoder.{3 * i}.bias"])
    for i in range(3):
        w = np.asarray(weights[f"fc.{2 * i}.weight"], np.float64)
        check(off[6 + 2 * i], _frags(w, 1))
        check(off[7 + 2 * i], np.concatenate([np.asarray(weights[f"fc.{2 * i}.bias"], np.float64), np.zeros(64 - w.shape[0])]))
    assert not img[~covered].any()


def test_welch_table_is_the_fp64_fold_rounded_once(pack_probe, tmp_path):
    dst = str(tmp_path / "table.bin")
    subprocess.run([pack_probe, "table", dst], check=True)
    tab = np.fromfile(dst, np.float32).reshape(64, 256)
    n, k = np.arange(256), np.arange(32)[:, None]
    w = 0.5 - 0.5 * np.cos(2 * np.pi * n / 256)
    g = np.sqrt(np.where(k == 0, 1.0, 2.0) / (30.0 * (w * w).sum()))
    arg = 2 * np.pi * ((k * n) % 256) / 256                                       # (reduced exactly, as the table's)
    want = np.concatenate([g * w * np.cos(arg), g * w * np.sin(arg)])
    # one fp32 rounding of the fp64 value; 1e-17: cos / sin at their zeros are a few 1e-17 in fp64, in libm and in numpy alike
    assert np.all(np.abs(tab - want) <= 2.0 ** -24 * np.abs(want) + 1e-17)
    assert tab[0, 0] == 0 and np.abs(tab[:32]).max() > 0.02 and np.all(tab[32] == 0)           # bin 0 has no sine
    # the table IS Welch: |cos row . x|^2 + |sin row . x|^2 of a detrended segment is the restatement's one-segment PSD
    x = H.fixture_pair(256)[0].reshape(2, 256, 26).astype(np.float64)
    d = x - x.mean(axis=1, keepdims=True)
    re, im = np.einsum("kn,bnc->bkc", tab[:32].astype(np.float64), d), np.einsum("kn,bnc->bkc", tab[32:].astype(np.float64), d)
    assert H.psd_error((re ** 2 + im ** 2).sum(axis=2) / 26, H.welch_psd(x)) <= 1e-6


class _StubTrainer:
    """generate_music_motion's contract on the host, per clip a function of its own noise and mel."""
    device = None
    encoder = None

    def generate_music_motion(self, mel, dim_pose, noise=None, smooth=None):
        mel = torch.as_tensor(mel)
        T = (mel.shape[1] - 1) // 3 + 1
        return (0.3 * noise[:, :T, :dim_pose] + mel[:, :T, :dim_pose] * 0.5).float().contiguous()


def _short_dataset(root, n, T):
    rng = np.random.default_rng(3)
    for i in range(n):
        d = os.path.join(root, f"clip{i:02d}")
        os.makedirs(d)
        np.save(os.path.join(d, "mel.npy"), rng.random((3 * T - 2, 128), dtype=np.float32))
        np.save(os.path.join(d, "motion.npy"), rng.standard_normal((T, 13, 2)).astype(np.float32))


def test_evaluate_dataset_without_the_new_arguments_is_unchanged(tmp_path):
    from diffusion_conductor_amd.evaluate import evaluate_dataset
    T = 24                                                  # shorter than the critic's 41 frames and Welch's 256
    _short_dataset(str(tmp_path), 5, T)
    plain = evaluate_dataset(_StubTrainer(), str(tmp_path), batch_size=2, seed=4, verbose=False)
    assert set(plain) == {"per_clip", "total_loss", "final_mse", "clips", "seconds", "frames_per_s", "main_thread_s"}
    with pytest.raises(ValueError, match="24 frames.*256"):
        evaluate_dataset(_StubTrainer(), str(tmp_path), batch_size=2, seed=4, verbose=False, rhythm=object())
    with pytest.raises(ValueError, match="24 frames.*41"):
        evaluate_dataset(_StubTrainer(), str(tmp_path), batch_size=2, seed=4, verbose=False, discriminator=object())


def test_evaluate_main_refuses_the_new_flags_beside_val_loss(capsys):
    from diffusion_conductor_amd import evaluate
    for flag in (["--rhythm"], ["--discriminator", "critic.pt"]):
        with pytest.raises(SystemExit) as e:
            evaluate.main(["--data_root", "nowhere", "--val_loss", *flag])
        assert e.value.code == 2 and "--val_loss" in capsys.readouterr().err


def test_strict_loading_and_shape_rules(weights):
    net = Discriminator_1DCNN("cuda:0")
    missing = dict(weights)
    del missing["fc.4.bias"]
    with pytest.raises(RuntimeError, match="missing keys.*fc.4.bias"):
        net.load_state_dict(missing, strict=True)
    extra = dict(weights)
    extra["module.fc.6.weight"] = np.zeros((1, 1), np.float32)
    with pytest.raises(RuntimeError, match="unexpected keys.*fc.6.weight"):
        net.load_state_dict(extra, strict=True)
    bad = dict(weights)
    bad["motion_encoder.0.weight"] = np.zeros((64, 25, 5), np.float32)
    with pytest.raises(RuntimeError, match="size mismatch for motion_encoder.0.weight"):
        net.load_state_dict(bad, strict=False)
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        net.forward(np.zeros((1, 41, 13, 2), np.float32))
    assert net.eval() is net and net.to("cuda:0") is net
    assert native.NativeDiscriminator.pooled_frames(1800) == (599, 298, 147) == H.pooled_frames(1800)
    assert native.NativeDiscriminator.pooled_frames(41)[2] == 1 and native.NativeDiscriminator.pooled_frames(40)[2] == 0
    assert native.NativeRhythm.windows(60) == native.NativeRhythm.windows(89) == 1 and native.NativeRhythm.windows(90) == 2


def test_rhythm_kernels_have_no_register_spills(tmp_path):
    """The kernels of csrc/dc_rhythm.hip fit their register budget without scratch."""
    import re
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(native.CSRC, "dc_rhythm.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value", src,
                          "-o", str(tmp_path / "dc_rhythm.s"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    spills, scratch, name = {}, {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"[VS]GPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = spills.get(name, 0) + int(m.group(1))
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    kernels = [k for k in spills if "k_psd" in k or "k_contour" in k or "k_sd" in k or "k_disc" in k]
    assert len(kernels) == 9, kernels          # psd cols + finish, contour, sd, two conv instances, head, mean, transpose
    assert all(spills[k] == 0 and scratch[k] == 0 for k in kernels), (spills, scratch)
