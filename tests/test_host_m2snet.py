"""M2SNet's host surface on a CPU-only box: the parameter spec and seeded weights (m2snet.py, synthetic.py), metrics.sync_stats, the
score's path through evaluate_dataset, and the fuse head's packing (csrc/dc_pack.h).  Known answers: tests/golden/g13_m2snet_sync.npz
(tools/make_golden_m2snet.py: the reference's M2SNet on seeded synthetic weights)."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from helpers import ROOT, golden
from helpers_m2snet import FIXTURE_TS, fixture_inputs, oracle_head
from test_motion_metrics_host import _FakeEncoder, _FakeTrainer, _dataset

from diffusion_conductor_amd import metrics, native
from diffusion_conductor_amd.m2snet import M2SNet, m2snet_shapes, strip_module_prefix
from diffusion_conductor_amd.motion_encoder import motion_encoder_shapes
from diffusion_conductor_amd.synthetic import (array_digest, synthetic_m2snet_state_dict, synthetic_motion_encoder_state_dict,
                                               synthetic_state_dict)


@pytest.fixture(scope="module")
def g13():
    return golden("g13_m2snet_sync.npz")


@pytest.fixture(scope="module")
def weights():
    return synthetic_m2snet_state_dict(0)


def test_param_spec_matches_reference_state_dict(g13, weights):
    spec = m2snet_shapes()
    assert len(spec) == 234
    assert list(spec) == [str(k) for k in g13["keys"]]
    assert [str(tuple(s)) for s in spec.values()] == [str(s) for s in g13["shapes"]]
    assert list(weights) == list(spec)
    assert all(tuple(np.shape(v)) == spec[k] for k, v in weights.items())
    assert np.array_equal(np.stack([array_digest(v) for v in weights.values()]), g13["weight_digest"])
    # assembled from the two existing seeded checkpoints
    den, mot = synthetic_state_dict(), synthetic_motion_encoder_state_dict()
    assert all(np.array_equal(weights[k], den[k]) for k in spec if k.startswith("music_encoder."))
    assert all(np.array_equal(weights["motion_encoder." + k], mot[k]) for k in motion_encoder_shapes())
    assert not any(k.startswith("proj.") for k in spec)


def test_fixture_inputs_regenerate_from_their_seeds(g13):
    assert tuple(g13["Ts"]) == FIXTURE_TS
    for T in FIXTURE_TS:
        mel, motion = fixture_inputs(T)
        assert mel.shape == (2, 3 * T - 2, 128) and motion.shape == (2, T, 13, 2)
        assert np.array_equal(array_digest(mel), g13[f"mel_digest_T{T}"]) and np.array_equal(array_digest(motion), g13[f"motion_digest_T{T}"])
        assert g13[f"prob_T{T}"].shape == (2, T, 1)
    lo, hi, pos = g13["logit_range"]           # what the seeded head is for: a threshold test that can fail
    assert lo <= -2 and hi >= 2 and 0.2 <= pos <= 0.8


def test_sync_stats_reproduces_reference_numbers(g13):
    st = metrics.sync_stats(g13["stats_matched"], g13["stats_mismatched"])
    assert isinstance(st["sync"], float) and isinstance(st["accuracy"], float)
    assert st["sync"] == float(g13["stats_sync"]) and st["non_sync"] == float(g13["stats_non_sync"])
    assert st["accuracy"] == float(g13["stats_accuracy"])
    # tensors and other shapes give the same numbers
    st2 = metrics.sync_stats(torch.from_numpy(g13["stats_matched"])[..., 0], torch.from_numpy(g13["stats_mismatched"]).reshape(-1))
    assert st2 == st
    # exactly 0.5 counts for neither side (M2SNet_eval.py:65-66: > 0.5 and < 0.5)
    m = np.array([[0.5, 0.75, 0.25, 1.0]], np.float32)
    n = np.array([[0.5, 0.5, 0.0, 0.875]], np.float32)
    st = metrics.sync_stats(m, n)
    assert st == {"sync": 0.625, "non_sync": 0.46875, "accuracy": 3 / 8}
    only = metrics.sync_stats(m)
    assert only["sync"] == 0.625 and math.isnan(only["non_sync"]) and only["accuracy"] == 0.5
    with pytest.raises(ValueError):
        metrics.sync_stats(np.zeros((0, 4), np.float32))


class _FakeM2SNet:
    """music_latent / motion_latent / fuse with canned per-frame predictions: elementwise, so nothing depends on the batch."""

    def music_latent(self, mel):
        mel = torch.as_tensor(mel)
        T = (mel.shape[1] - 1) // 3 + 1
        return mel[:, :3 * T:3, :64].contiguous()

    def motion_latent(self, x):
        return _FakeEncoder().latent(x)

    def fuse(self, mus, mot):
        return torch.sigmoid(4.0 * (mus * mot.transpose(1, 2)).sum(2))


def test_evaluate_dataset_adds_sync_scores_and_keeps_existing_keys(tmp_path):
    from diffusion_conductor_amd.evaluate import clip_noise, evaluate_dataset
    _dataset(str(tmp_path))
    timing = {"seconds", "frames_per_s", "main_thread_s", "steady_frames_per_s", "metrics_s"}
    new = {"m2s_sync_real", "m2s_sync_gen", "m2s_sync_mismatched", "m2s_accuracy_gen"}
    for kw in ({}, {"motion_encoder": _FakeEncoder(), "diversity_seed": 2}):
        base = evaluate_dataset(_FakeTrainer(), str(tmp_path), batch_size=2, seed=4, verbose=False, **kw)
        r = evaluate_dataset(_FakeTrainer(), str(tmp_path), batch_size=2, seed=4, verbose=False, m2snet=_FakeM2SNet(), **kw)
        assert set(r) == set(base) | new
        for k in set(base) - timing:
            assert r[k] == base[k], k
    # the scores are sync_stats on the model's predictions for the same poses: 5 clips in batches of 2, 2, 1 (no control for the last)
    fake, tr, ids = _FakeM2SNet(), _FakeTrainer(), sorted(r["per_clip"])
    real, gen, mis = [], [], []
    for lo in (0, 2, 4):
        idx = list(range(lo, min(lo + 2, 5)))
        mel = np.stack([np.load(os.path.join(str(tmp_path), ids[i], "mel.npy")) for i in idx])
        gt = torch.from_numpy(np.stack([np.load(os.path.join(str(tmp_path), ids[i], "motion.npy")) for i in idx]))
        pred = tr.generate_music_motion(mel, 26, noise=torch.stack([clip_noise(4, i, 24, 26) for i in idx]))
        mus, gl = fake.music_latent(mel), fake.motion_latent(pred.reshape(len(idx), 24, 13, 2))
        real.append(fake.fuse(mus, fake.motion_latent(gt)))
        gen.append(fake.fuse(mus, gl))
        if len(idx) > 1:
            mis.append(fake.fuse(mus, gl.roll(-1, 0)))
    st = metrics.sync_stats(torch.cat(gen), torch.cat(mis))
    assert r["m2s_sync_gen"] == st["sync"] and r["m2s_sync_mismatched"] == st["non_sync"] and r["m2s_accuracy_gen"] == st["accuracy"]
    assert r["m2s_sync_real"] == metrics.sync_stats(torch.cat(real))["sync"]
    assert 0 < r["m2s_accuracy_gen"] < 1
    one = evaluate_dataset(_FakeTrainer(), str(tmp_path), batch_size=1, seed=4, verbose=False, m2snet=_FakeM2SNet())
    assert math.isnan(one["m2s_sync_mismatched"]) and one["m2s_sync_real"] == pytest.approx(r["m2s_sync_real"], rel=1e-6)


def test_strict_loading_matches_the_motion_encoder(weights):
    ckpt = {"module." + k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}
    stripped = strip_module_prefix(ckpt)
    assert list(stripped) == list(weights)
    net = M2SNet("cuda:0")
    missing = dict(stripped)
    del missing["fuse_layer.4.bias"]
    with pytest.raises(RuntimeError, match="missing keys.*fuse_layer.4.bias"):
        net.load_state_dict(missing, strict=True)
    extra = dict(stripped)
    extra["proj.weight"] = torch.zeros(64, 64)
    with pytest.raises(RuntimeError, match="unexpected keys.*proj.weight"):
        net.load_state_dict(extra, strict=True)
    bad = dict(stripped)
    bad["fuse_layer.0.weight"] = torch.zeros(64, 127, 1)
    with pytest.raises(RuntimeError, match="size mismatch for fuse_layer.0.weight"):
        net.load_state_dict(bad, strict=False)
    with pytest.raises(NotImplementedError):
        net.features(torch.zeros(1, 4, 128), torch.zeros(1, 2, 13, 2))
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        net.forward(torch.zeros(1, 4, 128), torch.zeros(1, 2, 13, 2))
    assert net.eval() is net and net.to("cuda:0") is net


def test_head_packing_against_a_numpy_restatement(weights, tmp_path):
    """m2s_head_pack (csrc/dc_pack.h): every fragment element is the weight the MFMA operand layout asks for, and a k-ordered fp64
    evaluation THROUGH the image equals the fp64 head of helpers_m2snet."""
    cxx = shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"      # (dc_pack.h converts through _Float16: clang, the ROCm host compiler)
    if not os.path.exists(cxx):
        pytest.skip("no clang++")
    exe, fin, fout = str(tmp_path / "probe"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", native.CSRC, os.path.join(ROOT, "tests", "m2snet_pack_probe.cpp"), "-o", exe], check=True)
    names = [f"fuse_layer.{i}.{s}" for i in (0, 2, 4) for s in ("weight", "bias")]
    np.concatenate([weights[n].ravel() for n in names]).astype(np.float32).tofile(fin)
    offs = [int(v) for v in subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True).stdout.split()]
    w0o, b0o, w1o, b1o, w2o, b2o, total = offs
    img = np.fromfile(fout, np.float32)
    assert img.size == total
    lane = np.arange(64)

    def frags(W, nmt, ks):           # [mt][ks][lane] = W[32 mt + (lane & 31)][2 ks + (lane >> 5)], rows past n_out zero
        Wp = np.zeros((32 * nmt, W.shape[1]), np.float32)
        Wp[:W.shape[0]] = W
        return np.stack([np.stack([Wp[32 * mt + (lane & 31), 2 * k + (lane >> 5)] for k in range(ks)]) for mt in range(nmt)])
    W0, W1, W2 = (weights[f"fuse_layer.{i}.weight"][:, :, 0] for i in (0, 2, 4))
    assert np.array_equal(img[w0o:b0o].reshape(2, 64, 64), frags(W0, 2, 64))
    assert np.array_equal(img[w1o:b1o].reshape(2, 32, 64), frags(W1, 2, 32))
    assert np.array_equal(img[w2o:b2o].reshape(1, 32, 64), frags(W2, 1, 32))
    assert np.array_equal(img[b0o:b0o + 64], weights["fuse_layer.0.bias"]) and np.array_equal(img[b1o:b1o + 64], weights["fuse_layer.2.bias"])
    assert img[b2o] == weights["fuse_layer.4.bias"][0] and not img[b2o + 1:].any()

    # the head evaluated from the image alone, in fp64: row o of tile mt at k = 2 ks + h is fragment element lane = (o & 31) + 32 h
    def unpack(o, nmt, ks):
        f = img[o:o + nmt * ks * 64].astype(np.float64).reshape(nmt, ks, 2, 32)          # [mt][ks][h][row]
        return f.transpose(0, 3, 1, 2).reshape(nmt * 32, 2 * ks)
    rng = np.random.default_rng(5)
    mus, mot = rng.standard_normal((2, 7, 64)), rng.standard_normal((2, 64, 7))
    z = np.concatenate([mus, mot.transpose(0, 2, 1)], axis=2)
    h1 = np.maximum(z @ unpack(w0o, 2, 64).T + img[b0o:b0o + 64], 0)
    h2 = np.maximum(h1 @ unpack(w1o, 2, 32).T + img[b1o:b1o + 64], 0)
    logit = (h2 @ unpack(w2o, 1, 32).T)[..., 0] + img[b2o]
    ref, _ = oracle_head(weights, mus, mot)
    assert np.abs(logit - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())


def test_head_kernel_has_no_register_spills_and_no_lds(tmp_path):
    """k_m2s_head (csrc/dc_m2snet.hip) fits its register budget without scratch and uses no LDS."""
    import re
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(ROOT, "diffusion-conductor_amd", "csrc", "dc_m2snet.hip")
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value", src,
                          "-o", str(tmp_path / "dc_m2snet.s"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    vals, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"([VS]GPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            vals.setdefault(name, {})[m.group(1)] = int(m.group(2))
    kernels = [k for k in vals if "k_m2s_head" in k]
    assert len(kernels) == 1, list(vals)
    assert all(v == 0 for v in vals[kernels[0]].values()), vals
    asm = open(tmp_path / "dc_m2snet.s").read()
    assert asm.count("v_mfma_f32_32x32x2") >= 128 + 64 + 32 - 3 * 16      # (the motion half of layer 0 is a loop unrolled by 8)
