"""The M2S-GAN generator on the MI355X (csrc/dc_m2sgan.hip, generator.py) against the reference's fp32 poses and features of
tests/golden/g15_m2sgan*.npz (tools/make_golden_m2sgan.py) and the fp64 oracle of tests/helpers_m2sgan.py.

Bounds.  Each is four times the largest error measured on the MI355X over the cases it covers, rounded up to one significant
digit ("M2S-GAN generator"); the bound against the reference's fp32 fixture is that bound plus the
fixture's `ref_vs_fp64` (5.7e-7 for the poses, 1.5e-6 for the features):
  poses, end to end, against fp64                 measured 8.04e-7   bound 4e-6
  poses against the reference's fp32              measured 8.94e-7   bound 4e-6 + ref_vs_fp64
  features, end to end, against fp64              measured 1.67e-5   bound 7e-5   (the split-format music encoder's half)
  features[..., 64:], the noise branch's half     measured 1.50e-6   bound 6e-6
  poses of `decode` alone on fp32 features        measured 5.91e-7   bound 3e-6   (fp32 summation, K = 320 / 640, twelve convolutions deep)
  residual stream after n = 1 .. 6 blocks         measured 2.66e-6   bound 2e-5   (absolute, on values up to 12)
The first and last 65 frames of a clip (the reflected region of dilation 32 plus the pool's end frames) are held to the same
bounds as the rest; the maxima are printed per region.
tests/test_gpu_m2sgan_edges.py holds the decoder alone at the lengths that are no multiple of the pool kernel's 30-frame tile
(129 ... 181, 961) to DECODE_TOL and BLOCK_TOL, imported from here: measured there 5.61e-7 and 2.80e-6.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import golden
from helpers_m2sgan import (FIXTURE_CASES, case_name, fixture_inputs, load_fixture, oracle_blocks, oracle_decode, oracle_features,
                            oracle_head, temporal_block)

from diffusion_conductor_amd.generator import Generator, GeneratorBaseline
from diffusion_conductor_amd.m2snet import M2SNet
from diffusion_conductor_amd.native import DcError, NativeM2SGAN, lib
from diffusion_conductor_amd.synthetic import synthetic_m2sgan_state_dict, synthetic_m2snet_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POSE_TOL, FEAT_TOL, NOISE_FEAT_TOL, DECODE_TOL, BLOCK_TOL = 4e-6, 7e-5, 6e-6, 3e-6, 2e-5
EDGE = 65
IDS = [case_name(T, Tm) for T, Tm in FIXTURE_CASES]


@pytest.fixture(scope="module")
def g15():
    return load_fixture(golden)


@pytest.fixture(scope="module")
def weights():
    return synthetic_m2sgan_state_dict(0)            # pinned by the fixture's digests (test_host_m2sgan.py)


@pytest.fixture(scope="module")
def net(weights):
    return Generator(DEV).load_state_dict(weights, strict=True)


@pytest.fixture(scope="module")
def oracle(weights):
    """(T, Tm) -> (mel, latent, fp64 features, fp32 features, fp64 residual streams after 1 .. 6 blocks of the fp32 features, fp64
    poses of the fp64 features, fp64 poses of the fp32 features), computed once."""
    cache = {}

    def get(T, Tm):
        if (T, Tm) not in cache:
            mel, z = fixture_inputs(T, Tm)
            f64 = oracle_features(weights, mel, z)
            f32 = f64.astype(np.float32)
            streams = [oracle_blocks(weights, f32, 1)]
            for i in range(1, 6):
                streams.append(temporal_block(weights, i, streams[-1]))
            cache[(T, Tm)] = (mel, z, f64, f32, streams, oracle_decode(weights, f64), oracle_head(weights, streams[-1]))
        return cache[(T, Tm)]
    return get


def _regions(err):
    """max of err [B, T, C] over the first EDGE frames, the last EDGE frames and the frames between."""
    T = err.shape[1]
    mid = err[:, EDGE:T - EDGE]
    return float(err[:, :EDGE].max()), float(mid.max()) if mid.size else 0.0, float(err[:, T - EDGE:].max())


@pytest.mark.parametrize("T,Tm", FIXTURE_CASES, ids=IDS)
def test_parity_at_every_fixture_case(net, g15, oracle, T, Tm):
    mel, z, f64, _, _, p64, _ = oracle(T, Tm)
    n = case_name(T, Tm)
    pose = net(mel, z)
    assert tuple(pose.shape) == (2, T, 13, 2) and pose.dtype == torch.float32
    pose = pose.cpu().numpy().reshape(2, T, 26).astype(np.float64)
    feat = net.features(mel, z).cpu().numpy().astype(np.float64)
    assert feat.shape == (2, T, 128)
    ep, ef = np.abs(pose - p64), np.abs(feat - f64)
    ep_ref = float(np.abs(pose - g15[f"pose_{n}"].reshape(2, T, 26)).max())
    ef_ref = float(np.abs(feat - g15[f"features_{n}"]).max())
    print(f"M2S-GAN {n}: |pose - fp64| first/mid/last {_regions(ep)}  |pose - reference| {ep_ref:.2e}  |features - fp64| music "
          f"{ef[..., :64].max():.2e} noise {ef[..., 64:].max():.2e} first/mid/last {_regions(ef)}  |features - reference| {ef_ref:.2e}")
    assert max(_regions(ep)) <= POSE_TOL and max(_regions(ef)) <= FEAT_TOL, (n, _regions(ep), _regions(ef))
    assert max(_regions(ef[..., 64:])) <= NOISE_FEAT_TOL, (n, _regions(ef[..., 64:]))      # the noise branch's half: the new kernels' own bound
    assert ep_ref <= POSE_TOL + float(g15["ref_vs_fp64"]) and ef_ref <= FEAT_TOL + float(g15["ref_vs_fp64_features"]), (n, ep_ref, ef_ref)


@pytest.mark.parametrize("T,Tm", FIXTURE_CASES, ids=IDS)
def test_music_half_of_the_features_is_m2snets_latent(net, weights, T, Tm):
    """features[..., :64] is bit-identical to M2SNet.music_latent of an M2SNet with the same `music_encoder.*` weights: the same
    kernels in the same pinned format."""
    sd = synthetic_m2snet_state_dict(0)
    sd.update({k: v for k, v in weights.items() if k.startswith("music_encoder.")})
    m2s = M2SNet(DEV).load_state_dict(sd, strict=True)
    mel, z = fixture_inputs(T, Tm)
    assert torch.equal(net.features(mel, z)[..., :64], m2s.music_latent(mel))


@pytest.mark.parametrize("T,Tm", FIXTURE_CASES, ids=IDS)
def test_decoder_alone_block_by_block(net, oracle, T, Tm):
    """decode and debug_blocks(n) on the oracle's fp32 features against the fp64 decoder on the same fp32 values: the new kernels
    without the encoder; a wrong dilation, tap order or reflection shows in its block."""
    _, _, _, f32, streams, _, p64 = oracle(T, Tm)
    feat = torch.from_numpy(f32).to(DEV)
    for nblk in range(1, 7):
        h = net.debug_blocks(feat, nblk)
        assert tuple(h.shape) == (2, T, 64)
        e = np.abs(h.cpu().numpy().astype(np.float64) - streams[nblk - 1])
        print(f"M2S-GAN {case_name(T, Tm)} after block {nblk}: |h - fp64| first/mid/last {_regions(e)}  max |h| {streams[nblk - 1].max():.2f}")
        assert max(_regions(e)) <= BLOCK_TOL, (T, nblk, _regions(e))
    pose = net.decode(feat)
    assert tuple(pose.shape) == (2, T, 13, 2)
    e = np.abs(pose.cpu().numpy().reshape(2, T, 26).astype(np.float64) - p64)
    print(f"M2S-GAN {case_name(T, Tm)} decode alone: |pose - fp64| first/mid/last {_regions(e)}")
    assert max(_regions(e)) <= DECODE_TOL, (T, _regions(e))
    # forward is features followed by decode
    mel, z = oracle(T, Tm)[:2]
    assert torch.equal(net.decode(net.features(mel, z)), net(mel, z))


def test_bit_identical_in_any_batch_and_on_a_rerun(net):
    (mel, z), (mel2, z2) = fixture_inputs(150, 449), fixture_inputs(150, 449, B=5)
    mel, z, mel2, z2 = (torch.from_numpy(a).to(DEV) for a in (mel, z, mel2, z2))
    alone, alone_f = net(mel[:1], z[:1]).clone(), net.features(mel[:1], z[:1]).clone()
    pair = net(mel, z).clone()
    assert torch.equal(pair[0], alone[0])
    assert torch.equal(net(mel.flip(0), z.flip(0))[1], alone[0])
    assert torch.equal(net(mel2, z2)[0], alone[0]) and torch.equal(net.features(mel2, z2)[0], alone_f[0])
    assert torch.equal(net(mel2, z2)[1], pair[1])
    assert torch.equal(net(mel, z), pair) and torch.equal(net.features(mel[:1], z[:1]), alone_f)
    big_m, big_z = mel2[:1].expand(34, -1, -1).clone(), z2[:1].expand(34, -1, -1).clone()      # past the 32-clip chunk of a pass
    big_m[33], big_z[33] = mel[1], z[1]
    assert torch.equal(net(big_m, big_z)[33], pair[1]) and torch.equal(net(big_m, big_z)[0], alone[0])


def test_refusals_come_before_any_launch(weights):
    n = NativeM2SGAN(0)
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("tcn.TCN.tcn.tcn.network.0.net.3.weight", np.zeros(64, np.float32))
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("proj.weight", np.zeros(64 * 64, np.float32))
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("tcn.TCN.tcn.tcn.network.1.downsample.weight", np.zeros(64 * 64, np.float32))
    with pytest.raises(DcError, match="error -4.*elements"):
        n.set_param("tcn.TCN.tcn.tcn.network.0.conv1.weight_v", np.zeros(64 * 64 * 5, np.float32))
    with pytest.raises(DcError, match="error -4.*elements"):
        n.set_param("tcn.TCN.tcn.tcn.network.2.net.5.weight_g", np.zeros(63, np.float32))
    T, Tm, Ln = 150, 448, 5
    mel, z = torch.zeros(1, Tm, 128, device=DEV), torch.zeros(1, Ln, 8, device=DEV)
    sentinel = 7.0
    pose, feat = torch.full((1, T, 26), sentinel, device=DEV), torch.full((1, T, 128), sentinel, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L, ptr = lib(), lambda t: t.data_ptr()
    # every entry point before finalize: DC_ERR_INVALID
    assert L.dc_m2sgan_generate(n._h, ptr(mel), 1, Tm, ptr(z), Ln, ptr(pose), stream) == -1
    assert L.dc_m2sgan_features(n._h, ptr(mel), 1, Tm, ptr(z), Ln, ptr(feat), stream) == -1
    assert L.dc_m2sgan_decode(n._h, ptr(feat), 1, T, ptr(pose), stream) == -1
    assert L.dc_m2sgan_debug_blocks(n._h, ptr(feat), 1, T, 1, ptr(pose), stream) == -1
    with pytest.raises(DcError, match="error -1.*finalize"):
        n.generate(mel, z)
    last = "noise_BN.running_var"
    for k, v in weights.items():             # aliases and counters included: accepted
        if k != last:
            n.set_param(k, v)
    with pytest.raises(DcError, match="error -4.*noise_BN.running_var"):
        n.finalize()
    assert L.dc_m2sgan_generate(n._h, ptr(mel), 1, Tm, ptr(z), Ln, ptr(pose), stream) == -1
    n.set_param(last, weights[last])
    n.finalize()
    # T = 120 (Ln = 4), T != 30 Ln, T != (Tm - 1) / 3 + 1 (decode has no Tm: T <= 128), Tm < 4, B < 1, NULL
    for B, tm, ln in ((1, 358, 4), (1, Tm, 4), (1, Tm, 6), (1, 3, 5), (0, Tm, Ln)):
        assert L.dc_m2sgan_generate(n._h, ptr(mel), B, tm, ptr(z), ln, ptr(pose), stream) == -1, (B, tm, ln)
        assert L.dc_m2sgan_features(n._h, ptr(mel), B, tm, ptr(z), ln, ptr(feat), stream) == -1, (B, tm, ln)
    assert L.dc_m2sgan_generate(n._h, ptr(mel), 1, Tm, None, Ln, ptr(pose), stream) == -1
    for B, t in ((1, 120), (1, 128), (0, T)):
        assert L.dc_m2sgan_decode(n._h, ptr(feat), B, t, ptr(pose), stream) == -1
        assert L.dc_m2sgan_debug_blocks(n._h, ptr(feat), B, t, 1, ptr(pose), stream) == -1
    assert L.dc_m2sgan_debug_blocks(n._h, ptr(feat), 1, T, 7, ptr(pose), stream) == -1
    torch.cuda.synchronize()
    assert bool((pose == sentinel).all()) and bool((feat == sentinel).all())
    # ... and each as a ValueError of the Python surface
    for m, lat in ((torch.zeros(1, 358, 128, device=DEV), torch.zeros(1, 4, 8, device=DEV)), (mel, torch.zeros(1, 4, 8, device=DEV)),
                   (torch.zeros(1, 3, 128, device=DEV), z)):
        with pytest.raises(ValueError):
            n.generate(m, lat)
    with pytest.raises(ValueError):
        n.decode(torch.zeros(1, 120, 128, device=DEV))
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        Generator(DEV).forward(mel, z)
    assert tuple(n.generate(mel, z).shape) == (1, T, 26)
    torch.cuda.synchronize()
    n.close()


def test_encoder_format_is_pinned(net, monkeypatch):
    mel, z = fixture_inputs(150, 450)
    monkeypatch.delenv("DC_ME_PREC", raising=False)
    ref = net(mel, z).clone()
    monkeypatch.setenv("DC_ME_PREC", "f16")
    assert torch.equal(net(mel, z), ref)


def test_through_the_evaluator(net, tmp_path):
    """evaluate_dataset on GeneratorBaseline with the real motion encoder and M2SNet: per-clip scores bit-identical for batch sizes 1
    and 2, the poses those of Generator.forward on the clip's mel and clip_noise(seed, i)[:5, :8]."""
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN
    from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_motion, synthetic_motion_encoder_state_dict
    T, n, seed = 150, 3, 6
    mels = np.stack([smooth_mel(500 + i, 3 * T - 2, seed=7) for i in range(n)])
    gts = synthetic_motion(n, T, seed=22)
    for i in range(n):
        d = tmp_path / f"{i:03d}"
        d.mkdir()
        np.save(d / "mel.npy", mels[i])
        np.save(d / "motion.npy", gts[i])
    menc = MotionEncoder_STGCN(DEV).load_state_dict(synthetic_motion_encoder_state_dict())
    m2s = M2SNet(DEV).load_state_dict(synthetic_m2snet_state_dict(0), strict=True)
    made = []

    class Recording(GeneratorBaseline):
        def generate_music_motion(self, *a, **kw):
            made.append(super().generate_music_motion(*a, **kw).clone())
            return made[-1]
    base = Recording(net)
    runs = []
    for bs in (1, 2):
        del made[:]
        runs.append(ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=bs, seed=seed, verbose=False, motion_encoder=menc, m2snet=m2s))
        poses = torch.cat(made)                  # the batches in clip order
        assert tuple(poses.shape) == (n, T, 26)
        for i in range(n):
            z = ev.clip_noise(seed, i, T, 26)[:5, :8].unsqueeze(0)
            assert torch.equal(poses[i], net(mels[i:i + 1], z)[0].reshape(T, 26)), (bs, i)
    assert runs[0]["per_clip"] == runs[1]["per_clip"] and runs[0]["latent_mse"] == runs[1]["latent_mse"]
    for k in ("final_mse", "final_latent_mse", "fgd", "feat_dist", "diversity", "m2s_sync_real", "m2s_sync_gen"):
        assert runs[0][k] == runs[1][k], k
    for i, cid in enumerate(sorted(runs[0]["per_clip"])):
        assert runs[0]["per_clip"][cid] == float(ev.mse_loss(gts[i], poses[i].cpu().numpy().reshape(T, 13, 2)))
    with pytest.raises(ValueError, match="sampling loop"):
        ev.evaluate_dataset(base, str(tmp_path), 26, batch_size=2, seed=seed, verbose=False, guidance_scale=2.0)


def test_evaluate_main_scores_a_generator_checkpoint(weights, tmp_path, capsys):
    """--baseline_generator: a checkpoint file with DataParallel keys through evaluate.main with --metrics, --sync and --smooth: one
    JSON line, "model": "m2sgan", the evaluation's own keys beside it."""
    import json
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_motion
    T, n = 150, 3
    data = tmp_path / "data"
    for i in range(n):
        d = data / f"{i:03d}"
        d.mkdir(parents=True)
        np.save(d / "mel.npy", smooth_mel(600 + i, 3 * T - 2, seed=7))
        np.save(d / "motion.npy", synthetic_motion(1, T, seed=23, first=i)[0])
    ckpt = str(tmp_path / "generator.pt")
    torch.save({"module." + k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}, ckpt)
    assert ev.main(["--data_root", str(data), "--baseline_generator", ckpt, "--batch_size", "2", "--seed", "6", "--metrics", "--sync", "--smooth"]) == 0
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["model"] == "m2sgan" and r["clips"] == n and len(r["per_clip"]) == n
    assert {"final_mse", "final_latent_mse", "fgd", "feat_dist", "diversity", "m2s_sync_gen", "m2s_accuracy_gen"} <= set(r)
    assert all(np.isfinite(v) and v > 0 for v in r["per_clip"].values())
