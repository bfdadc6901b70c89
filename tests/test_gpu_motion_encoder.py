"""The ST-GCN motion encoder's HIP kernels (csrc/dc_stgcn.hip) and the latent-space scores on the MI355X, against the known
answers of tests/golden/g12_motion_metrics.npz (the reference's MotionEncoder_STGCN / Evaluator, tools/make_golden_stgcn.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import golden, make_model

from diffusion_conductor_amd import metrics
from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN
from diffusion_conductor_amd.native import DcError, NativeMotionEncoder, lib
from diffusion_conductor_amd.synthetic import synthetic_generated_motion, synthetic_motion, synthetic_motion_encoder_state_dict

pytestmark = pytest.mark.gpu
TS = (1, 2, 3, 17, 90, 1800)


@pytest.fixture(scope="module")
def g12():
    return golden("g12_motion_metrics.npz")


@pytest.fixture(scope="module")
def weights():
    return synthetic_motion_encoder_state_dict()        # pinned by the fixture's digests (test_motion_metrics_host.py)


def _motions(g12, T):
    return synthetic_motion(2, T, seed=int(g12["motion_seed"]), first=100 * T)


def _pairs(g12):
    real = synthetic_motion(g12["real_latent"].shape[0], g12["real_latent"].shape[2], seed=int(g12["pair_seed"]))
    return real, synthetic_generated_motion(real, seed=int(g12["gen_seed"]))


@pytest.fixture(scope="module")
def enc(weights):
    return MotionEncoder_STGCN("cuda:0").load_state_dict(weights, strict=True)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def test_latents_match_reference_at_every_length(enc, g12):
    for T in TS:
        lat = enc.latent(torch.from_numpy(_motions(g12, T))).cpu().numpy()
        assert lat.shape == (2, 64, T)
        if T == 1800:            # the fixture keeps three 32-frame windows of the long clips
            lat = lat[:, :, g12["latent_T1800_frames"]]
        ref = g12[f"latent_T{T}"]
        errs = [_rel(lat[i], ref[i]) for i in range(2)]
        assert max(errs) <= 1e-5, (T, errs)
    fwd = enc.forward(torch.from_numpy(_motions(g12, 17)).reshape(2, 17, 26)).cpu().numpy()
    assert fwd.shape == (2, 17, 64) and _rel(fwd.transpose(0, 2, 1), g12["latent_T17"]) <= 1e-5


def test_clip_latent_is_bit_identical_in_any_batch(enc, g12):
    m = torch.from_numpy(np.concatenate(_pairs(g12)))      # 12 clips of 90 frames
    alone = enc.latent(m[3:4]).cpu()
    batch = enc.latent(m[:7]).cpu()
    rev = enc.latent(m.flip(0)).cpu()
    assert torch.equal(batch[3], alone[0])
    assert torch.equal(rev[m.shape[0] - 1 - 3], alone[0])
    assert torch.equal(rev.flip(0)[:7], batch)


def test_scores_from_hip_latents_match_reference(enc, g12):
    real_m, gen_m = _pairs(g12)
    real = list(enc.latent(torch.from_numpy(real_m)).cpu().numpy())
    gen = list(enc.latent(torch.from_numpy(gen_m)).cpu().numpy())
    fgd, feat_dist = metrics.frechet_gesture_distance(gen, real)
    assert abs(fgd - g12["fgd"]) <= 1e-4 * abs(g12["fgd"]), (fgd, g12["fgd"])
    assert abs(feat_dist - g12["feat_dist"]) <= 1e-5 * abs(g12["feat_dist"])
    for s, ref in zip(g12["div_seeds"], g12["diversity"]):
        d = metrics.diversity_score(gen, int(s))
        assert abs(d - ref) <= 1e-5 * abs(ref), (s, d, ref)
    se = metrics.sync_error([metrics.latent_mse(a, b) for a, b in zip(gen, real)])
    assert abs(se - g12["se"]) <= 1e-5 * abs(g12["se"]), (se, g12["se"])


def test_error_paths(weights):
    e = NativeMotionEncoder(0)
    with pytest.raises(DcError, match="error -4.*unknown"):
        e.set_param("st_gcn.not_a_parameter", np.zeros(3, np.float32))
    with pytest.raises(DcError, match="error -4.*elements"):
        e.set_param("fc.0.bias", np.zeros(63, np.float32))
    x = torch.zeros(1, 4, 13, 2, device="cuda:0")
    with pytest.raises(DcError, match="error -1.*finalize"):
        e.encode(x)
    for k, v in weights.items():
        if k != "st_gcn.edge_importance.7":
            e.set_param(k, v)
    with pytest.raises(DcError, match="error -4.*edge_importance.7"):
        e.finalize()
    e.set_param("st_gcn.edge_importance.7", weights["st_gcn.edge_importance.7"])
    e.finalize()
    out = torch.empty(1, 64, 4, device="cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for B, T in ((0, 4), (1, 0), (-1, 4)):
        assert lib().dc_motion_encoder_encode(e._h, x.data_ptr(), B, T, out.data_ptr(), stream) == -1
    assert e.encode(x).shape == (1, 64, 4)
    torch.cuda.synchronize()
    e.close()


def test_evaluate_dataset_scores_equal_recomputed(enc, tmp_path):
    """evaluate_dataset with the real sampler and encoder: the latent scores are metrics.py's on latent() of the poses
    generate_music_motion returns for the same mel and noise, and of the ground truth."""
    import types
    from diffusion_conductor_amd import DDPMTrainer
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.synthetic import batch_mel, synthetic_motion
    T, n = 40, 5
    mels = batch_mel(n, 3 * T - 2)
    gts = synthetic_motion(n, T, seed=21)
    for i in range(n):
        d = tmp_path / f"{i:03d}"
        d.mkdir()
        np.save(d / "mel.npy", mels[i])
        np.save(d / "motion.npy", gts[i])
    opt = types.SimpleNamespace(device=torch.device("cuda:0"), diffusion_steps=25, is_train=False)
    tr = DDPMTrainer(opt, make_model("fp16"))
    tr.eval_mode()
    r = ev.evaluate_dataset(tr, str(tmp_path), 26, batch_size=3, seed=5, verbose=False, motion_encoder=enc, diversity_seed=1)
    gen, real = [], []
    for lo in (0, 3):                  # the driver's batches
        idx = range(lo, min(lo + 3, n))
        noise = torch.stack([ev.clip_noise(5, i, T, 26) for i in idx]).cuda()
        pred = tr.generate_music_motion(torch.from_numpy(mels[lo:lo + len(idx)]), 26, noise=noise)
        gen += list(enc.latent(pred).cpu().numpy())
        real += list(enc.latent(torch.from_numpy(gts[lo:lo + len(idx)])).cpu().numpy())
    per = [metrics.latent_mse(a, b) for a, b in zip(gen, real)]
    fgd, fd = metrics.frechet_gesture_distance(gen, real)
    ids = [f"{i:03d}" for i in range(n)]
    assert [r["latent_mse"][c] for c in ids] == [float(v) for v in per]
    assert r["final_latent_mse"] == float(metrics.sync_error(per))
    assert r["fgd"] == float(fgd) and r["feat_dist"] == float(fd)
    assert r["diversity"] == float(metrics.diversity_score(gen, 1))
    print(f"latent scores: SE {r['final_latent_mse']:.4g} FGD {r['fgd']:.4g} feat_dist {r['feat_dist']:.4g} "
          f"diversity {r['diversity']:.4g} ({r['metrics_s'] * 1e3:.1f} ms on the host)")
