"""M2SNet on the MI355X (csrc/dc_m2snet.hip, m2snet.py) against the reference's fp32 probabilities of tests/golden/g13_m2snet_sync.npz
(tools/make_golden_m2snet.py) and the fp64 oracle of tests/helpers_m2snet.py.

Bounds.  Each is four times the largest error measured on the MI355X over the cases it covers, rounded up to one significant
digit ("M2SNet"):
  logit, end to end, against fp64         measured 1.06e-4   bound 5e-4   (the split-format music encoder's 6e-6 through the seeded
                                                                           head's gain, |d logit / d z| = 19.5: `fuse` alone is 18 times closer)
  probability, end to end, against fp64   measured 2.60e-5   bound 2e-4
  probability against the reference fp32  measured 2.61e-5   bound 2e-4   (the reference itself is 2.3e-6 from fp64)
  logit of `fuse` alone on fp32 latents   measured 5.86e-6   bound 3e-5   (fp32 summation through the same gain)
  probability of `fuse` alone             measured 1.46e-6   bound 6e-6
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import golden, make_model
from helpers_m2snet import FIXTURE_TS, fixture_inputs, oracle_head, oracle_latents

from diffusion_conductor_amd.m2snet import M2SNet
from diffusion_conductor_amd.native import DcError, NativeM2SNet, lib
from diffusion_conductor_amd.synthetic import batch_mel, synthetic_m2snet_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOGIT_TOL, PROB_TOL, PROB_REF_TOL = 5e-4, 2e-4, 2e-4
FUSE_LOGIT_TOL, FUSE_PROB_TOL = 3e-5, 6e-6


@pytest.fixture(scope="module")
def g13():
    return golden("g13_m2snet_sync.npz")


@pytest.fixture(scope="module")
def weights():
    return synthetic_m2snet_state_dict(0)            # pinned by the fixture's digests (test_host_m2snet.py)


@pytest.fixture(scope="module")
def net(weights):
    return M2SNet(DEV).load_state_dict(weights, strict=True)


@pytest.fixture(scope="module")
def oracle(weights):
    """(T, Tm) -> (mel, motion, fp64 music latent, fp64 motion latent, fp64 logit, fp64 probability), computed once."""
    cache = {}

    def get(T, Tm=None):
        key = (T, Tm or 3 * T - 2)
        if key not in cache:
            mel, motion = fixture_inputs(T, Tm)
            mus, mot = oracle_latents(weights, mel, motion)
            cache[key] = (mel, motion, mus, mot) + oracle_head(weights, mus, mot)
        return cache[key]
    return get


def _fp32_latents(oracle, T=65):
    """The oracle's latents of the two T = 65 fixture clips rounded to fp32 (what `fuse` is fed), on the host."""
    _, _, mus, mot, _, _ = oracle(65)
    return mus[:, :T].float().contiguous(), mot[:, :, :T].float().contiguous()


@pytest.mark.parametrize("T", FIXTURE_TS)
def test_parity_at_every_fixture_length(net, g13, oracle, T):
    mel, motion, _, _, logit64, prob64 = oracle(T)
    prob = net(mel, motion).cpu().numpy()
    assert prob.shape == (2, T, 1) and prob.dtype == np.float32
    logit = net.logits(mel, motion).cpu().numpy()
    assert logit.shape == (2, T)
    e_ref = float(np.abs(prob.astype(np.float64) - g13[f"prob_T{T}"]).max())
    e_logit = float(np.abs(logit - logit64).max())
    e_prob = float(np.abs(prob[..., 0] - prob64).max())
    print(f"M2SNet T={T}: |p - reference| {e_ref:.2e}  |logit - fp64| {e_logit:.2e}  |p - fp64| {e_prob:.2e}")
    assert e_ref <= PROB_REF_TOL and e_logit <= LOGIT_TOL and e_prob <= PROB_TOL, (T, e_ref, e_logit, e_prob)


@pytest.mark.parametrize("Tm", (97, 98, 99))
def test_other_mel_lengths_give_the_same_frames(net, oracle, Tm):
    mel, motion, _, _, logit64, prob64 = oracle(33, Tm)
    prob = net(mel, motion).cpu().numpy()
    logit = net.logits(mel, motion).cpu().numpy()
    assert prob.shape == (2, 33, 1)
    e_logit, e_prob = float(np.abs(logit - logit64).max()), float(np.abs(prob[..., 0] - prob64).max())
    print(f"M2SNet T=33 Tm={Tm}: |logit - fp64| {e_logit:.2e}  |p - fp64| {e_prob:.2e}")
    assert e_logit <= LOGIT_TOL and e_prob <= PROB_TOL, (Tm, e_logit, e_prob)


@pytest.mark.parametrize("T", (1, 31, 32, 33, 65))
def test_fuse_alone_is_at_fp32_summation_level(net, weights, oracle, T):
    """The head on latents it is handed (the oracle's, as fp32) against the fp64 head on the same fp32 values: the new kernel alone."""
    mus, mot = _fp32_latents(oracle, T)
    logit64, prob64 = oracle_head(weights, mus, mot)
    prob, logit = net.fuse(mus, mot, return_logits=True)
    assert tuple(prob.shape) == (2, T) and tuple(logit.shape) == (2, T)
    assert torch.equal(net.fuse(mus, mot), prob)                 # without the logit output: the same probabilities
    e_logit = float(np.abs(logit.cpu().numpy() - logit64).max())
    e_prob = float(np.abs(prob.cpu().numpy() - prob64).max())
    print(f"M2SNet fuse T={T}: |logit - fp64| {e_logit:.2e}  |p - fp64| {e_prob:.2e}")
    assert e_logit <= FUSE_LOGIT_TOL and e_prob <= FUSE_PROB_TOL, (T, e_logit, e_prob)


def test_threshold_agrees_with_the_oracle(net, oracle):
    """p > 0.5 is the oracle's logit > 0 on every frame whose fp64 |logit| exceeds the logit bound; at most 1 % of the frames are
    that close to the threshold (the seeded head spreads the logits over [-2.5, 2.6])."""
    n = close = 0
    for T in FIXTURE_TS:
        mel, motion, _, _, logit64, _ = oracle(T)
        prob = net(mel, motion).cpu().numpy()[..., 0]
        far = np.abs(logit64) > LOGIT_TOL
        assert np.array_equal(prob[far] > 0.5, logit64[far] > 0), T
        n, close = n + far.size, close + int((~far).sum())
    print(f"M2SNet threshold: {close} of {n} frames within {LOGIT_TOL} of the threshold")
    assert close <= 0.01 * n, (close, n)


def test_fuse_is_bit_identical_in_any_batch(net, oracle):
    mus, mot = _fp32_latents(oracle)
    mus, mot = mus.to(DEV), mot.to(DEV)
    alone = [t.clone() for t in net.fuse(mus[:1], mot[:1], return_logits=True)]
    g = torch.Generator().manual_seed(3)
    for B, positions in ((3, (0, 1, 2)), (65, (0, 63, 64))):      # 65: past the 64-clip chunk of the score's passes
        M = torch.randn((B, 65, 64), generator=g).to(DEV)
        Y = torch.randn((B, 64, 65), generator=g).to(DEV)
        for pos in positions:
            m, y = M.clone(), Y.clone()
            m[pos], y[pos] = mus[0], mot[0]
            prob, logit = net.fuse(m, y, return_logits=True)
            assert torch.equal(prob[pos], alone[0][0]) and torch.equal(logit[pos], alone[1][0]), (B, pos)


def test_score_is_bit_identical_in_any_batch(net, oracle):
    mel, motion = (torch.from_numpy(a) for a in oracle(33)[:2])
    alone = net.logits(mel[:1], motion[:1]).clone()
    p_alone = net(mel[:1], motion[:1]).clone()
    others = torch.from_numpy(batch_mel(1, 97, seed=9))
    g = torch.Generator().manual_seed(4)
    for B, positions in ((3, (0, 1, 2)), (65, (0, 63, 64))):
        for pos in positions:
            m = others.expand(B, -1, -1).clone()
            x = 0.5 * torch.randn((B, 33, 13, 2), generator=g)
            m[pos], x[pos] = mel[0], motion[0]
            assert torch.equal(net.logits(m, x)[pos], alone[0]), (B, pos)
            assert torch.equal(net(m, x)[pos], p_alone[0]), (B, pos)


def test_nan_in_a_motion_latent_frame_stays_in_that_frame(net, oracle):
    mus, mot = _fp32_latents(oracle)
    clean = net.fuse(mus, mot, return_logits=True)
    bad = mot.clone()
    bad[1, 17, 40] = float("nan")                     # one channel of one frame of clip 1
    prob, logit = net.fuse(mus, bad, return_logits=True)
    hit = torch.zeros(2, 65, dtype=torch.bool)
    hit[1, 40] = True
    for got, ref in ((prob.cpu(), clean[0].cpu()), (logit.cpu(), clean[1].cpu())):
        assert torch.equal(torch.isnan(got), hit)
        assert torch.equal(got[~hit], ref[~hit])


def test_nan_pose_frame_reaches_ten_frames_each_way(net, oracle):
    mel, motion = (torch.from_numpy(a) for a in oracle(65)[:2])
    clean = net.logits(mel, motion).cpu()
    p_clean = net(mel, motion).cpu()
    bad = motion.clone()
    bad[0, 30] = float("nan")
    logit, prob = net.logits(mel, bad).cpu(), net(mel, bad).cpu()[..., 0]
    hit = torch.zeros(2, 65, dtype=torch.bool)
    hit[0, 20:41] = True                               # the ST-GCN's ten temporal convolutions: t - 10 .. t + 10
    assert torch.equal(torch.isnan(logit), hit) and torch.equal(torch.isnan(prob), hit)
    assert torch.equal(logit[~hit], clean[~hit]) and torch.equal(prob[~hit], p_clean[..., 0][~hit])


def test_error_paths(weights):
    n = NativeM2SNet(0)
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("fuse_layer.1.weight", np.zeros(3, np.float32))
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("proj.weight", np.zeros(64 * 64, np.float32))
    with pytest.raises(DcError, match="error -4.*elements"):
        n.set_param("fuse_layer.0.weight", np.zeros(64 * 127, np.float32))
    with pytest.raises(DcError, match="error -4.*elements"):
        n.set_param("music_encoder.conv4.0.bias", np.zeros(63, np.float32))
    mel = torch.zeros(1, 10, 128, device=DEV)
    motion = torch.zeros(1, 4, 13, 2, device=DEV)
    sentinel = 7.0
    out = torch.full((1, 4), sentinel, device=DEV)
    lat_m, lat_y = torch.zeros(1, 4, 64, device=DEV), torch.zeros(1, 64, 4, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L, ptr = lib(), lambda t: t.data_ptr()
    # every entry point before finalize: DC_ERR_INVALID
    assert L.dc_m2snet_score(n._h, ptr(mel), ptr(motion), 1, 10, 4, ptr(out), None, stream) == -1
    assert L.dc_m2snet_fuse(n._h, ptr(lat_m), ptr(lat_y), 1, 4, ptr(out), None, stream) == -1
    assert L.dc_m2snet_encode_music(n._h, ptr(mel), 1, 10, ptr(lat_m), stream) == -1
    with pytest.raises(DcError, match="error -1.*finalize"):
        n.score(mel, motion)
    for k, v in weights.items():
        if k != "fuse_layer.4.bias":
            n.set_param(k, v)
    with pytest.raises(DcError, match="error -4.*fuse_layer.4.bias"):
        n.finalize()
    assert L.dc_m2snet_score(n._h, ptr(mel), ptr(motion), 1, 10, 4, ptr(out), None, stream) == -1
    n.set_param("fuse_layer.4.bias", weights["fuse_layer.4.bias"])
    n.finalize()
    # T != (Tm - 1) / 3 + 1, Tm < 4, B < 1: DC_ERR_INVALID, nothing written
    for B, Tm, T in ((1, 10, 3), (1, 10, 5), (1, 3, 1), (1, 0, 1), (0, 10, 4)):
        assert L.dc_m2snet_score(n._h, ptr(mel), ptr(motion), B, Tm, T, ptr(out), None, stream) == -1, (B, Tm, T)
    assert L.dc_m2snet_encode_music(n._h, ptr(mel), 1, 3, ptr(lat_m), stream) == -1
    assert L.dc_m2snet_fuse(n._h, ptr(lat_m), ptr(lat_y), 1, 0, ptr(out), None, stream) == -1
    torch.cuda.synchronize()
    assert bool((out == sentinel).all())
    with pytest.raises(DcError, match="error -1.*latent frames"):
        n.score(mel, torch.zeros(1, 5, 13, 2, device=DEV))
    assert tuple(n.score(mel, motion).shape) == (1, 4)
    torch.cuda.synchronize()
    n.close()


def test_both_motion_layouts_give_the_same_bits(net, oracle):
    mel, motion = oracle(17)[:2]
    a = net(mel, motion)
    b = net(mel, motion.reshape(2, 17, 26))
    assert torch.equal(a, b)
    assert torch.equal(net.logits(mel, torch.from_numpy(motion)), net.logits(torch.from_numpy(mel).to(DEV), motion.reshape(2, 17, 26)))
    with pytest.raises(ValueError, match="motion must be"):
        net(mel, motion.reshape(2, 17, 2, 13))
    # the split entry points compose to forward
    lat = net.fuse(net.music_latent(mel), net.motion_latent(motion))
    assert torch.equal(lat.unsqueeze(2), a)


def test_sampler_music_encoder_is_untouched(weights):
    """A dc_sampler holding the diffusion checkpoint's encoder gives the same encode_music bits before and after an M2SNet (with
    other `music_encoder.*` weights) is created, used and destroyed in the same process."""
    m = make_model("fp16")
    mel = torch.from_numpy(batch_mel(2, 97)).to(DEV)
    before = [t.clone() for t in m.encode_music(mel, DEV)]
    other = {k: (np.ascontiguousarray(v[::-1]) if k.startswith("music_encoder.") and k.endswith("conv2d_layer.0.weight") else v)
             for k, v in weights.items()}                    # output channels of every 3x3 conv reversed: another encoder
    n = M2SNet(DEV).load_state_dict(other, strict=True)
    motion = fixture_inputs(33)[1]
    p = n(mel, motion)
    assert bool(torch.isfinite(p).all())
    mid = [t.clone() for t in m.encode_music(mel, DEV)]
    n._native.close()
    del n
    torch.cuda.synchronize()
    after = m.encode_music(mel, DEV)
    for a, b, c in zip(before, mid, after):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_evaluate_dataset_sync_scores_equal_recomputed(net, tmp_path):
    """evaluate_dataset with the real sampler and the real M2SNet: the m2s_* scores are sync_stats on fuse() of the music latent with the
    latents of the ground truth, of the poses generate_music_motion returns for the same mel and noise, and of those poses rolled by one."""
    import types
    from diffusion_conductor_amd import DDPMTrainer, metrics
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.synthetic import synthetic_motion
    T, n = 40, 5
    mels = batch_mel(n, 3 * T - 2)
    gts = synthetic_motion(n, T, seed=21)
    for i in range(n):
        d = tmp_path / f"{i:03d}"
        d.mkdir()
        np.save(d / "mel.npy", mels[i])
        np.save(d / "motion.npy", gts[i])
    opt = types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=25, is_train=False)
    tr = DDPMTrainer(opt, make_model("fp16"))
    tr.eval_mode()
    base = ev.evaluate_dataset(tr, str(tmp_path), 26, batch_size=3, seed=5, verbose=False)
    r = ev.evaluate_dataset(tr, str(tmp_path), 26, batch_size=3, seed=5, verbose=False, m2snet=net)
    assert r["per_clip"] == base["per_clip"] and r["final_mse"] == base["final_mse"]
    real, gen, mis = [], [], []
    for lo in (0, 3):                  # the driver's batches
        idx = range(lo, min(lo + 3, n))
        noise = torch.stack([ev.clip_noise(5, i, T, 26) for i in idx]).cuda()
        pred = tr.generate_music_motion(torch.from_numpy(mels[lo:lo + len(idx)]), 26, noise=noise)
        mus = net.music_latent(mels[lo:lo + len(idx)])
        gl = net.motion_latent(pred)
        real.append(net.fuse(mus, net.motion_latent(gts[lo:lo + len(idx)])).cpu())
        gen.append(net.fuse(mus, gl).cpu())
        mis.append(net.fuse(mus, gl.roll(-1, 0)).cpu())
        assert torch.equal(gen[-1].unsqueeze(2), net(mels[lo:lo + len(idx)], pred).cpu())
    st = metrics.sync_stats(torch.cat(gen), torch.cat(mis))
    assert (r["m2s_sync_gen"], r["m2s_sync_mismatched"], r["m2s_accuracy_gen"]) == (st["sync"], st["non_sync"], st["accuracy"])
    assert r["m2s_sync_real"] == metrics.sync_stats(torch.cat(real))["sync"]
    print(f"sync scores: real {r['m2s_sync_real']:.4f} generated {r['m2s_sync_gen']:.4f} mismatched {r['m2s_sync_mismatched']:.4f} "
          f"accuracy {r['m2s_accuracy_gen']:.4f}")


def test_encoder_format_is_pinned(net, oracle, monkeypatch):
    """The score's music encoder runs the split format whatever DC_ME_PREC tells the sampler's encoder."""
    mel, motion = oracle(33)[:2]
    monkeypatch.delenv("DC_ME_PREC", raising=False)
    ref = net.logits(mel, motion).clone()
    monkeypatch.setenv("DC_ME_PREC", "f16")
    assert torch.equal(net.logits(mel, motion), ref)
    monkeypatch.setenv("DC_ME_PREC", "split")
    assert torch.equal(net.logits(mel, motion), ref)
