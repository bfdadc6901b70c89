"""The BiLSTM pose decoder on the MI355X (csrc/dc_bilstm.hip, generator.py) against the fp64 oracle of tests/helpers_bilstm.py.

The gate.  A case's unit is u = max(ref_vs_fp64, emul_vs_fp64) of tests/golden/g17_bilstm*.npz (tools/make_golden_bilstm.py): the
deviation of the reference's fp32 values and of the fp32 restatement in the kernels' order from the fp64 oracle, two independent
fp32 evaluations of the same recurrence, measured on the CPU, per case and per quantity (poses, LSTM output after layer 1, after
layer 2) - the error grows with T.  The GPU has to stay within 4 u of the oracle: a third summation order (the MFMA projections),
the device's exp and tanh, and the amplification along the recurrence that every fp32 evaluation shares.  For the full generator
the restatement follows the kernels in the features too (the split format of its music encoder), and the decoder's own unit is kept
beside that one.  Measured values:
DESIGN.md section 14 and profiles/bilstm_gpu_tests.txt; every test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_bilstm as L
from helpers import golden
from helpers_m2sgan import case_name, fixture_inputs

from diffusion_conductor_amd.generator import Generator, Generator_CVPR_LSTM, GeneratorBaseline, PoseDecoderBiLSTM
from diffusion_conductor_amd.native import DcError, NativeBiLSTM, NativeM2SGAN, bilstm_pass_clips, lib
from diffusion_conductor_amd.synthetic import synthetic_bilstm_state_dict, synthetic_m2sgan_bilstm_state_dict, synthetic_m2sgan_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GATE = 4.0
RING = 8                                         # kRing of csrc/dc_bilstm.hip
ALL_CASES = [(n, T) for n, ts in L.CASES.items() for T in ts]


@pytest.fixture(scope="module")
def weights():
    return {n: synthetic_bilstm_state_dict(0, n) for n in L.CASES}      # pinned by the fixture's digests (test_host_bilstm.py)


@pytest.fixture(scope="module")
def nets(weights):
    return {n: PoseDecoderBiLSTM(n, 26, DEV).load_state_dict(sd, strict=True) for n, sd in weights.items()}


def _gpu(net, x):
    """(poses, hidden after layer 1, after layer 2) of the device, as arrays."""
    xd = torch.from_numpy(x).to(DEV)
    out = net(xd), net.hidden(xd, 1), net.hidden(xd, 2)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("input_size,T", ALL_CASES, ids=[f"in{n}_T{T}" for n, T in ALL_CASES])
def test_parity_at_every_fixture_case(nets, weights, input_size, T):
    g, n = golden(L.FILES[input_size]), L.case_key(T)
    x = L.features(input_size, T)
    want = L.decoder_fp64(weights[input_size], x)
    got = _gpu(nets[input_size], x)
    unit = np.maximum(g[f"ref_vs_fp64_{n}"], g[f"emul_vs_fp64_{n}"])
    err = np.array([L.max_abs(a, b) for a, b in zip(got, want)])
    print(f"in={input_size} T={T}: gpu_vs_fp64 pose {err[0]:.3e} h1 {err[1]:.3e} h2 {err[2]:.3e}   unit {unit}   ratio {err / unit}")
    assert got[0].shape == (L.B, T, 26) and got[1].shape == got[2].shape == (L.B, T, 256)
    assert (err <= GATE * unit).all(), (err, unit)
    # ... and the reference's own fp32 poses are as far away as the two fp32 errors allow
    assert L.max_abs(got[0], g[f"pose_{n}"]) <= (GATE + 1) * unit[0]


@pytest.mark.parametrize("T", (RING - 1, RING, RING + 1))
def test_around_the_prefetch_rings_depth(nets, weights, T):
    """Lengths one short of the ring, equal to it and one past it: the unit comes from torch's own fp32 nn.LSTM and the restatement."""
    sd, x = weights[20], L.features(20, T)
    want = L.decoder_fp64(sd, x)
    lstm = torch.nn.LSTM(20, 128, num_layers=2, bidirectional=True, batch_first=True)
    lstm.load_state_dict({k[5:]: torch.from_numpy(v) for k, v in sd.items() if k.startswith("LSTM.")}, strict=True)
    with torch.no_grad():
        t32 = lstm(torch.from_numpy(x))[0].numpy()
    emul = L.decoder_fp32_emulated(sd, x)
    unit = np.array([L.max_abs(emul[0], want[0]), L.max_abs(emul[1], want[1]), max(L.max_abs(emul[2], want[2]), L.max_abs(t32, want[2]))])
    got = _gpu(nets[20], x)
    err = np.array([L.max_abs(a, b) for a, b in zip(got, want)])
    print(f"T={T}: gpu_vs_fp64 {err}   unit {unit}")
    assert (err <= GATE * unit).all(), (err, unit)


def test_bit_identical_in_any_batch(nets):
    """Clip 0 of a case alone, in the pair, in the reversed pair, and - at T = 2 - behind 129 other clips: in the second pass."""
    net = nets[128]
    for T in (2, 33, 150):
        x = torch.from_numpy(L.features(128, T)).to(DEV)
        alone, alone_h = net(x[:1]).clone(), net.hidden(x[:1], 2).clone()
        pair, rev = net(x), net(torch.flip(x, dims=[0]).contiguous())
        assert torch.equal(pair[0], alone[0]) and torch.equal(rev[1], alone[0]) and torch.equal(rev[0], pair[1]), T
        assert torch.equal(net.hidden(x, 2)[0], alone_h[0]) and torch.equal(net(x[:1]), alone), T
    B = 130
    assert bilstm_pass_clips(B, 2) == 128 < B
    many = torch.from_numpy(L.features(128, 2, batch=B, seed=23)).to(DEV)
    x = torch.from_numpy(L.features(128, 2)).to(DEV)
    many[B - 1], many[3] = x[0], x[0]
    out, hid = net(many), net.hidden(many, 1)
    assert torch.equal(out[B - 1], net(x[:1])[0]) and torch.equal(out[3], out[B - 1])
    assert torch.equal(hid[B - 1], net.hidden(x[:1], 1)[0])
    assert bool(torch.isfinite(out).all())


def _swapped(sd):
    """The two directions' weights exchanged, layer by layer."""
    out = {}
    for k, v in sd.items():
        if k.startswith("LSTM."):
            out[k[:-8] if k.endswith("_reverse") else k + "_reverse"] = v
        else:
            out[k] = v
    return {k: out[k] for k in sd}


@pytest.mark.parametrize("T", (1, 2, 33))
def test_direction_wiring(nets, weights, T):
    """The forward walk with the reverse direction's weights over the clip reversed in time is the reverse walk over the clip: with
    the two directions' weights exchanged on the host, the first layer's output of the time-reversed clip is the original output
    reversed in time with its two halves exchanged - bit for bit (at T = 1 there is nothing to reverse: the halves alone swap)."""
    sd = weights[20]
    other = PoseDecoderBiLSTM(20, 26, DEV).load_state_dict(_swapped(sd), strict=True)
    x = torch.from_numpy(L.features(20, T)).to(DEV)
    h = nets[20].hidden(x, 1)
    hs = other.hidden(torch.flip(x, dims=[1]).contiguous(), 1)
    want = torch.flip(torch.cat([h[..., 128:], h[..., :128]], dim=-1), dims=[1])
    assert torch.equal(hs, want)
    assert not torch.equal(h[..., :128], h[..., 128:])
    if T > 1:                                    # the walk's direction matters: without the reversal in time the outputs differ
        assert not torch.equal(other.hidden(x, 1), torch.cat([h[..., 128:], h[..., :128]], dim=-1))
    other.close()


def test_nan_stays_in_its_clip(nets):
    net = nets[128]
    x = torch.from_numpy(L.features(128, 33)).to(DEV)
    clean = net(x).clone()
    x[1, 20, 5] = float("nan")
    out = net(x)
    assert torch.equal(out[0], clean[0]) and bool(torch.isnan(out[1]).all())


@pytest.fixture(scope="module")
def generator():
    return Generator(DEV, decoder="bilstm").load_state_dict(synthetic_m2sgan_bilstm_state_dict(0), strict=True)


GEN_IDS = [case_name(T, Tm) for T, Tm in L.GENERATOR_CASES]


@pytest.mark.parametrize("T,Tm", L.GENERATOR_CASES, ids=GEN_IDS)
def test_full_generator_wiring_and_its_decoder(generator, weights, T, Tm):
    """`decode(features)` is `forward`, bit for bit; the features are the TCN generator's, bit for bit (the same encoder and noise
    branch weights); and the decoder, on the features the device made, is within the gate of the fp64 decoder on those features."""
    g, n = golden(L.FILES["gen"]), case_name(T, Tm)
    mel, z = fixture_inputs(T, Tm)
    pose = generator(mel, z)
    feat = generator.features(mel, z)
    assert tuple(pose.shape) == (L.B, T, 13, 2) and tuple(feat.shape) == (L.B, T, 128)
    assert torch.equal(generator.decode(feat), pose)
    # (the decoder's own unit: the reference's fp32 run and the decoder's fp32 restatement on fp32 features, no encoder format in it)
    unit = max(float(g[f"ref_vs_fp64_{n}"]), float(g[f"decoder_emul_vs_fp64_{n}"]))
    err = L.max_abs(pose.cpu().numpy().reshape(L.B, T, 26), L.decoder_fp64(weights[128], feat.cpu().numpy())[0])
    print(f"generator T={T}: decoder on the device's features, gpu_vs_fp64 {err:.3e}   unit {unit:.3e}")
    assert err <= GATE * unit, (err, unit)
    if T > 128:                                  # (the TCN generator needs T > 128)
        tcn = Generator(DEV).load_state_dict(synthetic_m2sgan_state_dict(0), strict=True)
        assert torch.equal(tcn.features(mel, z), feat)


@pytest.mark.parametrize("T,Tm", L.GENERATOR_CASES, ids=GEN_IDS)
def test_full_generator_forward_against_the_fixture(generator, T, Tm):
    """`forward`, end to end, against the fixture's fp64 poses (fp64 features through the fp64 decoder) with the gate of 4 u.  The
    unit's restatement follows the kernels in both halves: the decoder's fp32 order, and the split format of the music encoder the
    generator's handle pins (tools/make_golden_bilstm.py, split_format_encoder - the reference's own encoder with its operands held
    as hi + lo of two bf16 values), whose features sit 1.2e-5 .. 1.4e-5 from fp64 where plain fp32 sits 7e-7 .. 9e-7.  That format
    and not the decoder sets the size of this error: u = 7.4e-6 at T = 30 and 4.5e-5 at T = 150, against 4.3e-7 and 2.9e-6 for the
    decoder on fp32 features."""
    g, n = golden(L.FILES["gen"]), case_name(T, Tm)
    mel, z = fixture_inputs(T, Tm)
    pose = generator(mel, z).cpu().numpy().reshape(L.B, T, 26)
    unit = max(float(g[f"ref_vs_fp64_{n}"]), float(g[f"emul_vs_fp64_{n}"]))
    err = L.max_abs(pose, g[f"pose64_{n}"])
    print(f"generator T={T}: forward, gpu_vs_fp64 {err:.3e}   unit {unit:.3e}   vs the reference's fp32 {L.max_abs(pose, g[f'pose_{n}']):.3e}")
    assert err <= GATE * unit, (err, unit)


def test_cvpr_lstm_generator(weights):
    g = golden(L.FILES[20])
    net = Generator_CVPR_LSTM(DEV).load_state_dict({"lstm." + k: v for k, v in weights[20].items()}, strict=True)
    for T in (31, 150):
        x, n = L.features(20, T), L.case_key(T)
        y = net(x, None)
        assert tuple(y.shape) == (L.B, T, 13, 2) and torch.equal(y, net.forward(x))
        unit = max(g[f"ref_vs_fp64_{n}"][0], g[f"emul_vs_fp64_{n}"][0])
        err = L.max_abs(y.cpu().numpy().reshape(L.B, T, 26), L.decoder_fp64(weights[20], x)[0])
        print(f"CVPR_LSTM T={T}: gpu_vs_fp64 {err:.3e}  unit {unit:.3e}")
        assert err <= GATE * unit
        assert L.max_abs(y.cpu().numpy().reshape(L.B, T, 26), g[f"pose_{n}"]) <= (GATE + 1) * unit


def test_refusals_come_before_any_launch(weights):
    sd = weights[20]
    n = NativeBiLSTM(0)
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("LSTM.weight_ih_l2", np.zeros(512 * 256, np.float32))
    with pytest.raises(DcError, match="error -4.*elements"):
        n.set_param("LSTM.weight_hh_l0", np.zeros(512 * 127, np.float32))
    with pytest.raises(DcError, match="error -4.*elements"):
        n.set_param("LSTM.weight_ih_l0", np.zeros(512 * 129, np.float32))      # In = 129
    with pytest.raises(DcError, match="error -4.*elements"):
        n.set_param("LSTM.weight_ih_l0_reverse", np.zeros(500, np.float32))
    T = 5
    sentinel = 7.0
    feat, pose, hid = torch.zeros(1, T, 20, device=DEV), torch.full((1, T, 26), sentinel, device=DEV), torch.full((1, T, 256), sentinel, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lb, ptr = lib(), lambda t: t.data_ptr()
    assert Lb.dc_bilstm_decode(n._h, ptr(feat), 1, T, ptr(pose), stream) == -1          # before finalize: DC_ERR_INVALID
    assert Lb.dc_bilstm_hidden(n._h, ptr(feat), 1, T, 2, ptr(hid), stream) == -1
    assert n.input_size == 0
    last = "out.4.bias"
    for k, v in sd.items():
        if k != last:
            n.set_param(k, v)
    with pytest.raises(DcError, match="error -4.*out.4.bias"):
        n.finalize()
    n.set_param(last, sd[last])
    n.set_param("LSTM.weight_ih_l0_reverse", np.zeros(512 * 21, np.float32))            # fits no In of the forward direction
    with pytest.raises(DcError, match="error -4.*LSTM.weight_ih_l0_reverse"):
        n.finalize()
    assert Lb.dc_bilstm_decode(n._h, ptr(feat), 1, T, ptr(pose), stream) == -1
    n.set_param("LSTM.weight_ih_l0_reverse", sd["LSTM.weight_ih_l0_reverse"])
    n.finalize()
    assert n.input_size == 20
    for B, t in ((0, T), (1, 0), (-1, T)):
        assert Lb.dc_bilstm_decode(n._h, ptr(feat), B, t, ptr(pose), stream) == -1
        assert Lb.dc_bilstm_hidden(n._h, ptr(feat), B, t, 1, ptr(hid), stream) == -1
    for layers in (0, 3):
        assert Lb.dc_bilstm_hidden(n._h, ptr(feat), 1, T, layers, ptr(hid), stream) == -1
    assert Lb.dc_bilstm_decode(n._h, None, 1, T, ptr(pose), stream) == -1
    torch.cuda.synchronize()
    assert bool((pose == sentinel).all()) and bool((hid == sentinel).all())
    with pytest.raises(ValueError, match="loaded for 20"):
        n.decode(torch.zeros(1, T, 21, device=DEV))
    assert tuple(n.decode(feat).shape) == (1, T, 26)
    torch.cuda.synchronize()
    n.close()


def test_features_only_generator_and_the_default_one():
    gan, lstm = synthetic_m2sgan_state_dict(0), synthetic_m2sgan_bilstm_state_dict(0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    Lb, ptr = lib(), lambda t: t.data_ptr()
    n = NativeM2SGAN(0, decoder="none")
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("tcn.fc.0.weight", gan["tcn.fc.0.weight"])                          # a `tcn.*` entry given to one
    with pytest.raises(DcError, match="error -4.*unknown"):
        n.set_param("tcn.LSTM.weight_hh_l0", lstm["tcn.LSTM.weight_hh_l0"])
    for k, v in lstm.items():
        if not k.startswith("tcn."):
            n.set_param(k, v)
    n.finalize()
    T, Tm, Ln = 30, 88, 1
    mel, z = (torch.from_numpy(a).to(DEV) for a in fixture_inputs(T, Tm))
    feat = n.features(mel, z)                                                           # T <= 128: fine without temporal blocks
    assert tuple(feat.shape) == (2, T, 128) and bool(torch.isfinite(feat).all())
    sentinel = 7.0
    pose = torch.full((2, 150, 26), sentinel, device=DEV)
    big = torch.zeros(2, 150, 128, device=DEV)
    assert Lb.dc_m2sgan_decode(n._h, ptr(big), 2, 150, ptr(pose), stream) == -1
    assert Lb.dc_m2sgan_debug_blocks(n._h, ptr(big), 2, 150, 1, ptr(pose), stream) == -1
    assert Lb.dc_m2sgan_generate(n._h, ptr(mel), 2, Tm, ptr(z), Ln, ptr(pose), stream) == -1
    assert Lb.dc_m2sgan_set_decoder(n._h, 2) == -1
    torch.cuda.synchronize()
    assert bool((pose == sentinel).all())
    with pytest.raises(ValueError, match="features only"):
        n.decode(big)
    n.close()
    # `tcn.*` entries set first, the decoder taken away afterwards: finalize refuses them
    m = NativeM2SGAN(0)
    for k, v in gan.items():
        m.set_param(k, v)
    assert Lb.dc_m2sgan_set_decoder(m._h, 1) == 0
    with pytest.raises(DcError, match="error -4.*tcn\\."):
        m.finalize()
    # ... and a handle that never hears of set_decoder (or is told TCN) behaves as before: T <= 128 refused, poses as Generator's
    assert Lb.dc_m2sgan_set_decoder(m._h, 0) == 0
    m.finalize()
    assert Lb.dc_m2sgan_features(m._h, ptr(mel), 2, Tm, ptr(z), Ln, ptr(feat), stream) == -1
    mel2, z2 = (torch.from_numpy(a).to(DEV) for a in fixture_inputs(150, 450))
    plain = NativeM2SGAN(0)
    for k, v in gan.items():
        plain.set_param(k, v)
    plain.finalize()
    assert torch.equal(m.generate(mel2, z2), plain.generate(mel2, z2))
    torch.cuda.synchronize()
    m.close()
    plain.close()


def test_through_the_evaluator(generator, tmp_path):
    """evaluate_dataset on GeneratorBaseline(bilstm generator), 4 clips at T = 150: the poses are Generator.forward's on the clip's mel and
    clip_noise(seed, i)[:5, :8], the scores equal for batch sizes 1 and 2.  (The rhythm scores need clips of 256 frames or more -
    evaluate_dataset refuses them at 150 - so they get a run of their own at T = 270.)"""
    from diffusion_conductor_amd import evaluate as ev
    from diffusion_conductor_amd.metrics import standard_deviation_percentage
    from diffusion_conductor_amd.rhythm import MotionRhythm
    from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_motion
    made = []

    class Recording(GeneratorBaseline):
        def generate_music_motion(self, *a, **kw):
            made.append(super().generate_music_motion(*a, **kw).clone())
            return made[-1]
    base = Recording(generator)
    n, seed = 4, 6
    for T, rhythm in ((150, None), (270, MotionRhythm(DEV))):
        root = tmp_path / f"T{T}"
        mels = np.stack([smooth_mel(700 + i, 3 * T - 2, seed=7) for i in range(n)])
        gts = synthetic_motion(n, T, seed=24)
        for i in range(n):
            d = root / f"{i:03d}"
            d.mkdir(parents=True)
            np.save(d / "mel.npy", mels[i])
            np.save(d / "motion.npy", gts[i])
        runs = []
        for bs in (1, 2):
            del made[:]
            runs.append(ev.evaluate_dataset(base, str(root), 26, batch_size=bs, seed=seed, verbose=False, rhythm=rhythm))
            poses = torch.cat(made)
            assert tuple(poses.shape) == (n, T, 26)
            for i in range(n):
                z = ev.clip_noise(seed, i, T, 26)[:T // 30, :8].unsqueeze(0)
                assert torch.equal(poses[i], generator(mels[i:i + 1], z)[0].reshape(T, 26)), (T, bs, i)
        assert runs[0]["per_clip"] == runs[1]["per_clip"] and runs[0]["final_mse"] == runs[1]["final_mse"]
        if rhythm is not None:
            for k in ("rde", "sce", "sd_gen", "sd_real"):
                assert runs[0][k] == runs[1][k], k
            sdp = standard_deviation_percentage(runs[0]["sd_gen"], runs[0]["sd_real"])
            assert np.isfinite(sdp) and sdp > 0
    with pytest.raises(ValueError, match="sampling loop"):
        ev.evaluate_dataset(base, str(tmp_path / "T150"), 26, batch_size=2, seed=seed, verbose=False, steps=10)
