"""The BiLSTM pose decoder's host surface on a CPU-only box: the parameter specs and seeded weights (generator.py, synthetic.py), the
fp64 oracle and the fp32 restatement of tests/helpers_bilstm.py against the reference's fp32 values, the loader's choice of decoder,
load_state_dict's errors, the SDP and the CLI's help.  Known answers: tests/golden/g17_bilstm*.npz (tools/make_golden_bilstm.py: the
reference's PoseDecoderBiLSTM, Generator_CVPR_LSTM and CNN-LSTM Generator on seeded synthetic weights)."""
import numpy as np
import pytest
import torch

import helpers_bilstm as L
from helpers import golden

from diffusion_conductor_amd import native
from diffusion_conductor_amd.generator import (Generator, Generator_CVPR_LSTM, GeneratorBaseline, PoseDecoderBiLSTM, bilstm_shapes,
                                               m2sgan_bilstm_shapes, m2sgan_decoder_of, m2sgan_shapes)
from diffusion_conductor_amd.metrics import standard_deviation_percentage
from diffusion_conductor_amd.synthetic import synthetic_bilstm_state_dict, synthetic_m2sgan_bilstm_state_dict, synthetic_m2sgan_state_dict


@pytest.fixture(scope="module")
def weights():
    return {n: synthetic_bilstm_state_dict(0, n) for n in L.CASES}


@pytest.mark.parametrize("input_size", sorted(L.CASES))
def test_param_spec_matches_reference_state_dict(weights, input_size):
    g, spec, sd = golden(L.FILES[input_size]), bilstm_shapes(input_size), weights[input_size]
    assert len(spec) == 22
    assert list(spec) == [str(k) for k in g["keys"]] == list(sd)
    assert [str(tuple(s)) for s in spec.values()] == [str(s) for s in g["shapes"]]
    assert all(tuple(np.shape(v)) == spec[k] and v.dtype == np.float32 for k, v in sd.items())
    assert L.digest(sd) == int(g["weight_digest"])
    assert tuple(int(t) for t in g["lengths"]) == L.CASES[input_size]


def test_generator_specs_match_reference_state_dicts(weights):
    g, spec, sd = golden(L.FILES["gen"]), m2sgan_bilstm_shapes(), synthetic_m2sgan_bilstm_state_dict(0)
    assert list(spec) == [str(k) for k in g["keys"]] == list(sd)
    assert [str(tuple(s)) for s in spec.values()] == [str(s) for s in g["shapes"]]
    assert L.digest(sd) == int(g["weight_digest"])
    assert [tuple(int(v) for v in c) for c in g["cases"]] == list(L.GENERATOR_CASES)
    # the generator cases' units: the full restatement (split-format encoder + fp32 decoder) and, beside it, the decoder's alone
    from helpers_m2sgan import case_name
    for T, Tm in L.GENERATOR_CASES:
        n = case_name(T, Tm)
        ref, full, dec = (float(g[f"{k}_{n}"]) for k in ("ref_vs_fp64", "emul_vs_fp64", "decoder_emul_vs_fp64"))
        assert 0 < ref < 1e-5 and 0 < dec < 1e-5 and dec < full < 1e-4, (n, ref, full, dec)
        assert g[f"pose_{n}"].shape == g[f"pose64_{n}"].shape == (L.B, T, 26) and g[f"pose64_{n}"].dtype == np.float64
        assert L.max_abs(g[f"pose_{n}"], g[f"pose64_{n}"]) == ref
    # the encoder and the noise branch are the TCN generator's, tensor for tensor; the decoder is the In = 128 one under `tcn.`
    tcn = synthetic_m2sgan_state_dict(0)
    shared = [k for k in spec if not k.startswith("tcn.")]
    assert shared == [k for k in m2sgan_shapes() if not k.startswith("tcn.")] and all(np.array_equal(sd[k], tcn[k]) for k in shared)
    assert all(np.array_equal(sd["tcn." + k], v) for k, v in weights[128].items())
    assert [str(k) for k in golden(L.FILES[20])["cvpr_keys"]] == ["lstm." + k for k in bilstm_shapes(20)]
    for bad in (0, 129):
        with pytest.raises(ValueError, match="1 .. 128"):
            bilstm_shapes(bad)


# (input size, T): the T = 900 and 1800 cases are restated by the fixture's tool only (minutes of numpy)
RESTATED = [(n, T) for n, ts in L.CASES.items() for T in ts if T <= 33] + [(20, 150)]


@pytest.mark.parametrize("input_size,T", RESTATED)
def test_oracle_and_restatement_reproduce_the_fixture(weights, input_size, T):
    """The fixture's units: the reference's fp32 values and the fp32 restatement, each against the fp64 oracle."""
    g, gh, sd, n = golden(L.FILES[input_size]), golden(L.HIDDEN_FILES[input_size]), weights[input_size], L.case_key(T)
    x = L.features(input_size, T)
    p64, a64, b64 = L.decoder_fp64(sd, x)
    ref = np.array([L.max_abs(g[f"pose_{n}"], p64), L.max_abs(gh[f"hidden1_{n}"], a64), L.max_abs(gh[f"hidden2_{n}"], b64)])
    pe, ae, be = L.decoder_fp32_emulated(sd, x)
    emul = np.array([L.max_abs(pe, p64), L.max_abs(ae, a64), L.max_abs(be, b64)])
    print(f"In={input_size} T={T}: ref_vs_fp64 {ref}  emul_vs_fp64 {emul}")
    # (the oracle's fp64 sums may differ in the last bits between BLAS builds: 1e-12 absolute on deviations of 1e-8 .. 1e-5)
    assert np.allclose(ref, g[f"ref_vs_fp64_{n}"], rtol=0, atol=1e-12) and np.allclose(emul, g[f"emul_vs_fp64_{n}"], rtol=0, atol=1e-12)
    assert (g[f"ref_vs_fp64_{n}"] < 1e-5).all() and (g[f"emul_vs_fp64_{n}"] < 1e-5).all()


def test_every_case_has_units_and_long_clips_stay_small():
    for input_size, lengths in L.CASES.items():
        g = golden(L.FILES[input_size])
        for T in lengths:
            r, e = g[f"ref_vs_fp64_{L.case_key(T)}"], g[f"emul_vs_fp64_{L.case_key(T)}"]
            assert r.shape == e.shape == (3,) and (r > 0).all() and (e > 0).all()
            assert max(r.max(), e.max()) < 1e-3, (input_size, T, r, e)
            assert g[f"pose_{L.case_key(T)}"].shape == (L.B, T, 26)


def test_oracle_matches_torch_fp64_lstm(weights):
    sd, x = weights[20], L.features(20, 31)
    lstm = torch.nn.LSTM(20, 128, num_layers=2, bidirectional=True, batch_first=True).double()
    lstm.load_state_dict({k[5:]: torch.from_numpy(v).double() for k, v in sd.items() if k.startswith("LSTM.")}, strict=True)
    with torch.no_grad():
        want = lstm(torch.from_numpy(x).double())[0].numpy()
    assert L.max_abs(L.lstm_fp64(sd, x), want) < 1e-12


def test_loader_picks_the_decoder_from_the_keys():
    assert m2sgan_decoder_of(m2sgan_bilstm_shapes()) == "bilstm"
    assert m2sgan_decoder_of(m2sgan_shapes()) == "tcn"
    assert Generator().decoder == "tcn" and Generator(decoder="bilstm").decoder == "bilstm"
    with pytest.raises(ValueError, match="decoder"):
        Generator(decoder="gru")
    with pytest.raises(ValueError, match="decoder"):
        native.NativeM2SGAN(0, decoder="gru")


def test_load_state_dict_errors(weights):
    sd = dict(weights[20])
    dec = PoseDecoderBiLSTM(20, 26)
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        dec.forward(np.zeros((1, 3, 20), np.float32))
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        dec.hidden(np.zeros((1, 3, 20), np.float32))
    missing = {k: v for k, v in sd.items() if k != "LSTM.bias_hh_l1_reverse"}
    with pytest.raises(RuntimeError, match=r"missing keys \['LSTM.bias_hh_l1_reverse'\]"):
        dec.load_state_dict(missing, strict=True)
    with pytest.raises(RuntimeError, match=r"unexpected keys \['LSTM.weight_ih_l2'\]"):
        dec.load_state_dict({**sd, "LSTM.weight_ih_l2": sd["LSTM.weight_ih_l1"]}, strict=True)
    with pytest.raises(RuntimeError, match=r"size mismatch for LSTM.weight_ih_l0: got \(512, 128\), expected \(512, 20\)"):
        dec.load_state_dict({**sd, "LSTM.weight_ih_l0": weights[128]["LSTM.weight_ih_l0"]}, strict=True)
    with pytest.raises(ValueError, match="26 values"):
        PoseDecoderBiLSTM(20, 20)
    cv = Generator_CVPR_LSTM()
    with pytest.raises(RuntimeError, match="missing keys"):
        cv.load_state_dict(sd, strict=True)                    # (the keys lack the `lstm.` prefix)
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        cv.forward(np.zeros((1, 3, 20), np.float32))
    # a CNN-LSTM checkpoint in a TCN generator, and the other way round
    with pytest.raises(RuntimeError, match="unexpected keys"):
        Generator().load_state_dict(synthetic_m2sgan_bilstm_state_dict(0), strict=True)
    with pytest.raises(RuntimeError, match="unexpected keys"):
        Generator(decoder="bilstm").load_state_dict(synthetic_m2sgan_state_dict(0), strict=True)
    with pytest.raises(RuntimeError, match="load_state_dict first"):
        Generator(decoder="bilstm").forward(np.zeros((1, 88, 128), np.float32), np.zeros((1, 1, 8), np.float32))


def test_baseline_refuses_loop_options_on_a_bilstm_generator():
    base = GeneratorBaseline(Generator(decoder="bilstm"))
    mel = np.zeros((1, 88, 128), np.float32)
    for kw in ({"steps": 10}, {"guidance_scale": 2.0}, {"solver": "dpmpp2m"}, {"takes": 2}):
        with pytest.raises(ValueError, match="one forward pass"):
            base.generate_music_motion(mel, **kw)


def test_frame_rules_follow_the_decoder():
    chk = native.NativeM2SGAN.check_frames
    with pytest.raises(ValueError, match="T > 128"):
        chk(30, 88, 1)
    chk(30, 88, 1, decoder="none")                             # no temporal block bounds a features-only generator
    with pytest.raises(ValueError, match="latent"):
        chk(30, 88, 2, decoder="none")


def test_standard_deviation_percentage():
    assert standard_deviation_percentage(0.05, 0.1) == pytest.approx(50.0)
    # the competition's form: the ratio of the MEANS over the clips, not the mean of the ratios
    assert standard_deviation_percentage([0.1, 0.3], torch.tensor([0.2, 0.2])) == pytest.approx(100.0)
    assert standard_deviation_percentage(np.float32(0.3), np.float32(0.2)) == pytest.approx(150.0, rel=1e-6)
    with pytest.raises(ValueError, match="not positive"):
        standard_deviation_percentage(0.1, 0.0)
    with pytest.raises(ValueError):
        standard_deviation_percentage([], [0.1])


def test_cli_help_names_both_flavours(capsys):
    from diffusion_conductor_amd import evaluate
    with pytest.raises(SystemExit):
        evaluate.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "tcn.TCN.*" in text and "tcn.LSTM.*" in text and "BiLSTM" in text      # (argparse may wrap a line at a hyphen)


def test_pass_size_formula():
    """clips per pass = min(B, 128, 2^28 // (1536 T)), at least 1: the workspace of 1536 floats per frame stays within 1 GiB."""
    f = native.bilstm_pass_clips
    assert f(2, 30) == 2 and f(130, 2) == 128 and f(500, 900) == 128
    assert f(500, 1800) == (1 << 28) // (1536 * 1800) == 97
    assert f(500, 1365) == 128 and f(500, 1366) == 127       # 2^28 / (1536 * 128) = 1365.33
    assert f(4, 1 << 20) == 1 and f(0, 5) == 0 and f(5, 0) == 0
    for T in (1, 1800, 5000, 100000):
        assert f(128, T) * T * 1536 <= (1 << 28)
