"""The mel front end on the MI355X (csrc/dc_mel.hip, mel.MelSpectrogram) against the fp64 oracle of tests/helpers_mel.py.

The bound of the accuracy tests is not a constant: for each input it is 8 x the worst error of the fp32 numpy restatement
(mel.mel_features_host / mel_power_host, dtype float32 - the reference's own precision) against the same oracle on that input,
computed here on the CPU, with a floor of 2^-20.  The factor covers an FFT whose summation order differs from pocketfft's, the
hardware logarithm's last bit and the rounding of v[i] (1 - w) + v[i + 1] w.  Unit: the output's [0, 1] scale for `features`, the
clip's maximum power for `power`."""
import ctypes as C
import wave

import numpy as np
import pytest
import torch

import helpers_mel as H
from helpers import make_model, state_dict_np
from helpers_rhythm import value_class

from diffusion_conductor_amd import mel as M
from diffusion_conductor_amd import native

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
LENGTHS = (2048, 2303, 2304, 22050, 44100)
_handles = {}


def spec(pad_mode="constant", sr=22050):
    if (pad_mode, sr) not in _handles:
        _handles[(pad_mode, sr)] = M.MelSpectrogram("cuda:0", sr, pad_mode)
    return _handles[(pad_mode, sr)]


def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint32)


def check_against_oracle(name, n, pad_mode, power, feats):
    """power [F, 128], feats [Tm, 128] of signal(name, n) from the GPU -> the two ratios error / yardstick (asserted <= 8)."""
    y = H.signal(name, n)
    op, of = H.oracle(name, n, pad_mode, "power"), H.oracle(name, n, pad_mode, "features")
    assert power.shape == op.shape == (1 + n // 256, 128) and feats.shape == of.shape == (H.out_frames(n), 128)
    yard_p = np.abs(M.mel_power_host(y, pad_mode=pad_mode).astype(np.float64) - op).max() / op.max()
    yard_f = np.abs(M.mel_features_host(y, pad_mode=pad_mode).astype(np.float64) - of).max()
    err_p = np.abs(power.astype(np.float64) - op).max() / op.max()
    err_f = np.abs(feats.astype(np.float64) - of).max()
    bound_p, bound_f = max(8.0 * yard_p, FLOOR), max(8.0 * yard_f, FLOOR)
    print(f"mel {name} n={n} {pad_mode}: power err {err_p:.3e} yardstick {yard_p:.3e} bound {bound_p:.3e} | features err {err_f:.3e} "
          f"yardstick {yard_f:.3e} bound {bound_f:.3e} | ratios {err_p / yard_p:.2f} {err_f / yard_f:.2f} | on the floor {np.mean(of == 0):.4f}")
    if name in H.ACCURACY_SIGNALS:
        assert np.mean(of == 0) <= 0.05              # elements on the -80 dB floor are 0 in both results and prove nothing
    assert np.isfinite(power).all() and np.isfinite(feats).all()
    assert err_p <= bound_p and err_f <= bound_f, (name, n, pad_mode, err_p, bound_p, err_f, bound_f)
    assert feats.min() >= 0.0 and feats.max() <= 1.0
    return err_p / yard_p, err_f / yard_f


# ---- accuracy --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
@pytest.mark.parametrize("name", H.SIGNALS)
def test_power_and_features_against_the_fp64_oracle(name, pad_mode):
    """Signals (a) noise and (b) chirp are the accuracy evidence; (c) tone and (d) tone + silence sit on the -80 dB floor in most
    elements and test the clamp under the same bound.  Lengths: 2048 (F = 9, Tm = 8: every frame touches padding, a downsizing
    resize), 2303 / 2304 (F steps from 9 to 10), 22050 (F = 87, Tm = 90), 44100."""
    ms = spec(pad_mode)
    for n in LENGTHS:
        y = torch.from_numpy(H.signal(name, n))
        check_against_oracle(name, n, pad_mode, ms.power(y)[0].cpu().numpy(), ms.features(y)[0].cpu().numpy())


@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_one_full_window_of_two_clips(pad_mode):
    """N = 1 323 000 (60 s: F = 5168, Tm = 5400), B = 2: 646 workgroups per clip, the shape a conducting call has."""
    n = 1323000
    y = torch.from_numpy(np.stack([H.signal("noise", n), H.signal("chirp", n)]))
    ms = spec(pad_mode)
    p, f = ms.power(y).cpu().numpy(), ms.features(y).cpu().numpy()
    assert p.shape == (2, 5168, 128) and f.shape == (2, 5400, 128)
    for i, name in enumerate(("noise", "chirp")):
        check_against_oracle(name, n, pad_mode, p[i], f[i])


# ---- edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_silence_is_exactly_one(pad_mode):
    ms = spec(pad_mode)
    y = torch.zeros(2, 22050)
    y[1] = torch.from_numpy(H.signal("noise", 22050))
    f, p = ms.features(y), ms.power(y)
    assert bits(p[0]).max() == 0                                        # power 0 ...
    assert np.array_equal(bits(f[0]), np.full((90, 128), np.float32(1.0).view(np.uint32)))      # ... dB 0, |0 + 80| / 80 = 1
    assert np.array_equal(bits(f[1]), bits(ms.features(y[1])[0]))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_a_non_finite_sample_poisons_its_clip_and_no_other(pad_mode, bad):
    """numpy's max and maximum propagate NaN: with one NaN sample `ref` is NaN and every element of the clip with it; +inf ends the
    same way (inf - inf in the transform).  fmaxf would drop it at four places."""
    ms = spec(pad_mode)
    n = 22050
    clean = np.stack([H.signal("noise", n), H.signal("chirp", n), H.signal("tone", n)])
    want = ms.features(torch.from_numpy(clean))
    for at in (0, 5000, n - 1):                      # the first sample sits under the window's zero in its first frame
        y = clean.copy()
        y[1, at] = bad
        got = ms.features(torch.from_numpy(y))
        assert (value_class(got[1].cpu().numpy()) == 3).all(), (at, np.unique(value_class(got[1].cpu().numpy())))
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[2]), bits(want[2]))
        p = ms.power(torch.from_numpy(y))[1].cpu().numpy()
        touched = (value_class(p) != 0).any(axis=1)
        assert touched.any() and not touched.all()   # the power keeps it to the frames that hold the sample
    with np.errstate(invalid="ignore"):
        host = M.mel_features_host(y[1], pad_mode=pad_mode)
    assert (value_class(host) == 3).all()            # the numpy restatement agrees


def test_same_length_resize_returns_the_normalised_rows():
    """Tm_b = F_b: x = j exactly, w = 0 - the rows of |dB + 80| / 80, flipped, unchanged.  Bit for bit against the rows 3 m + 1 of the
    resize to 3 F_b, whose coordinate is m exactly; within fp32 rounding against the power normalised on the host."""
    ms = spec()
    n = 22050
    y = torch.from_numpy(np.stack([H.signal("chirp", n), H.signal("noise", n)]))
    F = 1 + n // 256
    same, triple = ms.features(y, mel_len_90fps=F), ms.features(y, mel_len_90fps=3 * F)
    assert same.shape == (2, F, 128) and triple.shape == (2, 3 * F, 128)
    assert np.array_equal(bits(same), bits(triple[:, 1::3]))
    p = ms.power(y).cpu().numpy()
    for b in range(2):
        db = np.float32(10) * np.log10(np.maximum(np.float32(1e-10), p[b])) - np.float32(10) * np.log10(np.maximum(np.float32(1e-10), p[b].max()))
        v = (np.abs(np.maximum(db, np.float32(-80)) + np.float32(80)) / np.float32(80))[:, ::-1]
        # two logarithms (|log10| < 16: an ulp is 2^-20) that the two libraries may each round 2 ulp apart, times 10, over 80; the rest
        # of the chain rounds at the ulp of 100 dB, 2^-17, three times
        assert np.abs(same[b].cpu().numpy() - v).max() <= (2 * 4 * 10 * 2.0 ** -20 + 3 * 2.0 ** -17) / 80
    assert same[0].cpu().numpy().max() == 1.0        # the loudest element is dB 0


# ---- batch independence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_a_clip_has_the_same_bits_alone_in_a_batch_and_on_a_rerun(pad_mode):
    ms = spec(pad_mode)
    lens = (2048, 22050, 30000)
    names = ("noise", "chirp", "tone_silence")
    N = max(lens)
    batch = np.full((3, N), np.nan, np.float32)      # what lies behind a clip's length is never read
    for i, (name, n) in enumerate(zip(names, lens)):
        batch[i, :n] = H.signal(name, n)
    yb = torch.from_numpy(batch)
    p, f = ms.power(yb, lens), ms.features(yb, lens)
    assert p.shape == (3, 1 + N // 256, 128) and f.shape == (3, H.out_frames(N), 128)
    assert np.array_equal(bits(p), bits(ms.power(yb, lens))) and np.array_equal(bits(f), bits(ms.features(yb, lens)))
    for i, (name, n) in enumerate(zip(names, lens)):
        Fb, Tb = 1 + n // 256, H.out_frames(n)
        alone = torch.from_numpy(H.signal(name, n))
        assert np.array_equal(bits(p[i, :Fb]), bits(ms.power(alone)[0])), name
        assert np.array_equal(bits(f[i, :Tb]), bits(ms.features(alone)[0])), name
        assert bits(p[i, Fb:]).max(initial=0) == 0 and bits(f[i, Tb:]).max(initial=0) == 0      # rows behind F_b / Tm_b are 0
        check_against_oracle(name, n, pad_mode, p[i, :Fb].cpu().numpy(), f[i, :Tb].cpu().numpy())


def test_a_batch_larger_than_a_pass_equals_two_calls():
    ms = spec()
    chunk = native.mel_pass_clips(2048)
    assert chunk == 32
    rng = np.random.default_rng(77)
    y = torch.from_numpy((0.1 * rng.standard_normal((chunk + 3, 2048))).astype(np.float32))
    lens = [2048] * (chunk + 3)
    whole_f, whole_p = ms.features(y, lens), ms.power(y, lens)
    cut = 7
    assert np.array_equal(bits(whole_f), np.concatenate([bits(ms.features(y[:cut])), bits(ms.features(y[cut:]))]))
    assert np.array_equal(bits(whole_p), np.concatenate([bits(ms.power(y[:cut])), bits(ms.power(y[cut:]))]))
    assert len({bits(whole_f[i]).tobytes() for i in range(chunk + 3)}) == chunk + 3      # (the clips differ)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    L = native.lib()
    h = spec()._native._h
    ip = C.POINTER(C.c_int32)
    dev = torch.device("cuda:0")
    y = torch.from_numpy(H.signal("noise", 4096)).to(dev).reshape(1, 4096)
    out = torch.full((2, 20, 128), -7.0, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def arr(*v):
        return (C.c_int32 * len(v))(*v)

    def refused(rc, text):
        torch.cuda.synchronize()
        assert rc == -1 and text in L.dc_last_error().decode(), (rc, L.dc_last_error())
        assert (out == -7.0).all()

    yp, op = y.data_ptr(), out.data_ptr()
    refused(L.dc_mel_features(h, yp, None, 0, 4096, None, 16, op, stream), "B must be >= 1")
    refused(L.dc_mel_features(h, yp, None, 1, 2047, None, 16, op, stream), "N >= 2048")
    refused(L.dc_mel_features(h, yp, arr(2047), 1, 4096, None, 16, op, stream), "length 2047 of clip 0")
    refused(L.dc_mel_features(h, yp, arr(4097), 1, 4096, None, 16, op, stream), "length 4097 of clip 0")
    refused(L.dc_mel_features(h, yp, None, 1, 4096, None, 0, op, stream), "Tm must be >= 1")
    refused(L.dc_mel_features(h, yp, None, 1, 4096, arr(0), 16, op, stream), "outside [1, 16]")
    refused(L.dc_mel_features(h, yp, None, 1, 4096, arr(17), 16, op, stream), "outside [1, 16]")
    refused(L.dc_mel_features(h, yp, None, 1, 4096, None, 15, op, stream), "the default of 16 output frames")
    refused(L.dc_mel_features(h, None, None, 1, 4096, None, 16, op, stream), "NULL")
    refused(L.dc_mel_features(h, yp, None, 1, 4096, None, 16, None, stream), "NULL")
    refused(L.dc_mel_features(None, yp, None, 1, 4096, None, 16, op, stream), "NULL")
    refused(L.dc_mel_power(h, yp, None, 0, 4096, op, stream), "B must be >= 1")
    refused(L.dc_mel_power(h, yp, None, 1, 100, op, stream), "N >= 2048")
    refused(L.dc_mel_power(h, yp, arr(5000), 1, 4096, op, stream), "length 5000 of clip 0")
    refused(L.dc_mel_power(h, yp, None, 1, 4096, None, stream), "NULL")
    refused(L.dc_mel_power(None, yp, None, 1, 4096, op, stream), "NULL")
    made = C.c_void_p()
    refused(L.dc_mel_create(0, 0, 0, C.byref(made)), "sr 0 must be >= 1")
    refused(L.dc_mel_create(0, 22050, 2, C.byref(made)), "unknown pad_mode 2")
    refused(L.dc_mel_create(0, 22050, 0, None), "out is NULL")
    assert not made.value
    with pytest.raises(ValueError, match="pad_mode"):
        M.MelSpectrogram("cuda:0", pad_mode="edge")
    with pytest.raises(ValueError, match="2048"):
        spec().features(torch.zeros(1, 2000))
    with pytest.raises(ValueError, match="lengths"):
        spec().features(torch.zeros(2, 4096), [4096, 100])
    # the same call, accepted, writes its rows and leaves the rest of the buffer alone
    assert L.dc_mel_features(h, yp, None, 1, 4096, None, 16, op, stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.reshape(-1)[:16 * 128].reshape(16, 128)), bits(spec().features(y)[0]))
    assert (out.reshape(-1)[16 * 128:] == -7.0).all()


def test_another_sample_rate_moves_the_filterbank_and_the_length():
    y = H.signal("noise", 16000)
    got = spec("constant", 16000).features(torch.from_numpy(y))[0].cpu().numpy()
    want = H.mel_features(y, sr=16000)
    assert got.shape == want.shape == (90, 128)
    yard = np.abs(M.mel_features_host(y, sr=16000).astype(np.float64) - want).max()
    assert np.abs(got - want).max() <= max(8 * yard, FLOOR)
    assert np.abs(H.mel_features(y, sr=22050, mel_len_90fps=90) - want).max() > 1e-2      # (the rate matters)


# ---- into the encoder and through the front door -----------------------------------------------------------------------------------
def test_features_feed_the_music_encoder_without_a_copy(tmp_path):
    model = make_model()
    f = spec().features(torch.from_numpy(H.signal("chirp", 44100)))
    assert f.is_cuda and f.dtype == torch.float32 and f.is_contiguous() and tuple(f.shape) == (1, 180, 128)
    a = model.encode_music(f, "cuda:0")
    np.save(tmp_path / "mel.npy", f[0].cpu().numpy())
    b = model.encode_music(torch.from_numpy(np.load(tmp_path / "mel.npy")).unsqueeze(0), "cuda:0")
    assert tuple(a[0].shape) == (1, 60, 64) and torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def _write_wav16(path, y, rate=22050):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.round(np.clip(y, -1, 1) * 32767).astype("<i2").tobytes())


def test_visualize_conducts_a_wav_as_it_conducts_its_mel(tmp_path):
    """visualize.main on a 2-s WAV = visualize.main on the --save_mel file of that run, bit for bit; the saved mel is
    extract_mel_feature of the file (tests/test_gpu_stages.py has the checkpoint and opt.txt this is modelled on)."""
    from diffusion_conductor_amd import visualize
    root = tmp_path / "checkpoints" / "ConductorMotion100" / "train"
    (root / "model").mkdir(parents=True)
    torch.save({"encoder": {k: torch.from_numpy(np.asarray(v)) for k, v in state_dict_np().items()}, "ep": 3, "total_it": 77},
               root / "model" / "latest.tar")
    (root / "opt.txt").write_text(
        "------------ Options -------------\n"
        f"checkpoints_dir: {tmp_path / 'checkpoints'}\ndataset_name: ConductorMotion100\nname: train\nunit_length: 4\n"
        "latent_dim: 128\nnum_layers: 8\ndiffusion_steps: 50\nno_clip: True\nno_eff: False\nlr: 0.0002\nis_train: True\n"
        "-------------- End ----------------\n")
    _write_wav16(tmp_path / "song.wav", H.signal("chirp", 44100))
    common = ["--opt_path", str(root / "opt.txt"), "--gpu_id", "0", "--seed", "7"]
    from_wav = visualize.main(common + ["--music_path", str(tmp_path / "song.wav"), "--save_mel", str(tmp_path / "mel.npy"),
                                        "--npy_path", str(tmp_path / "kp.npy")])
    mel = np.load(tmp_path / "mel.npy")
    assert mel.shape == (180, 128) and mel.dtype == np.float32
    assert np.array_equal(mel, M.extract_mel_feature(str(tmp_path / "song.wav")))
    y, sr = M.load_audio(tmp_path / "song.wav")
    assert sr == 22050 and np.abs(mel - H.mel_features(y)).max() <= max(8 * np.abs(M.mel_features_host(y) - H.mel_features(y)).max(), FLOOR)
    from_mel = visualize.main(common + ["--music_path", str(tmp_path / "mel.npy")])
    assert from_wav.shape == (60, 13, 2) and np.isfinite(from_wav).all()
    assert np.array_equal(from_wav.view(np.uint32), from_mel.view(np.uint32))
    assert np.array_equal(np.load(tmp_path / "kp.npy"), from_wav)
    # a directory of WAV files of two lengths is one batch; the shorter file's rows behind its own length are 0
    d = tmp_path / "songs"
    d.mkdir()
    _write_wav16(d / "a.wav", H.signal("chirp", 44100))
    _write_wav16(d / "b.wav", H.signal("noise", 30000))
    both = visualize.main(common + ["--music_path", str(d), "--save_mel", str(tmp_path / "mels.npy")])
    mels = np.load(tmp_path / "mels.npy")
    assert both.shape == (2, 60, 13, 2) and mels.shape == (2, 180, 128)
    assert np.array_equal(mels[0], mel) and not mels[1, H.out_frames(30000):].any() and mels[1, :H.out_frames(30000)].any()
