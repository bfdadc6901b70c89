"""The mel front end on a CPU-only box: the fp64 oracle against what pins it (librosa and cv2 are installed nowhere this project
runs, so nothing here is a comparison with a run of them), the tables the library uploads, the numpy restatement, the output
length, the WAV reader and the front door's refusals.  The kernels are tested in tests/test_gpu_mel.py."""
import os
import wave

import numpy as np
import pytest

import helpers_mel as H
from helpers import golden

from diffusion_conductor_amd import mel as M
from diffusion_conductor_amd import native


# ---- what pins the oracle --------------------------------------------------------------------------------------------------------
def test_oracle_reproduces_librosas_documented_values():
    """The examples in librosa's docstrings: mel_frequencies(n_mels=40) (fmin 0, fmax 11025) and mel(sr=22050, n_fft=2048), to
    the three decimals they are printed with."""
    mf = H.mel_frequencies(40, 0.0, 11025.0)
    assert np.abs(mf[:4] - [0.0, 85.317, 170.635, 255.952]).max() < 5e-4
    assert np.abs(mf[12:14] - [1024.856, 1119.114]).max() < 5e-4
    fb = H.mel_filterbank(22050, 2048, 128)
    assert fb.shape == (128, 1025) and np.abs(fb[0, :3] - [0.0, 0.016, 0.032]).max() < 5e-4
    nz = (fb > 0).sum(axis=1)
    assert nz.min() == 4 and nz.max() == 53          # no empty filter; a dense product would waste 95 % of its work
    assert M.out_frames(22050) == 90 and H.out_frames(1323000) == 5400


@pytest.mark.parametrize("pad_mode, boundary", [("constant", "zeros"), ("reflect", "even")])
def test_oracle_stft_against_scipy(pad_mode, boundary):
    signal = pytest.importorskip("scipy.signal")
    for n in (2048, 2303, 2304, 22050):
        y = H.signal("noise", n).astype(np.float64)
        _, _, Z = signal.stft(y, window="hann", nperseg=2048, noverlap=1792, boundary=boundary, padded=False)
        X = H.stft_frames(y, pad_mode)
        assert X.shape == (1 + n // 256, 1025) and Z.T.shape == X.shape
        assert np.abs(Z.T * H.hann().sum() - X).max() <= 1e-11 * np.abs(X).max()


def test_oracle_window_and_scale_by_a_closed_form():
    """A sine of amplitude a at exactly bin k: |X[k]| = a 2048 / 4 and |X[k +- 1]| = a 2048 / 8 under the PERIODIC Hann window (the
    symmetric one, n / 2047, misses both by 1e-3), in a frame away from the edges."""
    a, k = 0.37, 41
    y = a * np.sin(2.0 * np.pi * k * np.arange(8192) / 2048.0 + 0.3)
    X = np.abs(H.stft_frames(y, "constant")[16])
    assert abs(X[k] - a * 512.0) < 1e-9 and abs(X[k - 1] - a * 256.0) < 1e-9 and abs(X[k + 1] - a * 256.0) < 1e-9
    assert X[k + 2:].max() < 1e-9 and X[:k - 1].max() < 1e-9


def test_oracle_resize_is_cv2s_half_pixel_rule():
    rng = np.random.default_rng(5)
    v = rng.random((10, 3))
    assert np.array_equal(H.resize_time(v, 10), v)                       # Tm = F: the input's bits
    assert np.array_equal(H.resize_time(v.astype(np.float32), 10), v.astype(np.float32))
    down = H.resize_time(v, 9)                                           # x = (j + 0.5) 10 / 9 - 0.5: j = 4 sits at 4.5
    assert np.allclose(down[4], 0.5 * (v[4] + v[5]), rtol=0, atol=1e-7)  # (the coordinate is rounded to fp32)
    w0 = float(np.float32(0.5 * 10 / 9 - 0.5))
    assert np.allclose(down[0], v[0] * (1 - w0) + v[1] * w0, rtol=0, atol=1e-15)
    up = H.resize_time(v[:9], 20)                                        # x(0) = -0.275: clamped to v[0]; x(19) = 8.275: to v[8]
    assert np.array_equal(up[0], v[0]) and np.array_equal(up[19], v[8])
    assert np.allclose(up[10], v[4] * 0.775 + v[5] * 0.225, rtol=0, atol=1e-7)      # x(10) = 10.5 * 0.45 - 0.5 = 4.225


# ---- the tables the library uploads ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [22050, 16000])
def test_tables_are_the_fp32_rounding_of_the_oracle(sr):
    t = native.mel_tables(sr)
    assert np.array_equal(t["window"], H.hann().astype(np.float32))
    j = np.arange(2048, dtype=np.float64) * (2.0 * np.pi / 2048.0)
    assert np.abs(t["twiddle"] - np.stack([np.cos(j), -np.sin(j)], axis=1)).max() <= 2.0 ** -24
    first, count = t["first"].astype(np.int64), t["count"].astype(np.int64)
    assert count.min() >= 1 and (first >= 0).all() and (first + count <= 1025).all() and int(count.sum()) == t["weights"].size
    dense, at = np.zeros((128, 1025), np.float32), 0
    for m in range(128):
        dense[m, first[m]:first[m] + count[m]] = t["weights"][at:at + count[m]]
        at += count[m]
    assert np.array_equal(dense, H.mel_filterbank(sr).astype(np.float32))
    assert (t["weights"] != 0).all()


def test_tables_refuse_bad_arguments():
    with pytest.raises(native.DcError, match="sr must be >= 1"):
        native.mel_tables(0)
    small = np.empty(8, np.float32)
    assert native.lib().dc_mel_tables(22050, None, None, None, None, native._fptr(small), 8, None) == -1
    assert b"do not fit" in native.lib().dc_last_error()
    assert native.mel_pass_clips(2047) == 0 and native.mel_pass_clips(2048) == 32 and native.mel_pass_clips(1323000) == 32
    assert native.mel_pass_clips(60 * 22050 * 20) == (1 << 27) // ((1 + 60 * 22050 * 20 // 256) * 128)


# ---- the output length -----------------------------------------------------------------------------------------------------------
def test_output_length_is_pythons_double_expression():
    """int(n / sr * 90): the package's and the ABI's copies against Python's, over ranges where the product is not exact - and
    where n * 90 // sr, the integer form, disagrees."""
    disagree = 0
    for sr, ns in ((22050, range(2048, 16001)), (22050, range(1322000, 1323001)), (16000, range(2048, 4096)),
                   (44100, range(88000, 89000))):
        for n in ns:
            want = int(n / sr * 90)
            assert M.out_frames(n, sr) == want and native.mel_out_frames(n, sr) == want and H.out_frames(n, sr) == want, (n, sr)
            disagree += want != n * 90 // sr
    assert disagree > 0                                # the trap is inside the range
    assert native.mel_out_frames(-1, 22050) == 0 and native.mel_out_frames(2048, 0) == 0


# ---- the numpy restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad_mode", ["constant", "reflect"])
def test_host_restatement_against_the_oracle(pad_mode):
    for name in H.SIGNALS:
        for n in (2048, 2303, 2304, 22050):
            y = H.signal(name, n)
            want = H.oracle(name, n, pad_mode, "features")
            assert want.shape == (H.out_frames(n), 128)
            got64 = M.mel_features_host(y, pad_mode=pad_mode, dtype=np.float64)
            assert got64.dtype == np.float64 and np.abs(got64 - want).max() <= 1e-12
            got32 = M.mel_features_host(y, pad_mode=pad_mode)
            assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 2e-5      # fp32 through a -80 dB logarithm
            p = M.mel_power_host(y, pad_mode=pad_mode, dtype=np.float64)
            ref = H.oracle(name, n, pad_mode, "power")
            assert np.abs(p - ref).max() <= 1e-12 * ref.max()
    silent = M.mel_features_host(np.zeros(4096, np.float32), pad_mode=pad_mode)
    assert silent.shape == (16, 128) and (silent == 1.0).all()
    bad = H.signal("noise", 4096).copy()
    bad[1000] = np.nan
    assert np.isnan(M.mel_features_host(bad, pad_mode=pad_mode)).all()
    assert M.mel_features_host(H.signal("noise", 4096), mel_len_90fps=5, pad_mode=pad_mode).shape == (5, 128)


def test_host_restatement_and_oracle_against_the_fixture():
    g = golden("g21_mel.npz")
    cases = [(name, 2304, pad) for name in H.SIGNALS for pad in ("constant", "reflect")] + [("chirp", 22050, "constant")]
    for name, n, pad in cases:
        y = g[f"wave_{name}_{n}"]
        assert y.dtype == np.float32 and np.array_equal(y, H.signal(name, n))
        assert np.abs(H.oracle(name, n, pad, "features") - g[f"features_{name}_{n}_{pad}"]).max() <= 1e-12
        assert np.abs(H.oracle(name, n, pad, "power") / g[f"power_{name}_{n}_{pad}"].max() - g[f"power_{name}_{n}_{pad}"] /
                      g[f"power_{name}_{n}_{pad}"].max()).max() <= 1e-12
        assert np.abs(M.mel_features_host(y, pad_mode=pad, dtype=np.float64) - g[f"features_{name}_{n}_{pad}"]).max() <= 1e-12


def test_pad_modes_differ_in_the_edge_frames_only():
    y = H.signal("noise", 22050)
    a, b = H.mel_power(y, pad_mode="constant"), H.mel_power(y, pad_mode="reflect")
    differs = np.abs(a - b).max(axis=1) > 0
    assert differs[:4].all() and differs[-4:].all() and not differs[4:-4].any()
    with pytest.raises(ValueError, match="pad_mode"):
        M.mel_power_host(y, pad_mode="edge")
    with pytest.raises(ValueError, match="2048"):
        M.mel_power_host(y[:2047])


# ---- audio in --------------------------------------------------------------------------------------------------------------------
def _write_wav(path, frames, width, rate=22050):
    """frames: int64 [n, channels] of `width`-byte little-endian PCM."""
    raw = np.zeros(frames.shape + (width,), np.uint8)
    u = frames & ((1 << (8 * width)) - 1)
    for i in range(width):
        raw[..., i] = (u >> (8 * i)) & 0xFF
    with wave.open(str(path), "wb") as f:
        f.setnchannels(frames.shape[1])
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(raw.tobytes())


@pytest.mark.parametrize("width", [2, 3, 4])
def test_load_audio_reads_pcm_wav(tmp_path, width):
    rng = np.random.default_rng(width)
    top = 1 << (8 * width - 1)
    frames = rng.integers(-top, top, size=(3000, 2), dtype=np.int64)
    frames[0], frames[1] = (-top, -top), (top - 1, top - 1)          # both ends of the range
    _write_wav(tmp_path / "a.wav", frames, width)
    y, sr = M.load_audio(tmp_path / "a.wav")
    assert sr == 22050 and y.dtype == np.float32 and y.shape == (3000,)
    assert np.array_equal(y, (frames.astype(np.float64) / top).mean(axis=1).astype(np.float32))
    assert y[0] == -1.0 and y[1] == np.float32((top - 1) / top)
    y2, sr2 = M.load_audio(tmp_path / "a.wav", sr=None)
    assert sr2 == 22050 and np.array_equal(y, y2)


def test_load_audio_resamples_or_names_the_rates(tmp_path):
    n = np.arange(16000)
    frames = np.round(12000 * np.sin(2 * np.pi * 440.0 * n / 16000.0)).astype(np.int64)[:, None]
    _write_wav(tmp_path / "b.wav", frames, 2, rate=16000)
    y, sr = M.load_audio(tmp_path / "b.wav", sr=None)
    assert sr == 16000 and y.shape == (16000,)
    try:
        import scipy.signal  # noqa: F401
    except ImportError:
        with pytest.raises(ValueError, match="16000.*22050"):
            M.load_audio(tmp_path / "b.wav")
    else:
        y, sr = M.load_audio(tmp_path / "b.wav")
        assert sr == 22050 and y.shape == (22050,) and y.dtype == np.float32
        t = np.arange(2000, 20000)
        assert np.abs(y[t] - (12000 / 32768) * np.sin(2 * np.pi * 440.0 * t / 22050.0)).max() < 2e-3


def test_load_audio_and_the_front_door_refuse_other_containers(tmp_path):
    from diffusion_conductor_amd import visualize
    with pytest.raises(ValueError, match="mp3"):
        M.load_audio("x.mp3")
    _write_wav(tmp_path / "c.wav", np.zeros((10, 1), np.int64), 1)
    with pytest.raises(ValueError, match="16, 24 or 32 bits"):
        M.load_audio(tmp_path / "c.wav")
    with pytest.raises(ValueError, match="audio decoding"):
        visualize.load_mels("x.mp3")
    assert visualize.audio_files("x.mp3") is None and visualize.audio_files("m.npy") is None
    assert visualize.audio_files("song.wav") == ["song.wav"]
    d = tmp_path / "songs"
    d.mkdir()
    for name in ("b.wav", "a.WAV", "notes.txt"):
        (d / name).write_bytes(b"")
    assert visualize.audio_files(str(d)) == [os.path.join(str(d), "a.WAV"), os.path.join(str(d), "b.wav")]
    (d / "mel.npy").write_bytes(b"")
    assert visualize.audio_files(str(d)) is None              # a directory that holds mels is load_mels's
    args = visualize.make_parser().parse_args(["--opt_path", "o.txt", "--music_path", "song.wav", "--save_mel", "m.npy"])
    assert args.music_path == "song.wav" and args.save_mel == "m.npy"
