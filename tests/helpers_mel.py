"""The fp64 oracle of the mel front end (csrc/dc_mel.hip, diffusion_conductor_amd/mel.py) and the seeded signals its tests share.

numpy only, written from the definitions - librosa's documented STFT / Slaney filterbank / power_to_db and cv2's half-pixel
INTER_LINEAR rule -, needing neither scipy, nor librosa, nor cv2, nor the reference.  Nothing here imports the package: the
oracle must not share a line with what it judges."""
import numpy as np

N_FFT, HOP, N_MELS, BINS = 2048, 256, 128, 1025
SR = 22050


# ---- Slaney's mel scale (librosa.hz_to_mel / mel_to_hz with htk=False) ----------------------------------------------------------
def hz_to_mel(f):
    f = np.asarray(f, np.float64)
    lin = f / (200.0 / 3.0)
    log = 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0)
    return np.where(f >= 1000.0, log, lin)


def mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def mel_frequencies(n_mels, fmin, fmax):
    return mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels))


def mel_filterbank(sr=SR, n_fft=N_FFT, n_mels=N_MELS):
    """librosa.filters.mel(sr, n_fft, n_mels) with its defaults (fmin 0, fmax sr / 2, Slaney norm) in fp64: [n_mels, 1 + n_fft / 2]."""
    fft_f = np.arange(1 + n_fft // 2, dtype=np.float64) * (float(sr) / n_fft)
    mel_f = mel_frequencies(n_mels + 2, 0.0, sr / 2.0)
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    w = np.zeros((n_mels, fft_f.shape[0]))
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
    return w * (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]


def hann(n=N_FFT):
    """The periodic Hann window (scipy.signal.get_window('hann', n, fftbins=True))."""
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


# ---- STFT, mel power, dB, resize -------------------------------------------------------------------------------------------------
def pad_signal(y, pad_mode):
    y = np.asarray(y, np.float64)
    if pad_mode == "constant":
        return np.concatenate([np.zeros(N_FFT // 2), y, np.zeros(N_FFT // 2)])
    assert pad_mode == "reflect", pad_mode
    return np.concatenate([y[N_FFT // 2:0:-1], y, y[-2:-N_FFT // 2 - 2:-1]])


def stft_frames(y, pad_mode="constant"):
    """librosa.stft(y, n_fft=2048, hop_length=256, center=True, pad_mode=...).T: complex [1 + len(y) // 256, 1025]."""
    p = pad_signal(y, pad_mode)
    F = 1 + (p.shape[0] - N_FFT) // HOP
    idx = np.arange(F)[:, None] * HOP + np.arange(N_FFT)[None, :]
    return np.fft.rfft(p[idx] * hann()[None, :], axis=1)


def mel_power(y, sr=SR, pad_mode="constant"):
    """librosa.feature.melspectrogram(y, sr, n_mels=128, hop_length=256).T in fp64: [F, 128]."""
    X = stft_frames(y, pad_mode)
    return (X.real ** 2 + X.imag ** 2) @ mel_filterbank(sr).T


def power_to_unit(p):
    """|power_to_db(p, ref=np.max) + 80| / 80 (amin 1e-10, top_db 80)."""
    p = np.asarray(p, np.float64)
    db = 10.0 * np.log10(np.maximum(1e-10, p)) - 10.0 * np.log10(np.maximum(1e-10, np.max(p)))
    db = np.maximum(db, np.max(db) - 80.0)
    return np.abs(db + 80.0) / 80.0


def out_frames(n, sr=SR):
    """The reference's int(len(y) / sr * 90), Python's own arithmetic."""
    return int(n / sr * 90)


def resize_time(v, Tm):
    """cv2.resize(v.T, (Tm, C), interpolation=INTER_LINEAR).T for v [F, C]: the half-pixel rule along time, in v's dtype, with the
    source coordinate rounded to fp32 as cv2 does."""
    v = np.asarray(v)
    F = v.shape[0]
    x = ((np.arange(Tm, dtype=np.float64) + 0.5) * (F / Tm) - 0.5).astype(np.float32)
    i = np.floor(x).astype(np.int64)
    w = (x - i.astype(np.float32)).astype(np.float32)
    lo = i < 0
    hi = i >= F - 1
    i = np.where(lo, 0, np.where(hi, F - 1, i))
    w = np.where(lo | hi, np.float32(0), w).astype(v.dtype)
    i1 = np.minimum(i + 1, F - 1)
    return v[i] * (1 - w)[:, None] + v[i1] * w[:, None]


def mel_features(y, sr=SR, mel_len_90fps=None, pad_mode="constant"):
    """extract_mel_feature (Diffusion_Stage/tools/visualization.py:152-167) behind librosa.load, in fp64: [Tm, 128]."""
    y = np.asarray(y, np.float64)
    Tm = out_frames(y.shape[0], sr) if mel_len_90fps is None else int(mel_len_90fps)
    v = power_to_unit(mel_power(y, sr, pad_mode))[:, ::-1]
    return resize_time(v, Tm)


# ---- the seeded signals of the tests (sr = 22050) --------------------------------------------------------------------------------
SIGNALS = ("noise", "chirp", "tone", "tone_silence")
ACCURACY_SIGNALS = ("noise", "chirp")            # the other two sit on the -80 dB floor nearly everywhere: the clamp's test


def signal(name, n, sr=SR):
    """fp32 [n]: (a) white noise at 0.1, (b) a 200 -> 6200 Hz chirp at 0.5 (one sweep per 2 s) plus noise at 1e-3, (c) a pure 440 Hz
    tone, (d) a tone followed by silence."""
    rng = np.random.default_rng({"noise": 21, "chirp": 22, "tone": 23, "tone_silence": 24}[name] * 100003 + n)
    t = np.arange(n, dtype=np.float64) / sr
    if name == "noise":
        y = 0.1 * rng.standard_normal(n)
    elif name == "chirp":
        # 200 -> 6200 Hz in 2 s, then again (the phase is continuous: 6400 whole cycles per sweep), whatever n: a shorter signal is a
        # prefix of a longer one.  One sweep stretched over 60 s would be a near-stationary tone in every frame, whose peak puts the
        # 1e-3 noise at -79.3 dB - on the floor in 6.4 % of the elements, where both results are 0 and prove nothing.
        ts = np.arange(n, dtype=np.int64) % (2 * sr) / sr
        y = 0.5 * np.sin(2.0 * np.pi * (200.0 * ts + 0.5 * 3000.0 * ts * ts)) + 1e-3 * rng.standard_normal(n)
    elif name == "tone":
        y = 0.5 * np.sin(2.0 * np.pi * 440.0 * t)
    else:
        y = 0.5 * np.sin(2.0 * np.pi * 440.0 * t)
        y[n // 2:] = 0.0
    return y.astype(np.float32)


_cache = {}


def oracle(name, n, pad_mode, what):
    """The fp64 result for signal(name, n): what = "power" [F, 128] or "features" [Tm, 128]; computed once per session."""
    key = (name, n, pad_mode)
    if key not in _cache:
        y = signal(name, n)
        p = mel_power(y, SR, pad_mode)
        _cache[key] = {"power": p, "features": resize_time(power_to_unit(p)[:, ::-1], out_frames(n))}
    return _cache[key][what]
