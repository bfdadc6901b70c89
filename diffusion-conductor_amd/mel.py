"""The mel spectrogram the models read, from a waveform, on the MI355X: the first step of "audio in, poses out".

The reference's ``extract_mel_feature`` (Diffusion_Stage/tools/visualization.py:152-167, the same function in
Contrastive_Stage/utils/music_utils.py:8-23 and ProspectiveCup/utils/music_utils.py) is closed-form arithmetic behind
``librosa.load``::

    mel    = librosa.feature.melspectrogram(y=y, sr=sr, n_mels=128, hop_length=256)    # STFT 2048 / 256, Hann, Slaney filterbank
    mel_dB = librosa.power_to_db(mel, ref=np.max)
    norm   = np.flip(np.abs(mel_dB + 80) / 80, 0)                                      # channel 0 is the highest band
    return cv2.resize(norm, (int(len(y) / sr * 90), 128)).T                            # linear, along time, to 90 fps

``MelSpectrogram`` computes it per clip of a batch with csrc/dc_mel.hip (dc_mel_* in include/dc_ddim.h); its ``features`` is the
``[B, Tm, 128]`` device tensor ``MotionTransformer.encode_music`` reads.  ``extract_mel_feature`` has the reference's name and
argument order and returns the numpy ``[Tm, 128]`` the dataset stores as ``mel.npy``.  ``mel_features_host`` restates the function
in numpy for a box without a GPU (the precedent of metrics.motion_beats_host).

``pad_mode``: librosa's ``stft`` pads the 1024 samples in front of and behind the clip with zeros since 0.10 (``"constant"``, the
default here) and reflected the clip before (``"reflect"``); the reference pins no version.  The two differ in the first and last
four STFT frames only - plus ``ref``, should the clip's maximum sit there.

Neither librosa nor cv2 is a dependency, and nothing here was compared with a run of them: the arithmetic is pinned to librosa's
documented values, an independent STFT and cv2's half-pixel rule (tests/helpers_mel.py, tests/test_host_mel.py).  mp3 and other
containers stay outside: ``load_audio`` reads PCM WAV.
"""
from __future__ import annotations

import os

import numpy as np

N_FFT, HOP, N_MELS = 2048, 256, 128
PAD_MODES = ("constant", "reflect")


def out_frames(n, sr=22050):
    """The reference's ``int(len(y) / sr * 90)``: the 90-fps frames of n samples (a double division, a double product, truncation;
    dc_mel_out_frames is the library's copy)."""
    return int(int(n) / int(sr) * 90)


# ---- audio in ---------------------------------------------------------------------------------------------------------------
def load_audio(path, sr=22050):
    """A PCM WAV file (16, 24 or 32 bits, any channel count) -> (y fp32 [n] in [-1, 1), sr): the samples scaled by 2^-(bits-1), the
    channels averaged as ``librosa.load(mono=True)`` does.  ``sr`` None keeps the file's rate.  A file at another rate is resampled
    with ``scipy.signal.resample_poly`` when scipy imports (ValueError naming the two rates otherwise).  That is NOT librosa's
    resampler (soxr): the mel of a resampled file differs from the reference's by the two resamplers' difference.  Anything but
    ``.wav`` is refused: there is no mp3 decoder here - convert first (``ffmpeg -i x.mp3 -ar 22050 x.wav``)."""
    import wave
    path = os.fspath(path)
    if not path.lower().endswith(".wav"):
        raise ValueError(f"{path}: load_audio reads PCM .wav files; mp3 and other containers need a decoder this package does not have")
    with wave.open(path, "rb") as f:
        ch, width, rate, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        if f.getcomptype() != "NONE" or width not in (2, 3, 4):
            raise ValueError(f"{path}: PCM of 16, 24 or 32 bits expected, got {8 * width} bits ({f.getcomptype()})")
        raw = np.frombuffer(f.readframes(n), np.uint8)
    raw = raw[:raw.size // (width * ch) * (width * ch)].reshape(-1, ch, width)
    v = np.zeros(raw.shape[:2], np.int64)
    for i in range(width):                             # little endian
        v |= raw[:, :, i].astype(np.int64) << (8 * i)
    v -= (v >> (8 * width - 1)) << (8 * width)         # two's complement
    y = (v.astype(np.float64) / float(1 << (8 * width - 1))).mean(axis=1)
    if sr is not None and int(sr) != rate:
        try:
            from scipy.signal import resample_poly
        except ImportError:
            raise ValueError(f"{path} is sampled at {rate} Hz, not at {int(sr)} Hz, and scipy (resample_poly) is not installed: "
                             "resample the file first") from None
        g = int(np.gcd(int(sr), rate))
        y = resample_poly(y, int(sr) // g, rate // g)
        rate = int(sr)
    return y.astype(np.float32), rate


# ---- the function in numpy ------------------------------------------------------------------------------------------------------
def _slaney_hz(m):
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), (200.0 / 3.0) * m)


def _filterbank(sr):
    """librosa.filters.mel(sr=sr, n_fft=2048, n_mels=128): fp64 [128, 1025]."""
    nyq = sr / 2.0
    top = 15.0 + np.log(nyq / 1000.0) / (np.log(6.4) / 27.0) if nyq >= 1000.0 else nyq / (200.0 / 3.0)
    f = _slaney_hz(np.linspace(0.0, top, N_MELS + 2))
    bins = np.arange(N_FFT // 2 + 1, dtype=np.float64) * (float(sr) / N_FFT)
    lower = (bins[None, :] - f[:N_MELS, None]) / (f[1:N_MELS + 1] - f[:N_MELS])[:, None]
    upper = (f[2:, None] - bins[None, :]) / (f[2:] - f[1:N_MELS + 1])[:, None]
    return np.maximum(0.0, np.minimum(lower, upper)) * (2.0 / (f[2:] - f[:N_MELS]))[:, None]


def mel_power_host(y, sr=22050, pad_mode="constant", dtype=np.float32):
    """``librosa.feature.melspectrogram(y, sr, n_mels=128, hop_length=256).T`` in numpy: [1 + len(y) // 256, 128] of `dtype`."""
    if pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be one of {PAD_MODES}, got {pad_mode!r}")
    y = np.asarray(y, dtype).reshape(-1)
    if y.shape[0] < N_FFT:
        raise ValueError(f"{y.shape[0]} samples: one {N_FFT}-sample window is the least")
    h = N_FFT // 2
    edge = (np.zeros(h, dtype), np.zeros(h, dtype)) if pad_mode == "constant" else (y[h:0:-1], y[-2:-h - 2:-1])
    p = np.concatenate([edge[0], y, edge[1]])
    window = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)).astype(dtype)
    fb = _filterbank(sr).astype(dtype)
    F = 1 + y.shape[0] // HOP
    out = np.empty((F, N_MELS), dtype)
    for f0 in range(0, F, 512):                        # (bounded memory: 512 frames of 2048 samples at a time)
        idx = (np.arange(f0, min(F, f0 + 512)) * HOP)[:, None] + np.arange(N_FFT)[None, :]
        X = np.fft.rfft(p[idx] * window[None, :], axis=1)
        out[f0:f0 + 512] = (X.real ** 2 + X.imag ** 2).astype(dtype) @ fb.T
    return out


def mel_features_host(y, sr=22050, mel_len_90fps=None, pad_mode="constant", dtype=np.float32):
    """``extract_mel_feature`` behind ``librosa.load`` in plain numpy, every array of `dtype` (float32: the reference's own
    precision - librosa's STFT of a float32 waveform is complex64 - and the yardstick of the GPU tests' tolerance): y [n] -> [Tm, 128],
    Tm = ``mel_len_90fps`` or ``int(n / sr * 90)``."""
    p = mel_power_host(y, sr, pad_mode, dtype)
    n = np.asarray(y).reshape(-1).shape[0]
    Tm = out_frames(n, sr) if mel_len_90fps is None else int(mel_len_90fps)
    if Tm < 1:
        raise ValueError(f"{Tm} output frames")
    ten, amin, top = dtype(10.0), dtype(1e-10), dtype(80.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        db = ten * np.log10(np.maximum(amin, p)) - ten * np.log10(np.maximum(amin, np.max(p)))
        db = np.maximum(db, np.max(db) - top)
        v = (np.abs(db + top) / top)[:, ::-1]
        # cv2.resize(.., (Tm, 128)), INTER_LINEAR: the half-pixel source coordinate in double, rounded to fp32, clamped at both ends
        F = v.shape[0]
        x = ((np.arange(Tm, dtype=np.float64) + 0.5) * (F / Tm) - 0.5).astype(np.float32)
        i = np.floor(x).astype(np.int64)
        w = x - i.astype(np.float32)
        edge = (i < 0) | (i >= F - 1)
        i = np.clip(i, 0, F - 1)
        w = np.where(edge, np.float32(0.0), w).astype(dtype)[:, None]
        return (v[i] * (dtype(1.0) - w) + v[np.minimum(i + 1, F - 1)] * w).astype(dtype)


# ---- on the GPU -----------------------------------------------------------------------------------------------------------------
class MelSpectrogram:
    """y: fp32 waveforms [B, N] or [N], torch tensors (on the device or on the host) or arrays, N >= 2048; `lengths`: None or the
    clips' sample counts (a clip's samples behind its length are not read).  Results are device tensors.  `sr` moves the filterbank
    and the default output length only; nothing is resampled."""

    def __init__(self, device="cuda:0", sr=22050, pad_mode="constant"):
        import torch
        from .native import NativeMel
        self.device = torch.device(device)
        self.sr, self.pad_mode = int(sr), pad_mode
        self._native = NativeMel(self.device.index or 0, sr, pad_mode)

    def _wave(self, y):
        import torch
        t = y if torch.is_tensor(y) else torch.as_tensor(np.asarray(y))
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2:
            raise ValueError(f"waveforms must be [B, N] or [N], got {tuple(t.shape)}")
        return t.to(self.device, torch.float32).contiguous()

    def power(self, y, lengths=None):
        """-> [B, F, 128], F = 1 + N // 256: ``librosa.feature.melspectrogram(..).T`` per clip; rows behind a clip's own frames are 0."""
        return self._native.power(self._wave(y), lengths)

    def features(self, y, lengths=None, mel_len_90fps=None):
        """-> [B, Tm, 128]: ``extract_mel_feature`` per clip.  `mel_len_90fps`: None (each clip's ``int(n / sr * 90)``), one int for
        all clips, or one per clip; Tm is the largest, rows behind a clip's own length are 0."""
        w = self._wave(y)
        tm = mel_len_90fps
        if tm is not None and np.ndim(tm) == 0:
            tm = [int(tm)] * int(w.shape[0])
        return self._native.features(w, lengths, tm)


def extract_mel_feature(audio, mel_len_90fps=None, sr=None, device="cuda:0", pad_mode="constant"):
    """The reference's ``extract_mel_feature(audio_file, mel_len_90fps=None)``: `audio` is the path of a WAV file (loaded at 22050 Hz
    unless `sr` says otherwise, ``load_audio``) or a 1-D array sampled at `sr` (22050 when None).  As in the reference only the first
    60 s are used.  -> numpy fp32 [Tm, 128], what the dataset stores as ``mel.npy``."""
    if isinstance(audio, (str, os.PathLike)):
        y, rate = load_audio(audio, 22050 if sr is None else sr)
    else:
        y, rate = np.asarray(audio, np.float32).reshape(-1), 22050 if sr is None else int(sr)
    y = y[:rate * 60]
    return MelSpectrogram(device, rate, pad_mode).features(y, None, mel_len_90fps)[0].cpu().numpy()
