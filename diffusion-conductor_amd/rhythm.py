"""What the rhythm and realism scores of the reference's M2S-GAN evaluation read off a motion, on the MI355X.

``MotionRhythm`` computes, per clip, the three small arrays those scores are made of (csrc/dc_rhythm.hip, dc_rhythm_* in
include/dc_ddim.h):

* ``psd(x)``      bins 0 .. 31 of the Welch power spectrum averaged over the 26 pose channels - scipy.signal.welch(x, 30) with its
                  defaults, as rhythm_density_error calls it (Contrastive_Stage/utils/loss.py:173-186);
* ``contour(x)``  the average-pooled speed contour of strengh_contour_error (loss.py:129-142);
* ``std(x)``      the mean over the channels of the standard deviation over time (Contrastive_Stage/M2SGAN_eval.py:101-102).

The scores themselves - RDE, SCE, the W-distance - are host numpy over these arrays: metrics.rhythm_density_error,
metrics.strength_contour_error, metrics.w_distance.  There is no CPU path for them.

Beat consistency (BC) comes from two more calls, with the music's beats as an input (librosa's tracker, get_music_beat, is a function
of the mel alone and stays outside the project: tools/music_beats_librosa.py, metrics.load_music_beats):

* ``motion_beats(x)``  motion_peak_onehot (Diffusion_Stage/tools/eval_new_metrics.py:285-309): the strict minima over +-10 frames of
                       the summed joint speed, the envelope with the reference's float32 bits;
* ``beat_scores(motion_beats, music_beats)``  alignment_score (:253-275): BC, and Beat Align, the direction the reference keeps
                       commented out.

metrics.motion_beats_host and metrics.beat_alignment_host restate the two in numpy for a box without a GPU.
"""
from __future__ import annotations

import numpy as np

POSE = 26


class MotionRhythm:
    """x: fp32 motions [B, T, 26] or [B, T, 13, 2], torch tensors (on the device or on the host) or arrays; results are device
    tensors.  psd needs T >= 256, contour and std T >= 60 (ValueError otherwise)."""

    def __init__(self, device="cuda:0"):
        import torch
        from .native import NativeRhythm
        self.device = torch.device(device)
        self._native = NativeRhythm(self.device.index or 0)

    def _motion(self, x):
        import torch
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        if t.dim() not in (3, 4) or t.numel() != t.shape[0] * t.shape[1] * POSE:
            raise ValueError(f"motion must be [B, T, 26] or [B, T, 13, 2], got {tuple(t.shape)}")
        return t.to(self.device, torch.float32).contiguous()

    def psd(self, x):
        """-> [B, 32]: bins 0 .. 31 (0 .. 3.63 Hz at fs = 30) of PSD.sum(channels) / 26."""
        return self._native.psd(self._motion(x))

    def contour(self, x):
        """-> [B, W], W = (T - 60) // 30 + 1."""
        return self._native.contour(self._motion(x), sd=False)[0]

    def std(self, x):
        """-> [B]."""
        return self._native.contour(self._motion(x), contour=False)[1]

    def contour_and_std(self, x):
        """Both from one call: ([B, W], [B])."""
        return self._native.contour(self._motion(x))

    def _onehot(self, a, what):
        import torch
        t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
        if t.dim() == 1:
            t = t.unsqueeze(0)
        if t.dim() != 2 or t.shape[1] < 1:
            raise ValueError(f"{what} must be one-hots [B, L], got {tuple(t.shape)}")
        return (t != 0).to(self.device, torch.uint8).contiguous()

    def motion_beats(self, x, length=None, order=10, envelope=False):
        """-> beats uint8 [B, T] (1 = a motion beat), or (beats, envelope fp32 [B, T]) with `envelope`.  `length`: None or the clips'
        frame counts (frames behind a clip's length are 0 and are not looked at); `order`: 1 .. 64, the reference's is 10."""
        beats, env = self._native.motion_beats(self._motion(x), length, order, envelope)
        return (beats, env) if envelope else beats

    def beat_scores(self, motion_beats, music_beats, music_stride=1, sigma=3.0, counts=False):
        """one-hots [B, T] and [B, Lm] (nonzero = a beat; tensors or arrays) -> fp32 [B, 2]: BC and Beat Align per clip (dc_ddim.h for
        the empty cases).  music_stride = 1 compares the two index lists as they are, as the reference does; 3 puts 90-fps music
        frames and 30-fps motion frames on one clock.  `counts`: also int32 [B, 2], the number of music and of motion beats."""
        scores, n = self._native.beat_scores(self._onehot(motion_beats, "motion_beats"), self._onehot(music_beats, "music_beats"),
                                             music_stride, sigma)
        return (scores, n) if counts else scores
