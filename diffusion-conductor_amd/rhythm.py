"""What the rhythm and realism scores of the reference's M2S-GAN evaluation read off a motion, on the MI355X.

``MotionRhythm`` computes, per clip, the three small arrays those scores are made of (csrc/dc_rhythm.hip, dc_rhythm_* in
include/dc_ddim.h):

* ``psd(x)``      bins 0 .. 31 of the Welch power spectrum averaged over the 26 pose channels - scipy.signal.welch(x, 30) with its
                  defaults, as rhythm_density_error calls it (Contrastive_Stage/utils/loss.py:173-186);
* ``contour(x)``  the average-pooled speed contour of strengh_contour_error (loss.py:129-142);
* ``std(x)``      the mean over the channels of the standard deviation over time (Contrastive_Stage/M2SGAN_eval.py:101-102).

The scores themselves - RDE, SCE, the W-distance - are host numpy over these arrays: metrics.rhythm_density_error,
metrics.strength_contour_error, metrics.w_distance.  There is no CPU path.
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
