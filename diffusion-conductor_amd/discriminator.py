"""The M2S-GAN critic, whose D(real) - D(fake) is the W-distance of the reference's evaluation.

``Discriminator_1DCNN`` is a drop-in for the reference's class of the same name (Contrastive_Stage/models/Discriminator.py:5-41)
in eval mode: ``forward(x)`` maps motions [B, T, 13, 2] to one score per clip [B, 1], ``features(x)`` returns the one-element list
with the encoder's output [B, 64, L3].  Three Conv1d(kernel 5) + ReLU + MaxPool1d(5, stride 3 / 2 / 2) stages and the per-frame fc
run on csrc/dc_rhythm.hip (dc_discriminator_* in include/dc_ddim.h).  Scoring only: no gradient penalty, no training.  There is no
CPU path.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from .m2snet import strip_module_prefix
from .motion_encoder import _to_numpy

CHANNELS, POSE, KERNEL, HIDDEN = 64, 26, 5, 32


def discriminator_shapes():
    """name -> shape of the 12 state_dict entries of the reference Discriminator_1DCNN (52 641 values), in the module's order."""
    e = OrderedDict()
    for i, cin in ((0, POSE), (3, CHANNELS), (6, CHANNELS)):
        e[f"motion_encoder.{i}.weight"], e[f"motion_encoder.{i}.bias"] = (CHANNELS, cin, KERNEL), (CHANNELS,)
    for i, (n, k) in ((0, (HIDDEN, CHANNELS)), (2, (HIDDEN, HIDDEN)), (4, (1, HIDDEN))):
        e[f"fc.{i}.weight"], e[f"fc.{i}.bias"] = (n, k), (n,)
    return e


class Discriminator_1DCNN:  # noqa: N801  (the reference's class name)
    """Eval-mode M2S-GAN critic on the MI355X.  x: fp32 motions [B, T, 13, 2] (or [B, T, 26]) with T >= 41, torch tensors or arrays;
    results are device tensors."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        self._native = None

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics for the keys: with strict=True a missing or unexpected key raises RuntimeError.  Every
        shape is checked.  A DataParallel `module.` prefix is accepted."""
        from .native import NativeDiscriminator
        state_dict = strip_module_prefix(state_dict)
        spec = discriminator_shapes()
        missing = [k for k in spec if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for Discriminator_1DCNN: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in state_dict.items():
            if k in spec and tuple(np.shape(_to_numpy(v))) != spec[k]:
                raise RuntimeError(f"size mismatch for {k}: got {tuple(np.shape(_to_numpy(v)))}, expected {spec[k]}")
        net = NativeDiscriminator(self.device.index or 0)
        for k, v in state_dict.items():
            if k in spec:
                net.set_param(k, _to_numpy(v).astype(np.float32))
        net.finalize()
        if self._native is not None:
            self._native.close()
        self._native = net
        return self

    def eval(self):
        return self

    def to(self, device):
        import torch
        if torch.device(device) != self.device and self._native is not None:
            raise RuntimeError("move the model before load_state_dict (its weights live on the device it was loaded on)")
        self.device = torch.device(device)
        return self

    def _net(self):
        if self._native is None:
            raise RuntimeError("Discriminator_1DCNN: load_state_dict first")
        return self._native

    def _motion(self, x):
        import torch
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        if t.dim() not in (3, 4) or t.numel() != t.shape[0] * t.shape[1] * POSE:
            raise ValueError(f"motion must be [B, T, 13, 2] or [B, T, 26], got {tuple(t.shape)}")
        return t.to(self.device, torch.float32).contiguous()

    def features(self, x):
        """Discriminator_1DCNN.features: [the encoder's output [B, 64, L3]]."""
        net = self._net()
        return [net.features(self._motion(x))]

    def forward(self, x):
        """The reference's forward: one score per clip, [B, 1]."""
        net = self._net()
        return net.score(self._motion(x)).unsqueeze(1)

    __call__ = forward


def load_m2sgan_discriminator(path, device="cuda:0"):
    """A critic checkpoint (the plain state_dict Contrastive_Stage/M2SGAN_eval.py:453 loads; a DataParallel `module.` prefix is
    stripped) -> a loaded Discriminator_1DCNN."""
    import torch
    sd = torch.load(path, map_location="cpu")
    return Discriminator_1DCNN(device).load_state_dict(sd, strict=True)
