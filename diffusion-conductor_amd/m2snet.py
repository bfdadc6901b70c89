"""M2SNet, the reference's learned music-motion synchronisation discriminator, as an evaluation score.

``M2SNet`` is a drop-in for the reference's class of the same name (Contrastive_Stage/models/M2SNet.py:7-41) in eval mode:
``forward(mel, motion)`` is, for every motion frame, the probability that the motion is in sync with the music - the quantity
Contrastive_Stage/M2SNet_eval.py:58-107 averages over matched and mismatched pairs (metrics.sync_stats).  Its MusicEncoder
(models/MusicEncoder.py:30-53) runs on the kernels of csrc/dc_music.hip with M2SNet's OWN ``music_encoder.*`` weights (not the
diffusion checkpoint's), its MotionEncoder_STGCN on csrc/dc_stgcn.hip, the fuse head on csrc/dc_m2snet.hip (dc_m2snet_* in
include/dc_ddim.h).  There is no CPU path: scoring needs the MI355X.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from .motion_encoder import N_JOINTS, _to_numpy, motion_encoder_shapes

MODULE_PREFIX = "module."          # the checkpoint is a DataParallel state_dict (M2SNet_eval.py:109 `.module`)
LATENT = 64


def m2snet_shapes():
    """name -> shape of every state_dict entry of M2SNet (234 entries, in the reference module's order: music_encoder, motion_encoder,
    fuse_layer)."""
    from .param_spec import param_shapes
    e = OrderedDict((k, v) for k, v in param_shapes().items() if k.startswith("music_encoder."))
    for k, v in motion_encoder_shapes().items():
        e["motion_encoder." + k] = v
    for i, (cout, cin) in ((0, (LATENT, 2 * LATENT)), (2, (LATENT, LATENT)), (4, (1, LATENT))):
        e[f"fuse_layer.{i}.weight"] = (cout, cin, 1)
        e[f"fuse_layer.{i}.bias"] = (cout,)
    return e


def strip_module_prefix(state_dict):
    """The DataParallel prefix removed from every key that has it."""
    return OrderedDict((k[len(MODULE_PREFIX):] if k.startswith(MODULE_PREFIX) else k, v) for k, v in state_dict.items())


class M2SNet:
    """Eval-mode M2SNet on the MI355X.  mel: fp32 [B, Tm, 128]; motion: fp32 [B, T, 13, 2] or [B, T, 26] with T = (Tm-1)//3+1;
    torch tensors or arrays.  Results are device tensors."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        self._native = None
        self._motion_sd, self._motion = None, None

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics for the keys: with strict=True a missing or unexpected key raises RuntimeError.  Every
        shape is checked."""
        from .native import NativeM2SNet
        spec = m2snet_shapes()
        missing = [k for k in spec if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for M2SNet: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in state_dict.items():
            if k in spec and tuple(np.shape(_to_numpy(v))) != spec[k]:
                raise RuntimeError(f"size mismatch for {k}: got {tuple(np.shape(_to_numpy(v)))}, expected {spec[k]}")
        net = NativeM2SNet(self.device.index or 0)
        for k, v in state_dict.items():
            if k in spec:
                net.set_param(k, _to_numpy(v).astype(np.float32))
        net.finalize()
        if self._native is not None:
            self._native.close()
        self._native = net
        pre = "motion_encoder."
        self._motion_sd = {k[len(pre):]: _to_numpy(v) for k, v in state_dict.items() if k in spec and k.startswith(pre)}
        self._motion = None
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
            raise RuntimeError("M2SNet: load_state_dict first")
        return self._native

    def _tensor(self, x):
        import torch
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        return t.to(self.device, torch.float32).contiguous()

    def _motion_input(self, x):
        t = self._tensor(x)
        if t.dim() == 3 and t.shape[-1] == 2 * N_JOINTS:
            t = t.reshape(t.shape[0], t.shape[1], N_JOINTS, 2)
        if t.dim() != 4 or tuple(t.shape[2:]) != (N_JOINTS, 2):
            raise ValueError(f"motion must be [B, T, 13, 2] or [B, T, 26], got {tuple(t.shape)}")
        return t

    def _mel(self, x):
        t = self._tensor(x)
        if t.dim() != 3 or t.shape[2] != 128:
            raise ValueError(f"mel must be [B, Tm, 128], got {tuple(t.shape)}")
        return t

    def music_latent(self, mel, out=None):
        """music_encoder(mel): [B, T, 64] fp32 on the device (enqueued on the current stream)."""
        return self._net().encode_music(self._mel(mel), out=out)

    def motion_latent(self, motion, out=None):
        """motion_encoder.features(motion)[-1]: [B, 64, T] fp32 on the device, for `fuse`.  (A MotionEncoder_STGCN of this model's
        `motion_encoder.*` entries, created on first use: the library's handle keeps its own for `forward`.)"""
        self._net()
        if self._motion is None:
            from .motion_encoder import MotionEncoder_STGCN
            self._motion = MotionEncoder_STGCN(self.device).load_state_dict(self._motion_sd, strict=False)
        return self._motion.latent(self._motion_input(motion), out=out)

    def fuse(self, music_latent, motion_latent, return_logits=False):
        """The fuse head on latents the caller holds - music [B, T, 64] (music_latent()) and motion [B, 64, T]
        (MotionEncoder_STGCN.latent()): the probabilities [B, T], or (probabilities, logits) with `return_logits`.  Evaluation
        encodes a piece once and scores it against several motions."""
        return self._net().fuse(self._tensor(music_latent), self._tensor(motion_latent), logits=return_logits)

    def fuse_pairs(self, music_latent, motion_latent, len_music=None, len_motion=None, return_frames=False):
        """The fuse head on EVERY pair of `music_latent` [Bm, T, 64] and `motion_latent` [Bn, 64, T], without the Bm x Bn
        concatenation (M2SNet.py:31-36 per pair, reduced as M2SNet_eval.py:58-68 reduces a batch): a dict of device tensors [Bm, Bn] -
        "mean" (fp32, the mean probability over the pair's valid frames), "sum" (fp32), "above" and "below" (int32, the valid frames
        with p > 0.5 and with p < 0.5) and "count" (int32, the valid frames: min(len_music[i], len_motion[j]); a length of None is T) -
        and, with `return_frames`, "prob" [Bm, Bn, T], every frame's probability, bit-identical to `fuse` on that pair.  A pair's
        numbers do not depend on the other pairs of the call.  Runs on the current stream, like `fuse`."""
        import torch
        mus, mot = self._tensor(music_latent), self._tensor(motion_latent)
        total, above, below, prob = self._net().fuse_pairs(mus, mot, len_music, len_motion, frames=return_frames)
        T = int(mus.shape[1])
        lm, ln = (np.full(n, T, np.int32) if a is None else np.asarray(a, np.int32) for a, n in ((len_music, mus.shape[0]), (len_motion, mot.shape[0])))
        count = torch.from_numpy(np.minimum(lm[:, None], ln[None, :])).to(self.device)
        out = {"mean": total / count.to(torch.float32), "sum": total, "above": above, "below": below, "count": count}
        if return_frames:
            out["prob"] = prob
        return out

    def logits(self, mel, motion):
        """The value in front of the sigmoid, [B, T]."""
        return self._net().score(self._mel(mel), self._motion_input(motion), logits=True)[1]

    def forward(self, mel, motion):
        """The reference's forward: [B, T, 1], the per-frame probability that `motion` is in sync with `mel`."""
        return self._net().score(self._mel(mel), self._motion_input(motion)).unsqueeze(2)

    __call__ = forward

    def features(self, mel, motion):
        raise NotImplementedError("M2SNet.features: only the latents (`music_latent()`, MotionEncoder_STGCN.latent()) are provided; the "
                                  "intermediate feature maps serve the training feature loss, which this package does not run")


def load_m2snet_full(path, device="cuda:0"):
    """An M2SNet checkpoint (a DataParallel state_dict, Contrastive_Stage/M2SNet_eval.py:118-119) -> a loaded M2SNet, every entry
    used (motion_encoder.load_m2snet keeps the motion encoder alone)."""
    import torch
    sd = torch.load(path, map_location="cpu")
    return M2SNet(device).load_state_dict(strip_module_prefix(sd), strict=True)
