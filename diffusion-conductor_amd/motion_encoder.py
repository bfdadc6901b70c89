"""M2SNet's ST-GCN motion encoder, the latent space of the evaluation metrics (metrics.py).

``MotionEncoder_STGCN`` is a drop-in for the reference's class of the same name (Diffusion_Stage/trainers/ddpm_trainer.py:27-63,
repeated in tools/eval_new_metrics.py and tools/eval_old_metrics.py) in eval mode, over the HIP kernels of csrc/dc_stgcn.hip
(dc_motion_encoder_* in include/dc_ddim.h).  ``load_m2snet`` is MotionPretrain (ddpm_trainer.py:66-80) without its hard-coded
checkpoint path.  There is no CPU path: encoding needs the MI355X.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

M2SNET_PREFIX = "module.motion_encoder."
N_JOINTS, N_BLOCKS, LATENT = 13, 10, 64


def motion_encoder_shapes():
    """name -> shape of every state_dict entry of MotionEncoder_STGCN (165 entries, in the reference module's order)."""
    e = OrderedDict()

    def bn(p, n):
        for s in ("weight", "bias", "running_mean", "running_var"):
            e[p + s] = (n,)
        e[p + "num_batches_tracked"] = ()

    e["st_gcn.A"] = (1, N_JOINTS, N_JOINTS)
    bn("st_gcn.data_bn.", 2 * N_JOINTS)
    for i in range(N_BLOCKS):
        p = f"st_gcn.st_gcn_networks.{i}."
        cin = 2 if i == 0 else 32
        e[p + "gcn.conv.weight"] = (32, cin, 1, 1)
        e[p + "gcn.conv.bias"] = (32,)
        bn(p + "tcn.0.", 32)
        e[p + "tcn.2.weight"] = (32, 32, 3, 1)
        e[p + "tcn.2.bias"] = (32,)
        bn(p + "tcn.3.", 32)
    for i in range(N_BLOCKS):
        e[f"st_gcn.edge_importance.{i}"] = (1, N_JOINTS, N_JOINTS)
    e["st_gcn.fcn.weight"] = (32, 256, 1, 1)
    e["st_gcn.fcn.bias"] = (32,)
    e["fc.0.weight"] = (LATENT, 32 * N_JOINTS, 1)
    e["fc.0.bias"] = (LATENT,)
    bn("fc.1.", LATENT)
    return e


# the ConductorMotionX skeleton of models/ST_GCN/st_gcn_utils/graph.py: 13 joints (nose, eyes, ears, shoulders, elbows, wrists,
# hips), self links plus these bones
SKELETON_EDGES = ((0, 1), (0, 2), (1, 3), (2, 4), (0, 5), (0, 6), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (11, 12), (5, 11),
                  (6, 12))


def skeleton_adjacency():
    """The graph's `uniform`-strategy A [1, 13, 13]: the hop <= 1 adjacency (self links included) with every column divided by its
    sum, A[v, w] = adj[v, w] / deg(w)."""
    adj = np.eye(N_JOINTS)
    for i, j in SKELETON_EDGES:
        adj[i, j] = adj[j, i] = 1.0
    return (adj / adj.sum(0, keepdims=True))[None].astype(np.float32)


def strip_m2snet_prefix(state_dict):
    """MotionPretrain's key filter (ddpm_trainer.py:74-77): the entries under `module.motion_encoder.`, prefix removed."""
    return OrderedDict((k[len(M2SNET_PREFIX):], v) for k, v in state_dict.items() if k.startswith(M2SNET_PREFIX))


def _to_numpy(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


class MotionEncoder_STGCN:  # noqa: N801  (the reference's class name)
    """Eval-mode MotionEncoder_STGCN on the MI355X.  ``latent(x)`` is the reference's ``features(x)[-1]``, [B, 64, T]; ``forward(x)``
    its ``forward(x)``, [B, T, 64].  Inputs are fp32 motions [B, T, 13, 2] (or [B, T, 26]) as torch tensors or arrays; results
    are device tensors."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        self._native = None

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics for the keys: with strict=True a missing or unexpected key raises RuntimeError (the
        reference loads with strict=True).  Every shape is checked."""
        from .native import NativeMotionEncoder
        spec = motion_encoder_shapes()
        missing = [k for k in spec if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for MotionEncoder_STGCN: missing keys {missing}, "
                               f"unexpected keys {unexpected}")
        for k, v in state_dict.items():
            if k in spec and tuple(np.shape(_to_numpy(v))) != spec[k]:
                raise RuntimeError(f"size mismatch for {k}: got {tuple(np.shape(_to_numpy(v)))}, expected {spec[k]}")
        enc = NativeMotionEncoder(self.device.index or 0)
        for k, v in state_dict.items():
            if k in spec:
                enc.set_param(k, _to_numpy(v).astype(np.float32))
        enc.finalize()
        if self._native is not None:
            self._native.close()
        self._native = enc
        return self

    def eval(self):
        return self

    def to(self, device):
        import torch
        if torch.device(device) != self.device and self._native is not None:
            raise RuntimeError("move the encoder before load_state_dict (its weights live on the device it was loaded on)")
        self.device = torch.device(device)
        return self

    def _input(self, x):
        import torch
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        if t.dim() == 3 and t.shape[-1] == 2 * N_JOINTS:
            t = t.reshape(t.shape[0], t.shape[1], N_JOINTS, 2)
        if t.dim() != 4 or tuple(t.shape[2:]) != (N_JOINTS, 2):
            raise ValueError(f"motion must be [B, T, 13, 2] or [B, T, 26], got {tuple(t.shape)}")
        return t.to(self.device, torch.float32).contiguous()

    def latent(self, x, out=None):
        """features(x)[-1]: [B, 64, T] fp32 on the device (enqueued on the current stream)."""
        if self._native is None:
            raise RuntimeError("MotionEncoder_STGCN: load_state_dict first")
        return self._native.encode(self._input(x), out=out)

    def forward(self, x):
        """The reference's forward: [B, T, 64]."""
        return self.latent(x).transpose(1, 2)

    __call__ = forward

    def features(self, x):
        raise NotImplementedError("MotionEncoder_STGCN.features: only the last entry (the latent, `latent()`) is provided; the "
                                  "intermediate feature maps serve the training feature loss, which this package does not run")


def load_m2snet(path, device="cuda:0"):
    """MotionPretrain (ddpm_trainer.py:66-80): an M2SNet checkpoint (a DataParallel state_dict) -> a loaded MotionEncoder_STGCN."""
    import torch
    sd = torch.load(path, map_location="cpu")
    return MotionEncoder_STGCN(device).load_state_dict(strip_m2snet_prefix(sd), strict=True)
