"""CPU ORACLE for the ST-GCN motion encoder (csrc/dc_stgcn.hip).  TEST INFRASTRUCTURE ONLY.

Only ``tests/`` and ``tools/`` may import this file.  The product path (diffusion-conductor_amd/) never does: encoding needs the
HIP library, and there is no CPU fallback.

What this is: a plain functional restatement, in PyTorch CPU ops on a dict of named tensors, of the reference's eval-mode
``MotionEncoder_STGCN.features(x)[-1]`` (paths relative to the reference's Diffusion_Stage):
  trainers/ddpm_trainer.py:27-63        the encoder: input permutes, st_gcn, channel flatten c*13 + v, fc = Conv1d + BatchNorm1d
  models/ST_GCN/ST_GCN.py:96-106        data_bn over the 26 channels v*2 + c, then the blocks with A * edge_importance[l]
  models/ST_GCN/ST_GCN.py:183-226       st_gcn: tcn = BN, ReLU, Conv (3, 1) with zero padding 1, BN; residual none in block 0,
                                        identity after; out = relu(tcn(gcn(x)) + res)
  models/ST_GCN/st_gcn_utils/tgcn.py:57-66   gcn: the 1x1 conv, then the joint mix  y[n, c, t, w] = sum_v y[n, c, t, v] Ahat[v, w]

It is deliberately NOT the kernel's arithmetic: every BatchNorm is applied unfolded after its conv as (x - mean) g / sqrt(var + eps)
+ b, the 1x1 conv runs before the joint mix (the kernel folds the BatchNorms at finalize and mixes first), and zero entries of Ahat
are multiplied through (the kernel skips them).  fp64 by default, so that the kernel's fp32 rounding is the only difference; fp32
on request, which reproduces the reference's own rounding order closely (tests/test_motion_metrics_host.py pins both against
tests/golden/g12_motion_metrics.npz).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

N_JOINTS, N_BLOCKS, EPS = 13, 10, 1e-5


def _t(v, dtype):
    return (v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(dtype)


def _bn(x, sd, prefix, dtype):
    """Eval-mode BatchNorm over dim 1, unfolded: (x - running_mean) weight / sqrt(running_var + eps) + bias."""
    shape = (1, -1) + (1,) * (x.dim() - 2)
    m, v = _t(sd[prefix + "running_mean"], dtype).view(shape), _t(sd[prefix + "running_var"], dtype).view(shape)
    g, b = _t(sd[prefix + "weight"], dtype).view(shape), _t(sd[prefix + "bias"], dtype).view(shape)
    return (x - m) * g / torch.sqrt(v + EPS) + b


def motion_encoder_latent(sd, motion, dtype=torch.float64):
    """features(x)[-1] of the eval-mode encoder: motion [B, T, 13, 2] (or [B, T, 26]) -> latent [B, 64, T] in `dtype`.
    `sd`: name -> array or tensor, the state_dict entries of motion_encoder.motion_encoder_shapes()."""
    x = _t(motion, dtype)
    B, T = x.shape[0], x.shape[1]
    x = x.reshape(B, T, N_JOINTS * 2).transpose(1, 2)                     # [B, 26, T], channel v*2 + c
    x = _bn(x, sd, "st_gcn.data_bn.", dtype)
    x = x.reshape(B, N_JOINTS, 2, T).permute(0, 2, 3, 1)                 # [B, C = 2, T, V]
    A = _t(sd["st_gcn.A"], dtype)[0]
    for l in range(N_BLOCKS):
        p = f"st_gcn.st_gcn_networks.{l}."
        ahat = A * _t(sd[f"st_gcn.edge_importance.{l}"], dtype)[0]     # [v, w]
        res = x if l > 0 else 0
        y = F.conv2d(x, _t(sd[p + "gcn.conv.weight"], dtype), _t(sd[p + "gcn.conv.bias"], dtype))
        y = torch.einsum("nctv,vw->nctw", y, ahat)
        y = torch.relu(_bn(y, sd, p + "tcn.0.", dtype))
        y = F.conv2d(y, _t(sd[p + "tcn.2.weight"], dtype), _t(sd[p + "tcn.2.bias"], dtype), padding=(1, 0))
        x = torch.relu(_bn(y, sd, p + "tcn.3.", dtype) + res)
    x = x.permute(0, 2, 1, 3).reshape(B, T, -1).transpose(1, 2)         # [B, 416, T], channel c*13 + v
    x = F.conv1d(x, _t(sd["fc.0.weight"], dtype), _t(sd["fc.0.bias"], dtype))
    return _bn(x, sd, "fc.1.", dtype)
