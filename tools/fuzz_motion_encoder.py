#!/usr/bin/env python3
"""GPU box: randomized (B, T, weight variant) cases of the ST-GCN motion encoder (csrc/dc_stgcn.hip, `MotionEncoder_STGCN.latent`)
against the fp64 oracle (oracle/stgcn_oracle.py) - batches biased to the 64-clip chunk edges, lengths biased to the 30-frame tile
and 32-frame wave edges, weights from synthetic.motion_encoder_weight_variant.  Bounds as tests/test_gpu_motion_encoder_edges.py:
rel-L2 per clip and per frame.  Test infrastructure: the oracle is the checker.  usage: python tools/fuzz_motion_encoder.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from oracle.stgcn_oracle import motion_encoder_latent  # noqa: E402

from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN  # noqa: E402
from diffusion_conductor_amd.synthetic import MOTION_ENCODER_VARIANTS, motion_encoder_weight_variant, synthetic_motion  # noqa: E402

torch.set_num_threads(min(16, os.cpu_count() or 1))
N = int(sys.argv[1]) if len(sys.argv) > 1 else 60
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
CLIP_TOL, FRAME_TOL = 2e-6, 5e-6
MAX_FRAMES = 16000          # B * T cap: the fp64 oracle takes 1 - 2 s per 16k clip-frames on 16 threads


def pick_b():
    k = rng.integers(0, 3)
    return int(rng.integers(63, 67)) if k == 0 else int(rng.integers(127, 131)) if k == 1 else int(rng.integers(1, 141))


def pick_t():
    k = rng.integers(0, 3)
    if k == 0:
        return int(30 * rng.integers(1, 67) + rng.integers(-1, 3))
    if k == 1:
        return int(32 * rng.integers(1, 63) + rng.choice([-1, 1]))
    return int(rng.integers(1, 2001))


encs, bad, worst, t0 = {}, 0, [0.0, 0.0], time.perf_counter()
for case in range(N):
    B, T = pick_b(), pick_t()
    if B * T > MAX_FRAMES:
        B = max(1, MAX_FRAMES // T)
    kind = str(rng.choice(MOTION_ENCODER_VARIANTS))
    if kind not in encs:
        sd = motion_encoder_weight_variant(kind, seed=3)
        encs[kind] = (sd, MotionEncoder_STGCN("cuda:0").load_state_dict(sd, strict=True))
    sd, enc = encs[kind]
    m = synthetic_motion(B, T, seed=int(rng.integers(0, 1 << 30)))
    hip = enc.latent(torch.from_numpy(m)).cpu().double().numpy()
    ref = motion_encoder_latent(sd, m).numpy()
    d = hip - ref
    ec = float((np.linalg.norm(d.reshape(B, -1), axis=1) / np.linalg.norm(ref.reshape(B, -1), axis=1)).max())
    ef = float((np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-30)).max())
    ok = bool(np.isfinite(hip).all()) and ec <= CLIP_TOL and ef <= FRAME_TOL
    bad += not ok
    worst = [max(worst[0], ec), max(worst[1], ef)]
    print(f"case {case:3d} B={B:3d} T={T:4d} {kind:17s}: clip {ec:.2e} frame {ef:.2e}{'' if ok else '   <-- FAIL'}", flush=True)
print(f"{N} cases, {bad} failures, {time.perf_counter() - t0:.0f} s; worst clip {worst[0]:.2e}, worst frame {worst[1]:.2e}")
sys.exit(1 if bad else 0)
