#!/usr/bin/env python3
"""CPU only: the factor A of tests/test_gpu_solver.py's order-2 bound for the fp16 / bf16 precisions (1e-3 A).  How much more of an
evaluation's error does the second-order multistep update carry to the final sample than DDIM does on the same list?  Measured in the
fp64 oracle alone (tests/helpers_solver.py), never in the library: every evaluation's output is perturbed by seeded relative noise of
1e-4, and the final sample's deviation from the unperturbed run is compared between order 2 and order 1 - per shape of the GPU test
(at most three clips of the wide ones) and per spacing, n = 25 timesteps of the 1000-step schedule.  A = the largest ratio, floored at
1 and rounded up to one digit.   usage: python tools/solver_amplification.py [out.txt]"""
import math
import os
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
from helpers import batch_noise, oracle_params, rel_l2, xf_pair  # noqa: E402
from helpers_solver import solver_loop  # noqa: E402
from diffusion_conductor_amd.sampler import get_named_beta_schedule, spaced_timesteps  # noqa: E402
import numpy as np  # noqa: E402

torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
S, N, REL = 1000, 25, 1e-4
# name -> (B, T, lengths, full attention, guidance scale): the caller shapes of tests/test_gpu_solver.py (the precision is the library's)
SHAPES = {"layer16": (1, 256, None, False, None), "narrow": (36, 256, None, False, None), "wide_aligned": (80, 256, None, False, None),
          "wide_flat": (55, 300, None, False, None), "group_96": (2, 96, [96, 70], False, None), "no_eff": (2, 96, [96, 70], True, None),
          "guided": (1, 256, None, False, 2.0)}
ac = np.cumprod(1.0 - get_named_beta_schedule("linear", S))
p = oracle_params(torch.float64)
lines, worst = [], 1.0
for name, (B, T, length, no_eff, w) in SHAPES.items():
    clips = [2, 3, B - 1 if (B - 1) % 4 != 1 else B - 3] if B > 3 else list(range(B))
    c = torch.tensor(clips)
    xfp, xfo = xf_pair(B, T, first=60)
    x = torch.from_numpy(batch_noise(B, T, first=60))[c].double()
    xfp, xfo = xfp[c].double(), xfo[c].double()
    ln = [(length or [T] * B)[i] for i in clips]
    for spacing in ("uniform", "logsnr"):
        ts = spaced_timesteps(ac, N, spacing)
        dev = {}
        for order in (1, 2):
            clean = solver_loop(p, x, xfp, xfo, ln, S, ts, order, w=w, no_eff=no_eff)
            noisy = solver_loop(p, x, xfp, xfo, ln, S, ts, order, w=w, no_eff=no_eff, perturb=(1234, REL))
            dev[order] = rel_l2(noisy, clean)
        ratio = dev[2] / dev[1]
        worst = max(worst, ratio)
        lines.append(f"{name:13s} {spacing:8s} n={len(ts):2d}  deviation order 1 {dev[1]:.3e}  order 2 {dev[2]:.3e}  ratio {ratio:.3f}")
        print(lines[-1], flush=True)
mag = 10 ** math.floor(math.log10(worst))
A = math.ceil(worst / mag - 1e-12) * mag
lines.append(f"largest ratio {worst:.3f} -> A = {A:g}")
print(lines[-1])
if len(sys.argv) > 1:
    open(sys.argv[1], "w").write("\n".join(lines) + "\n")
