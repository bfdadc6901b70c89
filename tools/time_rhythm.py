#!/usr/bin/env python3
"""Time the rhythm and realism scores on the MI355X with device events.

Run:  python tools/time_rhythm.py [--B 32] [--T 1800] [--iters 20] [--rounds 5]

At [B, T] (default 32 clips of 60 s) it times, after a warm-up of every shape, `iters` back-to-back calls between two events,
`rounds` times, the parts taken in turn within a round, and prints the median, minimum and maximum per call in milliseconds:
  psd                  MotionRhythm.psd of one motion batch (2 launches per 64 clips)
  contour              MotionRhythm.contour_and_std of one motion batch (2 launches per 64 clips)
  score                Discriminator_1DCNN.forward of one motion batch (5 launches per 32 clips)
  generate             Generator.forward alone: the call the scores ride behind in an evaluation of the baseline
  generate + 3         Generator.forward, then psd, contour_and_std and score of the generated batch
  generate + scores    Generator.forward, then psd, contour_and_std and score of BOTH the generated and the real batch - what
                       evaluate_dataset(rhythm=, discriminator=) enqueues per batch
and beside `score` its algorithmic FLOPs.  One JSON line at the end repeats the medians.
These are times per call as Python enqueues them: where a call is two launches of a few microseconds (psd, contour) the figure is
bounded below by the host's enqueue rate and is an upper bound of the kernels' own time."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def critic_flops(T):
    """2 x MACs of one clip: three convolutions at their conv lengths and the per-frame fc."""
    L1 = (T - 5) // 3 + 1
    L2 = (L1 - 5) // 2 + 1
    L3 = (L2 - 5) // 2 + 1
    return 2 * (64 * 5 * 26 * T + 64 * 5 * 64 * (L1 + L2) + (64 * 32 + 32 * 32 + 32) * L3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1800)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd.discriminator import Discriminator_1DCNN
    from diffusion_conductor_amd.generator import Generator
    from diffusion_conductor_amd.rhythm import MotionRhythm
    from diffusion_conductor_amd.synthetic import (batch_mel, synthetic_discriminator_state_dict, synthetic_m2sgan_state_dict,
                                                   synthetic_motion)
    dev = torch.device("cuda:0")
    B, T = a.B, a.T
    assert T % 30 == 0 and T >= 256, "the generator needs T = 30 Ln, Welch T >= 256"
    real = torch.from_numpy(synthetic_motion(B, T, seed=31) + np.float32(0.5)).to(dev).reshape(B, T, 26)
    mel = torch.from_numpy(batch_mel(B, 3 * T)).to(dev)
    z = torch.randn(B, T // 30, 8, generator=torch.Generator().manual_seed(0)).to(dev)
    gen = Generator(dev).load_state_dict(synthetic_m2sgan_state_dict())
    rh = MotionRhythm(dev)
    critic = Discriminator_1DCNN(dev).load_state_dict(synthetic_discriminator_state_dict())

    def scores(x):
        rh.psd(x)
        rh.contour_and_std(x)
        critic(x)

    def three_behind_generate():
        scores(gen(mel, z).reshape(B, T, 26))

    def behind_generate():
        fake = gen(mel, z).reshape(B, T, 26)
        scores(fake)
        scores(real)
    parts = [("psd", lambda: rh.psd(real)), ("contour", lambda: rh.contour_and_std(real)), ("score", lambda: critic(real)),
             ("generate", lambda: gen(mel, z)), ("generate + 3", three_behind_generate), ("generate + scores", behind_generate)]
    for _, fn in parts:                           # warm-up: code objects, workspaces
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in parts}
    for _ in range(a.rounds):
        for name, fn in parts:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.iters)
    print(f"B={B} T={T}: ms per call over {a.rounds} rounds of {a.iters} calls")
    for name, v in ms.items():
        print(f"  {name:20s} median {np.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}")
    sc = float(np.median(ms["score"])) * 1e-3
    gflop = critic_flops(T) * B / 1e9
    print(f"  score: {gflop:.2f} GFLOP -> {gflop / sc / 1e3:.2f} TFLOP/s exact fp32")
    print(f"  the six score calls add {np.median(ms['generate + scores']) - np.median(ms['generate']):.3f} ms to a generate of "
          f"{np.median(ms['generate']):.3f} ms")
    print(json.dumps({"B": B, "T": T, "score_gflop": round(gflop, 3), **{k: round(float(np.median(v)), 4) for k, v in ms.items()}}))


if __name__ == "__main__":
    main()
