#!/usr/bin/env python3
"""Time the M2S-GAN generator and its parts on the MI355X with device events ("M2S-GAN generator").

Run:  python tools/time_m2sgan.py [--B 32] [--Tm 5400] [--iters 20] [--rounds 5]

At [B, Tm] (default 32 clips of 60 s, T = 1800, a latent of 60 steps) it times, after a warm-up of every shape, `iters` back-to-back
calls between two events, `rounds` times, the parts taken in turn within a round, and prints the median, minimum and maximum per
call in milliseconds:
  m2snet music_latent   the MusicEncoder alone in the split format (M2SNet's: the same kernels, for comparison)
  features              Generator.features: music encoder + the noise branch's four launches
  decode                the six temporal blocks and the head on features the caller holds (13 launches per 32 clips)
  generate              Generator.forward end to end
and beside them the figures to read `decode` against: its algorithmic FLOPs (2 x 64 x (5 x 128 + 11 x 5 x 64 + 128 + 3 x 64 + 26)
per frame) and the activation bytes the 13 launches move through HBM / L2 by design.  One JSON line at the end repeats the medians."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LAUNCHES_DECODE, LAUNCHES_NOISE = 13, 4
FLOPS_PER_FRAME = 2 * 64 * (5 * 128 + 11 * 5 * 64 + 128 + 3 * 64 + 26)
# floats per frame the decode launches read and write by design: block 0 reads the 128-wide features (5 taps) and writes h and res;
# every other conv reads 5 x 64 and writes 64; conv2 reads the residual as well; the head reads 64 and writes 26
FLOATS_PER_FRAME = (5 * 128 + 128) + 11 * (5 * 64 + 64) + 6 * 64 + (64 + 26)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--Tm", type=int, default=5400)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd.generator import Generator
    from diffusion_conductor_amd.m2snet import M2SNet
    from diffusion_conductor_amd.synthetic import batch_mel, synthetic_m2sgan_state_dict, synthetic_m2snet_state_dict
    dev = torch.device("cuda:0")
    B, Tm, T = a.B, a.Tm, (a.Tm - 1) // 3 + 1
    assert T % 30 == 0 and T > 128, "the generator needs T = 30 Ln > 128"
    mel = torch.from_numpy(batch_mel(B, Tm)).to(dev)
    z = torch.randn(B, T // 30, 8, generator=torch.Generator().manual_seed(0)).to(dev)
    gen = Generator(dev).load_state_dict(synthetic_m2sgan_state_dict())
    m2s = M2SNet(dev).load_state_dict(synthetic_m2snet_state_dict())
    feat = gen.features(mel, z)
    parts = [("m2snet music_latent", lambda: m2s.music_latent(mel)), ("features", lambda: gen.features(mel, z)),
             ("decode", lambda: gen.decode(feat)), ("generate", lambda: gen(mel, z))]
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
    chunks = (B + 31) // 32
    print(f"B={B} Tm={Tm} T={T}: ms per call over {a.rounds} rounds of {a.iters} calls")
    for name, v in ms.items():
        print(f"  {name:24s} median {np.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}")
    dec = float(np.median(ms["decode"])) * 1e-3
    gflop, gbyte = FLOPS_PER_FRAME * B * T / 1e9, 4 * FLOATS_PER_FRAME * B * T / 1e9
    print(f"  decode: {LAUNCHES_DECODE * chunks} launches, {gflop:.1f} GFLOP -> {gflop / dec / 1e3:.1f} TFLOP/s exact fp32, "
          f"{gbyte:.2f} GB of activation reads and writes -> {gbyte / dec / 1e3:.2f} TB/s")
    print(f"  features: the music encoder's launches + {LAUNCHES_NOISE * chunks}")
    print(json.dumps({"B": B, "Tm": Tm, "decode_launches": LAUNCHES_DECODE * chunks, "decode_gflop": round(gflop, 2),
                      **{k: round(float(np.median(v)), 4) for k, v in ms.items()}}))


if __name__ == "__main__":
    main()
