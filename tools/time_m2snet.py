#!/usr/bin/env python3
"""Time M2SNet's score and its three parts on the MI355X with device events ("M2SNet").

Run:  python tools/time_m2snet.py [--B 32] [--Tm 5400] [--iters 20] [--rounds 5]

At [B, Tm] (default 32 clips of 60 s) it times, after a warm-up of every shape, `iters` back-to-back calls between two events,
`rounds` times, the parts taken in turn within a round, and prints the median, minimum and maximum per call in milliseconds:
  encode_music (sampler)   the diffusion model's MusicEncoder + proj in the split format   } the two encoders as they stand without
  motion encoder           MotionEncoder_STGCN.latent                                      } M2SNet (this part runs on any commit)
  m2snet music_latent      M2SNet's own MusicEncoder (no proj), split format
  m2snet fuse              the fuse head alone on the two latents
  m2snet score             forward end to end: music encoder + motion encoder + head
The head should be a small addition to the sum of the two encoders.  One JSON line at the end repeats the medians."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--Tm", type=int, default=5400)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd import MotionTransformer
    from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN
    from diffusion_conductor_amd.synthetic import (batch_mel, synthetic_motion, synthetic_motion_encoder_state_dict,
                                                   synthetic_state_dict)
    dev = torch.device("cuda:0")
    B, Tm, T = a.B, a.Tm, (a.Tm - 1) // 3 + 1
    mel = torch.from_numpy(batch_mel(B, Tm)).to(dev)
    motion = torch.from_numpy(synthetic_motion(B, T)).to(dev)
    model = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device=dev, no_clip=True, precision="mixed")
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict().items()}, strict=True)
    model = model.to(dev).eval()
    os.environ["DC_ME_PREC"] = "split"            # the sampler's encoder in the format M2SNet pins
    menc = MotionEncoder_STGCN(dev).load_state_dict(synthetic_motion_encoder_state_dict())
    parts = [("encode_music (sampler)", lambda: model.encode_music(mel, dev)), ("motion encoder", lambda: menc.latent(motion))]
    try:
        from diffusion_conductor_amd.m2snet import M2SNet
        from diffusion_conductor_amd.synthetic import synthetic_m2snet_state_dict
    except ImportError:
        print("(this commit has no M2SNet: the two encoders only)")
    else:
        net = M2SNet(dev).load_state_dict(synthetic_m2snet_state_dict())
        mus, mot = net.music_latent(mel), menc.latent(motion)
        parts += [("m2snet music_latent", lambda: net.music_latent(mel)), ("m2snet fuse", lambda: net.fuse(mus, mot)),
                  ("m2snet score", lambda: net(mel, motion))]
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
    print(f"B={B} Tm={Tm} T={T}: ms per call over {a.rounds} rounds of {a.iters} calls")
    for name, v in ms.items():
        print(f"  {name:24s} median {np.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}")
    print(json.dumps({"B": B, "Tm": Tm, **{k: round(float(np.median(v)), 4) for k, v in ms.items()}}))


if __name__ == "__main__":
    main()
