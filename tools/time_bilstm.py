#!/usr/bin/env python3
"""Time the BiLSTM pose decoder and its stages on the MI355X with device events.

Run:  python tools/time_bilstm.py [--T 1800] [--iters 10] [--rounds 5] [--out profiles/bilstm_timing.json]

At 32 x T and 1 x T (In = 128) it times, after a warm-up of every shape, `iters` back-to-back calls between two events, `rounds`
times, the parts taken in turn within a round, and reports the median, minimum and maximum per call in milliseconds:
  hidden1   layer 0: its input projection and its recurrence (plus the test hook's copy of [B, T, 256])
  hidden2   both layers (plus the same copy)
  decode    both layers and the head: PoseDecoderBiLSTM.forward
The stages follow by difference - layer 1 = hidden2 - hidden1, head = decode - hidden2 (less the copy, so a lower bound) - and a
recurrence step's time from hidden1 / T, an upper bound that still holds the projection.  Everything is written to --out as JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1800)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bilstm_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd.generator import PoseDecoderBiLSTM
    from diffusion_conductor_amd.synthetic import synthetic_bilstm_state_dict
    dev = torch.device("cuda:0")
    net = PoseDecoderBiLSTM(128, 26, dev).load_state_dict(synthetic_bilstm_state_dict(0, 128))
    result = {"T": a.T, "input_size": 128, "iters": a.iters, "rounds": a.rounds, "shapes": {}}
    for B in (32, 1):
        x = torch.randn(B, a.T, 128, generator=torch.Generator().manual_seed(B)).to(dev)
        parts = [("hidden1", lambda: net.hidden(x, 1)), ("hidden2", lambda: net.hidden(x, 2)), ("decode", lambda: net(x))]
        for _, fn in parts:                       # warm-up: code objects, the workspace
            for _ in range(2):
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
        med = {k: float(np.median(v)) for k, v in ms.items()}
        print(f"B={B} T={a.T}: ms per call over {a.rounds} rounds of {a.iters} calls")
        for name, v in ms.items():
            print(f"  {name:8s} median {np.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}")
        stages = {"layer0": med["hidden1"], "layer1": med["hidden2"] - med["hidden1"], "head": med["decode"] - med["hidden2"]}
        print(f"  by difference: layer 0 {stages['layer0']:.3f}  layer 1 {stages['layer1']:.3f}  head {stages['head']:.3f} ms;  "
              f"a step of layer 0 <= {1e3 * med['hidden1'] / a.T:.3f} us")
        result["shapes"][f"{B}x{a.T}"] = {"ms": {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
                                                for k, v in ms.items()},
                                         "stages_ms": {k: round(v, 4) for k, v in stages.items()},
                                         "step_us_upper": round(1e3 * med["hidden1"] / a.T, 4)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
