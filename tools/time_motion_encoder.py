#!/usr/bin/env python3
"""Device time of the ST-GCN motion encoder (csrc/dc_stgcn.hip) for what one bs = 32 batch of the evaluation driver encodes:
64 clips x 1800 frames (the 32 sampled motions and their 32 ground truths).

HIP events around `--iters` back-to-back encodes after `--warmup` untimed ones, repeated `--reps` times; prints the median and
the spread of the per-encode time and the achieved fraction of the fp32 MFMA peak (157.3 TFLOP/s on the MI355X) for the
algorithmic work: per frame 10 blocks of 1x1 conv (2 C_in 32 MACs), graph mix (32 x 13 x 13), temporal conv (3 x 32 x 32 x 13)
plus the 416 -> 64 fc, about 1.2 MFLOP, i.e. ~138 GFLOP per 64 x 1800 frames.  One JSON line at the end.

    python tools/time_motion_encoder.py [--clips 64] [--frames 1800] [--reps 7] [--iters 10] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP32_MFMA = 157.3e12


def flops_per_frame():
    V, C = 13, 32
    blocks = 0
    for cin in [2] + [C] * 9:
        blocks += 2 * (V * C * cin + C * V * V + 3 * C * C * V)      # 1x1 conv, graph mix, temporal conv
    return blocks + 2 * 64 * C * V                                   # fc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--frames", type=int, default=1800)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN
    from diffusion_conductor_amd.synthetic import synthetic_motion_encoder_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("time_motion_encoder needs the MI355X (no CPU timing)")
    enc = MotionEncoder_STGCN("cuda:0").load_state_dict(synthetic_motion_encoder_state_dict())
    x = (0.5 * torch.randn(a.clips, a.frames, 13, 2, generator=torch.Generator().manual_seed(0))).cuda()
    out = torch.empty(a.clips, 64, a.frames, device="cuda:0")
    for _ in range(a.warmup):
        enc.latent(x, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            enc.latent(x, out=out)
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e) / a.iters)
    med = statistics.median(ms)
    flop = flops_per_frame() * a.clips * a.frames
    res = {"clips": a.clips, "frames": a.frames, "ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
           "gflop": round(flop / 1e9, 2), "tflops": round(flop / (med * 1e-3) / 1e12, 2),
           "frac_fp32_mfma_peak": round(flop / (med * 1e-3) / PEAK_FP32_MFMA, 4), "device": torch.cuda.get_device_name(0)}
    print(f"{a.clips} clips x {a.frames} frames: median {med:.3f} ms per encode ({min(ms):.3f} .. {max(ms):.3f} over {a.reps} reps "
          f"of {a.iters}), {res['tflops']} TFLOP/s = {100 * res['frac_fp32_mfma_peak']:.1f} % of the fp32 MFMA peak")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
