#!/usr/bin/env python3
"""Time the mel front end on the MI355X with device events (the mel section).

Run:  python tools/time_mel.py [--seconds 60] [--batches 1 32] [--iters 20]

For each batch size B (default 1 and 32 clips of 60 s: N = 1 323 000 samples, F = 5168 frames, Tm = 5400) it times, after a warm-up
of that shape, single calls between two events, the two forms taken in turn, and prints the median, minimum and maximum of `iters`
calls in milliseconds:
  fused         MelSpectrogram.features: dc_mel_features, three launches; a frame's spectrum stays in LDS
  plain torch   the same numbers written here with torch on the same GPU: torch.stft (center, zero padding, periodic Hann), |X|^2,
                a dense matmul with the [1025, 128] filterbank, log10, the clamp, the flip and the linear interpolation
and the bytes the plain form materialises for the complex spectrum [B, 5168, 1025] alone.  The two results are compared first (the
plain form is a timing yardstick, not an oracle: the test suite has that).  One JSON line at the end repeats the medians."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def plain_torch(y, fb, window, Tm):
    """y [B, N] on the device -> [B, Tm, 128]."""
    X = torch.stft(y, 2048, hop_length=256, window=window, center=True, pad_mode="constant", return_complex=True)      # [B, 1025, F]
    p = (X.real ** 2 + X.imag ** 2).transpose(1, 2) @ fb                                                            # [B, F, 128]
    ref = p.amax(dim=(1, 2), keepdim=True)
    db = 10.0 * torch.log10(p.clamp_min(1e-10)) - 10.0 * torch.log10(ref.clamp_min(1e-10))
    v = ((db.clamp_min(-80.0) + 80.0).abs() / 80.0).flip(2)
    F = v.shape[1]
    x = ((torch.arange(Tm, dtype=torch.float64, device=y.device) + 0.5) * (F / Tm) - 0.5).float()
    i = x.floor().long()
    w = x - i.float()
    edge = (i < 0) | (i >= F - 1)
    i = i.clamp(0, F - 1)
    w = torch.where(edge, torch.zeros_like(w), w)[None, :, None]
    return v[:, i] * (1.0 - w) + v[:, (i + 1).clamp_max(F - 1)] * w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd import native
    from diffusion_conductor_amd.mel import MelSpectrogram, out_frames
    dev = torch.device("cuda:0")
    sr, N = 22050, 22050 * a.seconds
    F, Tm = 1 + N // 256, out_frames(N, sr)
    ms = MelSpectrogram(dev, sr)
    t = native.mel_tables(sr)
    dense, at = np.zeros((128, 1025), np.float32), 0
    for m in range(128):
        dense[m, t["first"][m]:t["first"][m] + t["count"][m]] = t["weights"][at:at + t["count"][m]]
        at += t["count"][m]
    fb = torch.from_numpy(dense.T.copy()).to(dev)
    window = torch.from_numpy(t["window"]).to(dev)
    result = {"N": N, "F": F, "Tm": Tm, "iters": a.iters}
    for B in a.batches:
        y = (0.1 * torch.randn(B, N, generator=torch.Generator().manual_seed(B))).to(dev)
        forms = [("fused", lambda: ms.features(y)), ("plain torch", lambda: plain_torch(y, fb, window, Tm))]
        got = [fn() for _, fn in forms]
        print(f"B={B} N={N} F={F} Tm={Tm}: largest difference between the two forms {float((got[0] - got[1]).abs().max()):.2e}")
        del got
        for _, fn in forms:                           # warm-up: code objects, workspaces, the allocator's blocks
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in forms}
        for _ in range(a.iters):
            for name, fn in forms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        for name, v in times.items():
            print(f"  {name:12s} median {np.median(v):9.3f} ms   min {min(v):9.3f}   max {max(v):9.3f}")
            result[f"{name.replace(' ', '_')}_ms_B{B}"] = round(float(np.median(v)), 4)
        print(f"  plain torch materialises {B * F * 1025 * 8 / 1e6:.1f} MB for the complex spectrum [{B}, {F}, 1025]; the fused form none "
              f"(its power plane [{B}, {F}, 128] is {B * F * 128 * 4 / 1e6:.1f} MB)")
        result[f"spectrum_bytes_B{B}"] = B * F * 1025 * 8
    print(json.dumps(result))


if __name__ == "__main__":
    main()
