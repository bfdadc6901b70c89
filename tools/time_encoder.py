#!/usr/bin/env python3
"""Device time of encode_music (csrc/dc_music.hip) for one bs = 32 batch of 60-s clips, in both activation formats.

HIP events around `--iters` back-to-back encodes after `--warmup` untimed ones, repeated `--reps` times per format; prints the median
and the spread of the per-encode time.  One JSON line at the end.  DC_DDIM_LIB=<another build of the same ABI> times that build:
alternate the two commands on one box to compare them (every process loads one library).  `--dump FILE.npz` also writes xf_out and
xf_proj of three small seeded shapes in both formats, and of the first in the split format's separate launches, to compare two builds bit for bit (`--compare A.npz B.npz` does, without a GPU).

    python tools/time_encoder.py [--clips 32] [--frames 5400] [--reps 20] [--iters 5] [--warmup 3] [--dump FILE.npz]
    python tools/time_encoder.py --compare A.npz B.npz
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DUMP_SHAPES = ((3, 25), (3, 97), (3, 385))
DUMP_SEPARATE = {"no_stem": {"DC_ME_NO_STEM": "1"}, "no_mid": {"DC_ME_NO_MID": "1"},
                 "no_stem_no_mid": {"DC_ME_NO_STEM": "1", "DC_ME_NO_MID": "1"}}      # at DUMP_SHAPES[0], split format


def compare(a, b):
    import numpy as np
    A, B = np.load(a), np.load(b)
    same = sorted(A.files) == sorted(B.files) and all(A[k].tobytes() == B[k].tobytes() for k in A.files)
    for k in sorted(A.files):
        print(f"{k}: {'identical' if k in B.files and A[k].tobytes() == B[k].tobytes() else 'DIFFERENT'}")
    print("all bits identical" if same else "results differ")
    return 0 if same else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=32)
    ap.add_argument("--frames", type=int, default=5400, help="mel frames per clip")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dump", metavar="FILE.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    a = ap.parse_args()
    if a.compare:
        raise SystemExit(compare(*a.compare))
    import numpy as np
    import torch
    from helpers import batch_mel, make_model
    if not torch.cuda.is_available():
        raise SystemExit("time_encoder needs the MI355X (no CPU timing)")
    nat = make_model("fp16")._ensure_native("cuda:0")
    if a.dump:
        out = {}
        for B, Tm in DUMP_SHAPES:
            mel = torch.from_numpy(batch_mel(B, Tm, first=Tm)).cuda()
            for fmt in ("split", "f16"):
                nat.set_encoder_format(fmt)
                xp, xo = nat.encode_music(mel)
                torch.cuda.synchronize()
                out[f"{B}x{Tm}_{fmt}_xf_proj"], out[f"{B}x{Tm}_{fmt}_xf_out"] = xp.cpu().numpy(), xo.cpu().numpy()
        # the split format's separate launches (the library reads the switches per call)
        B, Tm = DUMP_SHAPES[0]
        mel = torch.from_numpy(batch_mel(B, Tm, first=Tm)).cuda()
        nat.set_encoder_format("split")
        for name, env in DUMP_SEPARATE.items():
            os.environ.update(env)
            try:
                xp, xo = nat.encode_music(mel)
                torch.cuda.synchronize()
            finally:
                for k in env:
                    del os.environ[k]
            out[f"{B}x{Tm}_split_{name}_xf_proj"], out[f"{B}x{Tm}_split_{name}_xf_out"] = xp.cpu().numpy(), xo.cpu().numpy()
        os.makedirs(os.path.dirname(os.path.abspath(a.dump)), exist_ok=True)
        np.savez(a.dump, **out)
    mel = torch.from_numpy(batch_mel(a.clips, a.frames)).cuda()
    T = (a.frames - 1) // 3 + 1
    bufs = (torch.empty(a.clips, T, 64, device="cuda:0"), torch.empty(a.clips, T, 64, device="cuda:0"))
    res = {"clips": a.clips, "frames": a.frames, "lib": os.environ.get("DC_DDIM_LIB", "in-tree"), "device": torch.cuda.get_device_name(0)}
    for fmt in ("split", "f16"):
        nat.set_encoder_format(fmt)
        for _ in range(a.warmup):
            nat.encode_music(mel, out=bufs)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.iters):
                nat.encode_music(mel, out=bufs)
            e.record()
            e.synchronize()
            ms.append(s.elapsed_time(e) / a.iters)
        med = statistics.median(ms)
        res[fmt] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
        print(f"{a.clips} clips x {a.frames} mel frames, {fmt:5s}: median {med:.3f} ms per encode ({min(ms):.3f} .. {max(ms):.3f} over "
              f"{a.reps} reps of {a.iters})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
