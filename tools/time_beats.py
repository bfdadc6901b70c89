#!/usr/bin/env python3
"""Time beat consistency's two device calls on the MI355X with device events, and the host path they replace on the same box's CPU
(DESIGN.md section 15).

Run:  python tools/time_beats.py [--B 32] [--T 1800] [--Lm 5400] [--iters 20] [--rounds 5] [--out profiles/beats_timing.json]

At [B, T] (default 32 clips of 60 s, music beats [B, 5400], one every 45 mel frames = 120 beats per minute at 90 fps) it times, after
a warm-up of every shape, `iters` back-to-back calls between two events, `rounds` times, the parts taken in turn within a round:
  motion_beats         MotionRhythm.motion_beats of one motion batch (1 launch per 64 clips)
  beat_scores          MotionRhythm.beat_scores of its one-hots against the music beats (1 launch per 64 clips, plus the two small
                       torch kernels that turn the one-hots into uint8)
  both, both motions   what evaluate_dataset(music_beats=) enqueues per batch: the two calls on the generated and on the real motion
These are times per call as Python enqueues them: each is a launch of a few microseconds behind a few of torch's, so the figures are
bounded below by the host's enqueue rate and are an upper bound of the kernels' own time.

The host path is what a user has without the feature: per clip, numpy's norms and scipy.signal.argrelextrema for the beats and a Python
loop over the music beats for the score, as the reference's motion_peak_onehot and alignment_score do it (restated here in numpy /
scipy: the reference itself is not on the GPU box), for both motions of the same batch, single-threaded, wall clock; the poses'
copy back to the host is not counted.  Its beats and scores are checked against the device's before anything is timed.
Writes both figures as JSON; it promises no ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_motion_beats(m, order=10):
    """One clip [T, 13, 2] -> bool [T]: numpy + scipy, as a host evaluation does it."""
    from scipy.signal import argrelextrema
    v = np.zeros_like(m, dtype=np.float32)
    v[1:] = np.diff(m, axis=0)
    e = np.linalg.norm(v, axis=2).sum(axis=1)
    out = np.zeros(e.shape, bool)
    out[argrelextrema(e, np.less, order=order)[0]] = True
    return out


def host_bc(music, motion, sigma=3.0):
    """One clip's BC with a Python loop over its music beats."""
    mi, mo = np.flatnonzero(music), np.flatnonzero(motion)
    if not mo.size:
        return 0.0
    terms = []
    for i in mi:
        d = np.abs(i - mo).astype(np.float32)
        terms.append(np.exp(-d[np.argmin(d)] ** 2 / 2 / sigma ** 2))
    return sum(terms) / len(terms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1800)
    ap.add_argument("--Lm", type=int, default=5400)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beats_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd.rhythm import MotionRhythm
    from diffusion_conductor_amd.synthetic import synthetic_generated_motion, synthetic_motion
    dev = torch.device("cuda:0")
    B, T, Lm = a.B, a.T, a.Lm
    real_h = (synthetic_motion(B, T, seed=31) + np.float32(0.5)).astype(np.float32)
    gen_h = synthetic_generated_motion(real_h, seed=37)
    mus_h = np.zeros((B, Lm), np.uint8)
    for b in range(B):
        mus_h[b, (7 * b) % 45::45] = 1
    real, gen = (torch.from_numpy(x).to(dev).reshape(B, T, 26) for x in (real_h, gen_h))
    mus = torch.from_numpy(mus_h).to(dev)
    rh = MotionRhythm(dev)

    def both(x):
        return rh.beat_scores(rh.motion_beats(x), mus)

    # the host path gives the device's beats, and its scores agree to float32 rounding
    for x_h, x in ((real_h, real), (gen_h, gen)):
        beats = rh.motion_beats(x).cpu().numpy().astype(bool)
        bc = both(x).cpu().numpy()[:, 0]
        for b in range(B):
            hb = host_motion_beats(x_h[b])
            assert np.array_equal(hb, beats[b]), b
            assert abs(host_bc(mus_h[b], hb) - bc[b]) <= 2 * (int(mus_h[b].sum()) + 4) * 2.0 ** -24, b
    n_beats = int(rh.motion_beats(real).sum()) / B

    onehot = rh.motion_beats(real)
    parts = [("motion_beats", lambda: rh.motion_beats(real)), ("beat_scores", lambda: rh.beat_scores(onehot, mus)),
             ("both_calls_both_motions", lambda: (both(gen), both(real)))]
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
    torch.set_num_threads(1)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for x_h in (gen_h, real_h):
            for b in range(B):
                host_bc(mus_h[b], host_motion_beats(x_h[b]))
        host.append((time.perf_counter() - t0) * 1e3)
    print(f"B={B} T={T} Lm={Lm} ({n_beats:.1f} motion beats and {int(mus_h[0].sum())} music beats per clip): ms per call over "
          f"{a.rounds} rounds of {a.iters} calls")
    for name, v in ms.items():
        print(f"  {name:26s} median {np.median(v):8.3f}   min {min(v):8.3f}   max {max(v):8.3f}")
    print(f"  host, both motions         median {np.median(host):8.3f}   min {min(host):8.3f}   max {max(host):8.3f}   (numpy + scipy, one thread, 3 runs)")
    res = {"B": B, "T": T, "Lm": Lm, "motion_beats_per_clip": round(n_beats, 1), "music_beats_per_clip": int(mus_h[0].sum()),
           "device_ms": {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
           "host_both_motions_ms": {"median": round(float(np.median(host)), 3), "min": round(min(host), 3), "max": round(max(host), 3)},
           "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
