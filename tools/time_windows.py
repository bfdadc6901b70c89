#!/usr/bin/env python3
"""GPU box: wall time of DDPMTrainer.generate_long_music_motion, window by window (joint=False) against all windows in one loop
(joint=True), DDIM-50, fp16, windows of 1800 frames, overlap 300, synthetic mel:

    a 10-minute piece (L = 18 000, 12 windows) at B = 1 and B = 4, a 3-minute piece (L = 5 400, 4 windows) at B = 1.

The two paths are interleaved on ONE box (boxes differ by several per cent: only numbers of one run compare), two warm-up calls each,
then REPS timed calls each (host clock around a call and a device synchronisation: the encoder, the loops and the final copy);
prints every case's medians and the per-step time of k_windows_update from the profile loop.  DESIGN.md section 4.10 holds the
recorded ones (profiles/windows_times.txt).

    python tools/time_windows.py [REPS]"""
import os
import statistics
import sys
import time
from argparse import Namespace

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
from helpers import batch_mel, batch_noise, make_diffusion, make_model, xf_pair  # noqa: E402

from diffusion_conductor_amd import DDPMTrainer  # noqa: E402
from diffusion_conductor_amd.harness import plan_windows, window_weights  # noqa: E402

T, OVERLAP, S, P = 1800, 300, 50, 26
CASES = [("10 min, B = 1", 18000, 1), ("10 min, B = 4", 18000, 4), ("3 min, B = 1", 5400, 1)]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    m = make_model("fp16")
    tr = DDPMTrainer(Namespace(device="cuda", diffusion_steps=S, is_train=False), m)
    for name, L, B in CASES:
        W = len(plan_windows(L, T, OVERLAP))
        mel = torch.from_numpy(batch_mel(B, 3 * L)).cuda()
        noise = torch.from_numpy(batch_noise(B, L)).cuda()
        times = {False: [], True: []}
        for rep in range(-2, reps):
            for joint in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = tr.generate_long_music_motion(mel, P, overlap=OVERLAP, noise=noise, joint=joint)
                torch.cuda.synchronize()
                if rep >= 0:
                    times[joint].append(1e3 * (time.perf_counter() - t0))
        assert tuple(out.shape) == (B, L, P) and bool(torch.isfinite(out).all())
        seq, jnt = statistics.median(times[False]), statistics.median(times[True])
        print(f"{name}: L = {L}, {W} windows, internal batch {W * B} x {T}: sequential {seq:.1f} ms, joint {jnt:.1f} ms, x {seq / jnt:.2f} "
              f"(medians of {reps}; min {min(times[False]):.1f} / {min(times[True]):.1f}, max {max(times[False]):.1f} / {max(times[True]):.1f})",
              flush=True)
    # the blend kernel alone: the eager profile pass of the 10-minute piece at B = 1
    L, B = 18000, 1
    starts = [s for s, _ in plan_windows(L, T, OVERLAP)]
    xfp, xfo = xf_pair(len(starts) * B, T)
    nat = m.set_conditioning(xfp.cuda(), xfo.cuda(), windows=(starts, window_weights(L, T, starts), L))
    nat.set_known(None, None, None)
    nat.set_smoothing(0, 0)
    prof, _ = nat.profile_loop(torch.from_numpy(batch_noise(B, L)).cuda(), make_diffusion(S).native_coefficients())
    assert nat.status() == 0
    ms, n = prof["k_windows_update"]
    total = sum(v[0] for v in prof.values())
    print(f"profile loop, 10 min at B = 1: k_windows_update {1e3 * ms / n:.1f} us per step ({n} launches), "
          f"{100 * ms / total:.2f} % of the kernels' {total:.1f} ms; k_layer {prof['k_layer'][0]:.1f} ms, k_film_gemm {prof['k_film_gemm'][0]:.1f} ms")


if __name__ == "__main__":
    main()
