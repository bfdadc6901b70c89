#!/usr/bin/env python3
"""GPU box: ms per 50-evaluation loop at 32 x 1800 (fp16, HIP events around the loops) of
    the DDIM-50 loop on a 50-step schedule (dc_sampler_ddim_loop: the headline's loop),
    the order-1 solver loop on 50 timesteps of the 1000-step schedule (dc_sampler_solver_loop, "logsnr" list),
    the order-2 solver loop on the same list (one more [B,T,P] buffer read and written per step),
three interleaved runs of each on ONE box (boxes differ by several per cent: only numbers of one run compare).
Prints one line per (run, loop) and the medians; DESIGN.md section 4.8 holds the recorded ones."""
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
from helpers import batch_noise, make_diffusion, make_model, xf_pair  # noqa: E402
from diffusion_conductor_amd import native  # noqa: E402
from diffusion_conductor_amd.sampler import spaced_timesteps  # noqa: E402

B, T, N, LOOPS = int(os.environ.get("DC_B", "32")), int(os.environ.get("DC_T", "1800")), 50, 5


def main():
    m = make_model("fp16")
    coef50 = make_diffusion(N).native_coefficients()
    ac = make_diffusion(1000).alphas_cumprod
    ts = spaced_timesteps(ac, N, "logsnr")
    assert len(ts) == N
    rows = {o: native.solver_table(ac, ts, 0.0, o)[0] for o in (1, 2)}
    xfp, xfo = (t.cuda() for t in xf_pair(B, T))
    noise = torch.from_numpy(batch_noise(B, T)).cuda()
    nat = m.set_conditioning(xfp, xfo, [T] * B)
    loops = {"ddim-50 schedule": lambda: nat.ddim_loop(noise, coef50),
             "solver order 1": lambda: nat.solver_loop(noise, ts, rows[1]),
             "solver order 2": lambda: nat.solver_loop(noise, ts, rows[2])}
    res = {}
    for rep in range(3):
        for name, run in loops.items():
            for _ in range(2):
                run()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(LOOPS):
                run()
            b.record()
            torch.cuda.synchronize()
            assert nat.status() == 0
            res.setdefault(name, []).append(a.elapsed_time(b) / LOOPS)
            print(f"run {rep} {name} {B} x {T}: {res[name][-1]:.3f} ms per {N}-evaluation loop", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print("medians: " + "; ".join(f"{k} {v:.3f} ms" for k, v in med.items()))
    print(f"order 2 against order 1: {100 * (med['solver order 2'] / med['solver order 1'] - 1):+.2f} % "
          f"({1000 * (med['solver order 2'] - med['solver order 1']) / N:+.2f} us per step); order 1 against the 50-step schedule's loop: "
          f"{100 * (med['solver order 1'] / med['ddim-50 schedule'] - 1):+.2f} %")


if __name__ == "__main__":
    main()
