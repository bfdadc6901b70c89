#!/usr/bin/env python3
"""GPU box: ms per DDIM-50 loop (fp16, HIP events around the loop) with and without classifier-free guidance, three interleaved runs of
every configuration on ONE box (boxes differ by several per cent: only numbers of one run compare).

    python tools/time_guided.py big      guided 16 x 1800 (shared FiLM column | DC_GUIDE_FULL_FILM=1), unguided 32 x 1800, unguided 16 x 1800
    python tools/time_guided.py small    guided 1 x 1800, unguided 1 x 1800, unguided 2 x 1800

Prints one line per (run, configuration) and the medians; DESIGN.md section 4.7 holds the recorded ones (profiles/guided_times.txt)."""
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
from helpers import batch_noise, make_diffusion, make_model, xf_pair  # noqa: E402

T, S, W, LOOPS = int(os.environ.get("DC_T", "1800")), 50, 2.0, 5
CONFIGS = {"big": [("guided 16 shared", 16, True, None), ("guided 16 full", 16, True, "DC_GUIDE_FULL_FILM"),
                   ("unguided 32", 32, False, None), ("unguided 16", 16, False, None)],
           "small": [("guided 1", 1, True, None), ("unguided 1", 1, False, None), ("unguided 2", 2, False, None)]}


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "big"
    m = make_model("fp16")
    coef = make_diffusion(S).native_coefficients()
    inputs = {}
    for _, B, _, _ in CONFIGS[which]:
        if B not in inputs:
            xfp, xfo = xf_pair(B, T)
            inputs[B] = (xfp.cuda(), xfo.cuda(), torch.from_numpy(batch_noise(B, T)).cuda())
    res = {}
    for rep in range(3):
        for name, B, guided, env in CONFIGS[which]:
            xfp, xfo, noise = inputs[B]
            if env:
                os.environ[env] = "1"
            try:
                nat = m.set_conditioning(xfp, xfo, [T] * B, guided=guided)
                if guided:
                    nat.set_guidance_scale(W)
                for _ in range(2):
                    nat.ddim_loop(noise, coef)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(LOOPS):
                    nat.ddim_loop(noise, coef)
                b.record()
                torch.cuda.synchronize()
                ms = a.elapsed_time(b) / LOOPS
            finally:
                if env:
                    del os.environ[env]
            assert nat.status() == 0
            res.setdefault(name, []).append(ms)
            print(f"run {rep} {name} x {T}: {ms:.3f} ms per DDIM-{S} loop", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    print("medians: " + "; ".join(f"{k} {v:.3f} ms" for k, v in med.items()))
    if which == "big":
        print(f"shared column against the full GEMM: {100 * (med['guided 16 shared'] / med['guided 16 full'] - 1):+.1f} %; "
              f"guided 16 against unguided 32 (same internal tokens): {100 * (med['guided 16 shared'] / med['unguided 32'] - 1):+.1f} %; "
              f"against unguided 16: x {med['guided 16 shared'] / med['unguided 16']:.2f}")
    else:
        print(f"guided 1 against unguided 1: x {med['guided 1'] / med['unguided 1']:.2f}; against unguided 2: "
              f"{100 * (med['guided 1'] / med['unguided 2'] - 1):+.1f} %")


if __name__ == "__main__":
    main()
