#!/usr/bin/env python3
"""GPU box: ms per DDIM-50 loop (fp16, HIP events around the loop) over several takes per music against the plain loop over the same
clips with the music tiled, three interleaved runs of every configuration on ONE box (boxes differ by several per cent: only numbers of
one run compare).

    python tools/time_takes.py           8 musics x 4 takes, 1 x 4, 16 x 2, guided 8 x 2 - each: takes | DC_TAKES_FULL_FILM=1 | tiled

"takes" shares the FiLM GEMM (one take's groups); "full" is the same conditioning with the GEMM over every group (the launch forms of
the shared path without its saving); "tiled" is dc_sampler_set_conditioning on the tiled features, the loop as it was.  Prints one line
per (run, configuration) and the medians; DESIGN.md section 4.9 holds the recorded ones (profiles/takes_times.txt)."""
import os
import statistics
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R)
sys.path.insert(0, os.path.join(R, "tests"))
import torch  # noqa: E402
from helpers import batch_noise, make_diffusion, make_model, xf_pair  # noqa: E402

T, S, W, LOOPS = int(os.environ.get("DC_T", "1800")), 50, 2.0, 5
# (name, musics, takes, guided)
CONFIGS = [("8 x 4", 8, 4, False), ("1 x 4", 1, 4, False), ("16 x 2", 16, 2, False), ("guided 8 x 2", 8, 2, True)]
VARIANTS = ("takes", "full", "tiled")


def main():
    m = make_model("fp16")
    coef = make_diffusion(S).native_coefficients()
    inputs = {}
    for name, B, takes, _ in CONFIGS:
        xfp, xfo = xf_pair(B, T)
        inputs[name] = (xfp.cuda(), xfo.cuda(), xfp.repeat(takes, 1, 1).cuda(), xfo.repeat(takes, 1, 1).cuda(),
                        torch.from_numpy(batch_noise(B * takes, T)).cuda())
    res, outs = {}, {}
    for rep in range(3):
        for name, B, takes, guided in CONFIGS:
            xfp, xfo, xfp_t, xfo_t, noise = inputs[name]
            for var in VARIANTS:
                if var == "full":
                    os.environ["DC_TAKES_FULL_FILM"] = "1"
                try:
                    if var == "tiled":
                        nat = m.set_conditioning(xfp_t, xfo_t, [T] * (B * takes), guided=guided)
                    else:
                        nat = m.set_conditioning(xfp, xfo, [T] * B, guided=guided, takes=takes)
                    if guided:
                        nat.set_guidance_scale(W)
                    for _ in range(2):
                        out, _ = nat.ddim_loop(noise, coef)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(LOOPS):
                        nat.ddim_loop(noise, coef)
                    b.record()
                    torch.cuda.synchronize()
                    ms = a.elapsed_time(b) / LOOPS
                finally:
                    os.environ.pop("DC_TAKES_FULL_FILM", None)
                assert nat.status() == 0
                if rep == 0:
                    outs[(name, var)] = out.clone()
                res.setdefault((name, var), []).append(ms)
                print(f"run {rep} {name} x {T} {var}: {ms:.3f} ms per DDIM-{S} loop", flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for name, _, _, _ in CONFIGS:
        same = all(torch.equal(outs[(name, "takes")], outs[(name, v)]) for v in ("full", "tiled"))
        t, f, p = (med[(name, v)] for v in VARIANTS)
        print(f"medians {name} x {T}: takes {t:.3f} ms, full GEMM {f:.3f} ms, tiled plain {p:.3f} ms; takes against tiled "
              f"{100 * (t / p - 1):+.1f} %, against the full GEMM {100 * (t / f - 1):+.1f} %; same bits: {same}")


if __name__ == "__main__":
    main()
