#!/usr/bin/env python3
"""Time M2SNet's every-music-against-every-motion scores on the MI355X with device events ("Retrieval").

Run:  python tools/time_retrieval.py [--shapes 32,294] [--T 1800] [--rounds 20] [--e2e 294] [--out FILE.json]

For N musics x N motions of T latent frames (default 32 and 294 at 1800) three routes to the same [N, N] sums and counts are
timed in ONE process, after a warm-up of every route, in `rounds` interleaved rounds (a, b, c, a, b, c, ...), one call between two
events on the stream each:
  (a) fuse_pairs          M2SNet.fuse_pairs: k_m2s_pairs + k_m2s_pairs_reduce
  (b) fuse + roll         what there was before it: N calls of M2SNet.fuse on torch.roll'ed motion latents, torch reductions
  (c) plain torch         cat + three matmuls + sigmoid on the same GPU, the [N^2, T, 128] concatenation chunked over the musics to fit
and printed as median, minimum and maximum in milliseconds, with (a) / (b), route (b)'s own spread, and (a)'s share of the
arithmetic floor: pair tiles x 160 MFMAs x 4096 FLOP at the part's 157 TFLOP/s fp32 matrix rate.  Before timing, (a) is compared
with (b) (sums to the summation bound, counts exactly) and (c) with (a) (to 1e-3: another summation order).

--e2e N: also evaluate_dataset(retrieval=True) end to end on a synthetic N-clip set of T frames written to a temporary directory
(seeded synthetic weights, DDIM-25), and what the two fuse_pairs calls add behind the sampling ("m2s_retrieval_s")."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_FP32_MATRIX = 157.3e12


def floor_ms(n, T):
    return n * n * ((T + 31) // 32) * 160 * 4096 / PEAK_FP32_MATRIX * 1e3


def route_roll(net, mus, mot):
    n = mus.shape[0]
    total = torch.empty((n, n), device=mus.device)
    above = torch.empty((n, n), dtype=torch.int32, device=mus.device)
    below = torch.empty_like(above)
    rows = torch.arange(n, device=mus.device)
    for s in range(n):
        p = net.fuse(mus, torch.roll(mot, -s, 0).contiguous())
        cols = (rows + s) % n
        total[rows, cols] = p.sum(dim=1)
        above[rows, cols] = (p > 0.5).sum(dim=1, dtype=torch.int32)
        below[rows, cols] = (p < 0.5).sum(dim=1, dtype=torch.int32)
    return total, above, below


def route_torch(w, mus, mot, chunk):
    n, T = mus.shape[0], mus.shape[1]
    y = mot.transpose(1, 2)                                                   # [n, T, 64]
    total = torch.empty((n, n), device=mus.device)
    above = torch.empty((n, n), dtype=torch.int32, device=mus.device)
    below = torch.empty_like(above)
    for i0 in range(0, n, chunk):
        m = mus[i0:i0 + chunk]
        z = torch.cat([m[:, None].expand(-1, n, -1, -1), y[None].expand(m.shape[0], -1, -1, -1)], dim=3)      # [c, n, T, 128]
        h = torch.relu(z @ w[0].T + w[1])
        h = torch.relu(h @ w[2].T + w[3])
        p = torch.sigmoid(h @ w[4].T + w[5])[..., 0]
        total[i0:i0 + chunk] = p.sum(dim=2)
        above[i0:i0 + chunk] = (p > 0.5).sum(dim=2, dtype=torch.int32)
        below[i0:i0 + chunk] = (p < 0.5).sum(dim=2, dtype=torch.int32)
    return total, above, below


def time_shape(net, sd, n, T, rounds, dev):
    g = torch.Generator().manual_seed(n)
    mus = torch.randn((n, T, 64), generator=g).to(dev)
    mot = torch.randn((n, 64, T), generator=g).to(dev)
    w = [torch.from_numpy(np.asarray(sd[f"fuse_layer.{i}.{k}"], np.float32)).to(dev) for i in (0, 2, 4) for k in ("weight", "bias")]
    w = [t[:, :, 0] if t.dim() == 3 else t for t in w]
    chunk = max(1, min(n, int(2 ** 30 // (n * T * 128 * 4))))                  # 1 GiB of concatenation per pass
    routes = [("fuse_pairs", lambda: (lambda r: (r["sum"], r["above"], r["below"]))(net.fuse_pairs(mus, mot))),
              ("fuse_roll", lambda: route_roll(net, mus, mot)), ("torch", lambda: route_torch(w, mus, mot, chunk))]
    res = {name: fn() for name, fn in routes}                                  # warm-up, and the three results
    torch.cuda.synchronize()
    a, b, c = res["fuse_pairs"], res["fuse_roll"], res["torch"]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), "fuse_pairs and fuse + roll count differently"
    bound = (5 + (T + 31) // 32 + 12) * 2.0 ** -24 * float(a[0].max())         # both orders' depths (torch: a tree of <= 12 levels)
    assert float((a[0] - b[0]).abs().max()) <= bound, (float((a[0] - b[0]).abs().max()), bound)
    assert float(((a[0] - c[0]).abs() / a[0]).max()) <= 1e-3, float(((a[0] - c[0]).abs() / a[0]).max())
    ms = {name: [] for name, _ in routes}
    for _ in range(rounds):
        for name, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    out = {"N": n, "T": T, "rounds": rounds, "floor_ms": round(floor_ms(n, T), 4), "torch_chunk": chunk}
    print(f"{n} x {n} x {T}: ms per call, {rounds} interleaved rounds; floor {out['floor_ms']} ms")
    for name, v in ms.items():
        out[name] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                     "q1": round(float(np.percentile(v, 25)), 4), "q3": round(float(np.percentile(v, 75)), 4)}
        print(f"  {name:11s} median {out[name]['median']:10.3f}   min {out[name]['min']:10.3f}   max {out[name]['max']:10.3f}")
    out["a_over_b"] = round(out["fuse_pairs"]["median"] / out["fuse_roll"]["median"], 4)
    out["fraction_of_floor"] = round(out["floor_ms"] / out["fuse_pairs"]["median"], 4)
    print(f"  (a)/(b) {out['a_over_b']}   floor / (a) {out['fraction_of_floor']}")
    return out


def end_to_end(net, n, T, dev):
    from diffusion_conductor_amd import DDPMTrainer, MotionTransformer, evaluate as ev
    from diffusion_conductor_amd.synthetic import batch_mel, synthetic_motion, synthetic_state_dict
    root = tempfile.mkdtemp(prefix="dc_retrieval_")
    try:
        mels, gts = batch_mel(n, 3 * T - 2), synthetic_motion(n, T, seed=21)
        for i in range(n):
            d = os.path.join(root, f"{i:03d}")
            os.makedirs(d)
            np.save(os.path.join(d, "mel.npy"), mels[i])
            np.save(os.path.join(d, "motion.npy"), gts[i])
        model = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device=dev, no_clip=True)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict().items()}, strict=True)
        tr = DDPMTrainer(types.SimpleNamespace(device=dev, diffusion_steps=25, is_train=False), model.to(dev).eval())
        tr.eval_mode()
        out = {}
        for name, kw in (("sync", {}), ("retrieval", {"retrieval": True}), ("sync_again", {})):
            r = ev.evaluate_dataset(tr, root, 26, batch_size=32, seed=1, verbose=False, m2snet=net, **kw)
            out[name] = {"seconds": round(r["seconds"], 3), **({"m2s_retrieval_s": round(r["m2s_retrieval_s"], 4)} if kw else {})}
            print(f"evaluate_dataset {n} clips x {T}, DDIM-25, {name}: {out[name]}")
        return {"clips": n, "T": T, **out}
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32,294")
    ap.add_argument("--T", type=int, default=1800)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--e2e", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd.m2snet import M2SNet
    from diffusion_conductor_amd.native import NativeM2SNet
    from diffusion_conductor_amd.synthetic import synthetic_m2snet_state_dict
    dev = torch.device("cuda:0")
    sd = synthetic_m2snet_state_dict()
    net = M2SNet(dev).load_state_dict(sd)
    out = {"share": NativeM2SNet.pairs_share(), "shapes": [time_shape(net, sd, int(n), a.T, a.rounds, dev) for n in a.shapes.split(",") if n]}
    if a.e2e:
        out["e2e"] = end_to_end(net, a.e2e, a.T, dev)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
