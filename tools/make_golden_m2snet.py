#!/usr/bin/env python3
"""Generate tests/golden/g13_m2snet_sync.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_m2snet.py [reference Contrastive_Stage dir]     (default: beside oracle/make_golden.py's REF; ~1 min)

What it does
  1. imports the reference's Contrastive_Stage/models/M2SNet.py on the CPU (its `models` package: MusicEncoder, MotionEncoder_STGCN,
     ST_GCN);
  2. loads the seeded synthetic weights (synthetic.synthetic_m2snet_state_dict(0)) with load_state_dict(strict=True), eval();
  3. stores the reference's fp32 probabilities M2SNet(mel, motion) [2, T, 1] for seeded inputs (tests/helpers_m2snet.py
     fixture_inputs: synthetic.smooth_mel and synthetic.synthetic_motion) at T in {2, 3, 17, 31, 32, 33, 64, 65, 90}, Tm = 3 T - 2;
  4. stores the numbers Contrastive_Stage/M2SNet_eval.py:60-67 derives from one matched / mismatched pair set (the T = 90 clips
     against their own music, and with the two motions swapped): torch.mean(...).item() of each and the 0.5-threshold accuracy;
  5. asserts what the seeded fuse head is for (synthetic.synthetic_m2snet_state_dict): over all fixture frames the fp64 logits span
     more than [-2, 2], at least 20 % of the frames lie on each side of 0, and both hidden layers have dead and live ReLU units;
     and that the repository's fp64 oracle (tests/helpers_m2snet.py) agrees with the reference's fp32 probabilities to 1e-5 (the
     measured difference, the reference's own rounding, is stored as `ref_vs_fp64`).

Weights and inputs are regenerated from their seeds by the tests; the file pins them by key list, shapes and float64 digests
(synthetic.array_digest).  Only data is written; no reference source text is copied.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g13_m2snet_sync.npz")
T_STATS = 90


def main():
    from oracle.make_golden import REF
    import helpers_m2snet as H
    from diffusion_conductor_amd.m2snet import m2snet_shapes
    from diffusion_conductor_amd.synthetic import array_digest, synthetic_m2snet_state_dict
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(REF)), "Contrastive_Stage")
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    sys.path.insert(0, ref)
    from models.M2SNet import M2SNet
    torch.set_num_threads(8)

    sd = synthetic_m2snet_state_dict(seed=0)
    net = M2SNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net.eval()
    ref_keys = list(net.state_dict().keys())
    assert ref_keys == list(m2snet_shapes()), "param spec order differs from the reference module's"
    assert len(ref_keys) == 234

    out = {"keys": np.array(ref_keys), "shapes": np.array([str(tuple(v.shape)) for v in net.state_dict().values()]),
           "weight_digest": np.stack([array_digest(v) for v in sd.values()]), "mel_seed": H.MEL_SEED, "motion_seed": H.MOTION_SEED,
           "Ts": np.array(H.FIXTURE_TS)}
    logits, a1s, a2s, worst = [], [], [], 0.0
    for T in H.FIXTURE_TS:
        mel, motion = H.fixture_inputs(T)
        with torch.no_grad():
            prob = net(torch.from_numpy(mel), torch.from_numpy(motion)).numpy()
        assert prob.shape == (2, T, 1) and prob.dtype == np.float32
        out[f"prob_T{T}"] = prob
        out[f"mel_digest_T{T}"], out[f"motion_digest_T{T}"] = array_digest(mel), array_digest(motion)
        lg, p64, a1, a2 = H.oracle_head(sd, *H.oracle_latents(sd, mel, motion), hidden=True)
        worst = max(worst, float(np.abs(p64 - prob[..., 0]).max()))
        logits.append(lg.ravel())
        a1s.append(a1.reshape(-1, 64))
        a2s.append(a2.reshape(-1, 64))
    logits, a1s, a2s = np.concatenate(logits), np.concatenate(a1s), np.concatenate(a2s)
    print(f"fp64 oracle vs reference fp32 probability: max abs {worst:.2e}")
    assert worst <= 1e-5, worst          # (the reference's own fp32 rounding through the head's gain; a sanity bound)
    out["ref_vs_fp64"] = np.float64(worst)
    pos = float((logits > 0).mean())
    print(f"fp64 logits over {logits.size} frames: [{logits.min():.2f}, {logits.max():.2f}], {100 * pos:.0f} % above 0, "
          f"min |logit| {np.abs(logits).min():.2e}")
    assert logits.min() <= -2 and logits.max() >= 2, "the seeded head's logits do not span [-2, 2]"
    assert 0.2 <= pos <= 0.8, "fewer than 20 % of the frames on one side of 0"
    for name, a in (("fuse_layer.0", a1s), ("fuse_layer.2", a2s)):
        dead, live = int((a < 0).all(0).sum()), int((a > 0).all(0).sum())
        print(f"{name}: {dead} units dead on every frame, {live} live on every frame, {64 - dead - live} switching")
        assert dead >= 1 and live >= 1 and 64 - dead - live >= 1, name
    out["logit_range"] = np.array([logits.min(), logits.max(), pos])

    # M2SNet_eval.py:59-68 on one pair set: the clips against their own music (matched) and with the motions swapped (mismatched)
    mel, motion = H.fixture_inputs(T_STATS)
    with torch.no_grad():
        pred_11 = net(torch.from_numpy(mel), torch.from_numpy(motion))
        pred_12 = net(torch.from_numpy(mel), torch.from_numpy(motion).roll(-1, 0))
    tp = np.sum(pred_11.detach().cpu().numpy() > 0.5)
    tf = np.sum(pred_12.detach().cpu().numpy() < 0.5)
    acc = (tp + tf) / (pred_11.numel() + pred_12.numel())
    out.update(stats_T=T_STATS, stats_matched=pred_11.numpy(), stats_mismatched=pred_12.numpy(),
               stats_sync=np.float64(torch.mean(pred_11).item()), stats_non_sync=np.float64(torch.mean(pred_12).item()),
               stats_accuracy=np.float64(acc.item()))
    print(f"sync {out['stats_sync']!r} non_sync {out['stats_non_sync']!r} accuracy {out['stats_accuracy']!r}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
