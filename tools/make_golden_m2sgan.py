#!/usr/bin/env python3
"""Generate tests/golden/g15_m2sgan.npz (and its g15_m2sgan_features_*.npz) by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_m2sgan.py [reference Contrastive_Stage dir]     (default: beside oracle/make_golden.py's REF; ~1 min)

What it does
  1. imports the reference's Contrastive_Stage/models/Generator.py on the CPU (its `models` package: MusicEncoder, TCN);
  2. loads the seeded synthetic weights (synthetic.synthetic_m2sgan_state_dict(0)) with load_state_dict(strict=True), eval();
  3. stores the reference's fp32 poses Generator(mel, latent) [2, T, 13, 2] and Generator.features [2, T, 128] for seeded inputs
     (tests/helpers_m2sgan.py fixture_inputs: synthetic.smooth_mel and a seeded normal latent [2, T / 30, 8]) at the cases
     helpers_m2sgan.FIXTURE_CASES;
  4. asserts, on the reference alone, that a test on this fixture can fail: over all fixture frames the poses span more than
     [0.2, 0.8]; in every temporal block both ReLUs have units dead on every frame, units live on every frame and switching units;
     swapping the two clips' latents moves the poses by more than 1e-2;
  5. asserts that the repository's fp64 oracle (tests/helpers_m2sgan.py) agrees with the reference's fp32 poses and features at the
     level of the reference's own fp32 rounding (stored as `ref_vs_fp64`, `ref_vs_fp64_features`).

Weights and inputs are regenerated from their seeds by the tests; the file pins them by key list, shapes and float64 digests
(synthetic.array_digest).  Only data is written; no reference source text is copied.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "g15_m2sgan.npz")


def main():
    from oracle.make_golden import REF
    import helpers_m2sgan as H
    from diffusion_conductor_amd.generator import m2sgan_shapes
    from diffusion_conductor_amd.synthetic import array_digest, synthetic_m2sgan_state_dict
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(REF)), "Contrastive_Stage")
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    sys.path.insert(0, ref)
    warnings.filterwarnings("ignore", category=FutureWarning)
    from models.Generator import Generator
    torch.set_num_threads(8)

    sd = synthetic_m2sgan_state_dict(seed=0)
    net = Generator()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net.eval()
    ref_keys = list(net.state_dict().keys())
    assert ref_keys == list(m2sgan_shapes()), "param spec order differs from the reference module's"
    assert len(ref_keys) == 278
    assert [tuple(v.shape) for v in net.state_dict().values()] == list(m2sgan_shapes().values())

    out = {"keys": np.array(ref_keys), "shapes": np.array([str(tuple(v.shape)) for v in net.state_dict().values()]),
           "weight_digest": np.stack([array_digest(v) for v in sd.values()]), "mel_seed": H.MEL_SEED, "latent_seed": H.LATENT_SEED,
           "cases": np.array(H.FIXTURE_CASES)}
    feats = {name: {} for name in H.FEATURE_FILES}      # (fp32 features do not compress: several files, each under the 1 MiB limit)
    poses, pres, worst, worst_f, moved = [], None, 0.0, 0.0, np.inf
    for T, Tm in H.FIXTURE_CASES:
        mel, z = H.fixture_inputs(T, Tm)
        with torch.no_grad():
            pose = net(torch.from_numpy(mel), torch.from_numpy(z)).numpy()
            feat = net.features(torch.from_numpy(mel), torch.from_numpy(z)).numpy()
            swapped = net(torch.from_numpy(mel), torch.from_numpy(z[::-1].copy())).numpy()
        assert pose.shape == (2, T, 13, 2) and pose.dtype == np.float32 and feat.shape == (2, T, 128)
        n = H.case_name(T, Tm)
        out[f"pose_{n}"] = pose
        feats[H.feature_file(T, Tm)][f"features_{n}"] = feat
        out[f"mel_digest_{n}"], out[f"latent_digest_{n}"] = array_digest(mel), array_digest(z)
        pre = []
        f64, p64 = H.oracle_generate(sd, mel, z, pre)
        worst = max(worst, float(np.abs(p64 - pose.reshape(2, T, 26)).max()))
        worst_f = max(worst_f, float(np.abs(f64 - feat).max()))
        moved = min(moved, float(np.abs(swapped - pose).max()))
        poses.append(pose.ravel())
        pre = [a.reshape(-1, 64) for a in pre]
        pres = pre if pres is None else [np.concatenate([a, b]) for a, b in zip(pres, pre)]
    poses = np.concatenate(poses)
    print(f"fp64 oracle vs reference fp32: poses max abs {worst:.2e}, features max abs {worst_f:.2e}")
    assert worst <= 1e-5 and worst_f <= 1e-5, (worst, worst_f)      # (the reference's own fp32 rounding; a sanity bound)
    out["ref_vs_fp64"], out["ref_vs_fp64_features"] = np.float64(worst), np.float64(worst_f)
    print(f"poses over {poses.size // 26} frames: [{poses.min():.3f}, {poses.max():.3f}], std {poses.std():.3f}")
    assert poses.min() < 0.2 and poses.max() > 0.8, "the seeded decoder's poses do not span [0.2, 0.8]"
    print(f"swapping the two clips' latents moves the poses by at least {moved:.2e} (max abs per case)")
    assert moved > 1e-2, "the latent does not reach the poses"
    units = []
    for i, a in enumerate(pres):
        dead, live = int((a < 0).all(0).sum()), int((a > 0).all(0).sum())
        print(f"block {i // 2} relu{i % 2 + 1}: {dead} units dead on every frame, {live} live on every frame, {64 - dead - live} switching")
        assert dead >= 1 and live >= 1 and 64 - dead - live >= 1, (i, dead, live)
        units.append((dead, live, 64 - dead - live))
    out["pose_range"] = np.array([poses.min(), poses.max(), poses.std()])
    out["latent_swap_moves"] = np.float64(moved)
    out["relu_units"] = np.array(units)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")
    for name, d in feats.items():
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **d)
        print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")
        assert os.path.getsize(path) < 2 ** 20


if __name__ == "__main__":
    main()
