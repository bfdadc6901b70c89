#!/usr/bin/env python3
"""Generate tests/golden/g16_rhythm.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_rhythm.py [reference Contrastive_Stage dir]     (default: beside oracle/make_golden.py's REF; seconds)

What it does
  1. imports the reference's Contrastive_Stage/utils/loss.py (rhythm_density_error, strengh_contour_error) and
     models/Discriminator.py on the CPU;
  2. loads the seeded synthetic critic weights (synthetic.synthetic_discriminator_state_dict(0)) with load_state_dict(strict=True);
  3. for the seeded motion pairs of tests/helpers_rhythm.py (fixture_pair: synthetic_motion around 0.5 and its perturbed
     companion, two clips at every length of helpers_rhythm.FIXTURE_T) stores, clip by clip as the reference's evaluation calls them
     (batch size 1): RDE and SCE, the two standard deviations of M2SGAN_eval.py:101-102, D(x) of both motions and D.features(x) of
     the real one, and scipy.signal.welch's bins 0 .. 31 summed over the channels / 26 - each where the length allows it;
  4. stores, per quantity, `ref_vs_fp64_*`: the largest distance between the reference's fp32 value and the repository's fp64
     restatement (tests/helpers_rhythm.py) in the unit the tests use, and asserts it is at the level of fp32 rounding;
  5. asserts, on the reference alone, that a test on this fixture can fail: the critic's scores of real and generated motion
     differ by more than 1e-3 at every length, the first stage's ReLU has dead and live inputs (more than 5 % of each) at every
     length, and RDE and SCE are away from 0.

Motions and weights are regenerated from their seeds by the tests; the file pins them by float64 digests (synthetic.array_digest).
Only data is written; no reference source text is copied.
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g16_rhythm.npz")


def main():
    from oracle.make_golden import REF
    import helpers_rhythm as H
    from diffusion_conductor_amd.discriminator import discriminator_shapes
    from diffusion_conductor_amd.synthetic import array_digest, synthetic_discriminator_state_dict
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(REF)), "Contrastive_Stage")
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    sys.path.insert(0, ref)
    warnings.filterwarnings("ignore")
    from models.Discriminator import Discriminator_1DCNN
    from scipy import signal
    from utils.loss import rhythm_density_error, strengh_contour_error
    torch.set_num_threads(8)

    sd = synthetic_discriminator_state_dict(0)
    D = Discriminator_1DCNN()
    D.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    D.eval()
    keys = list(D.state_dict().keys())
    assert keys == list(discriminator_shapes()) and len(keys) == 12
    assert [tuple(v.shape) for v in D.state_dict().values()] == list(discriminator_shapes().values())
    assert sum(v.numel() for v in D.state_dict().values()) == 52641

    out = {"keys": np.array(keys), "shapes": np.array([str(tuple(v.shape)) for v in D.state_dict().values()]),
           "weight_digest": np.stack([array_digest(v) for v in sd.values()]), "lengths": np.array(H.FIXTURE_T),
           "real_seed": H.REAL_SEED, "gen_seed": H.GEN_SEED}
    worst = {k: 0.0 for k in ("rde", "sce", "sd", "psd", "score", "features")}
    relu_dead, relu_live, gap = [], [], np.inf
    for T in H.FIXTURE_T:
        real, gen = H.fixture_pair(T)
        out[f"real_digest_T{T}"], out[f"gen_digest_T{T}"] = array_digest(real), array_digest(gen)
        tr, tg = torch.from_numpy(real), torch.from_numpy(gen)
        with torch.no_grad():
            d_real, d_gen = D(tr).numpy()[:, 0], D(tg).numpy()[:, 0]
            feat = D.features(tr)[0].numpy()
            pre = D.motion_encoder[0](tr.flatten(start_dim=2).transpose(1, 2)).numpy()
        assert feat.shape == (2, 64, H.pooled_frames(T)[2])
        out[f"d_real_T{T}"], out[f"d_gen_T{T}"], out[f"features_T{T}"] = d_real, d_gen, feat
        f64 = H.critic_features(sd, real)
        worst["features"] = max(worst["features"], float(np.abs(f64 - feat).max()))
        worst["score"] = max(worst["score"], float(np.abs(H.critic_score(sd, real) - d_real).max()),
                             float(np.abs(H.critic_score(sd, gen) - d_gen).max()))
        gap = min(gap, float(np.abs(d_real - d_gen).min()))
        relu_dead.append(float((pre < 0).mean()))
        relu_live.append(float((pre > 0).mean()))
        if T >= H.MIN_CONTOUR_T:
            with torch.no_grad():
                s = np.array([strengh_contour_error(tr[i:i + 1], tg[i:i + 1]).item() for i in range(2)])
                sd_real = np.array([torch.mean(torch.std(tr[i:i + 1], dim=1)).item() for i in range(2)])
                sd_gen = np.array([torch.mean(torch.std(tg[i:i + 1], dim=1)).item() for i in range(2)])
            out[f"sce_T{T}"], out[f"sd_real_T{T}"], out[f"sd_gen_T{T}"] = s, sd_real, sd_gen
            c_real, c_gen = H.contour(real), H.contour(gen)
            out[f"contour_real_T{T}"], out[f"contour_gen_T{T}"] = c_real.astype(np.float32), c_gen.astype(np.float32)
            worst["sce"] = max(worst["sce"], float(np.abs(H.sce(c_real, c_gen) - s).max()))
            worst["sd"] = max(worst["sd"], float(np.abs(H.sd(real) - sd_real).max()), float(np.abs(H.sd(gen) - sd_gen).max()))
        if T >= H.MIN_PSD_T:
            r = np.array([rhythm_density_error(tr[i:i + 1], tg[i:i + 1]) for i in range(2)])
            out[f"rde_T{T}"] = r
            psd = {}
            for name, m in (("real", real), ("gen", gen)):
                x = m.reshape(2, T, 26)
                p = np.stack([sum(signal.welch(x[i, :, c], 30)[1] for c in range(26)) / 26 for i in range(2)])[:, :H.BINS]
                assert p.dtype == np.float32                      # scipy runs in fp32 on fp32 input
                out[f"psd_{name}_T{T}"] = psd[name] = p
                worst["psd"] = max(worst["psd"], H.psd_error(p, H.welch_psd(m)))
            worst["rde"] = max(worst["rde"], float(np.abs(H.rde(H.welch_psd(real), H.welch_psd(gen)) - r).max()))
            assert r.min() > 0.1, r
        if T >= H.MIN_CONTOUR_T:
            assert out[f"sce_T{T}"].min() > 0.1, out[f"sce_T{T}"]
    for k, v in worst.items():
        print(f"fp64 restatement vs reference fp32, {k}: {v:.2e}")
        out[f"ref_vs_fp64_{k}"] = np.float64(v)
    assert worst["rde"] <= 1e-4 and worst["sce"] <= 1e-4 and worst["sd"] <= 1e-6 and worst["psd"] <= 1e-5, worst
    assert worst["score"] <= 1e-5 and worst["features"] <= 1e-5, worst
    print(f"|D(real) - D(generated)| >= {gap:.2e} over all clips; first ReLU: {min(relu_dead):.2f} .. {max(relu_dead):.2f} of its inputs dead")
    assert gap > 1e-3, "the critic does not tell the two motions apart"
    assert min(relu_dead) > 0.05 and min(relu_live) > 0.05, (relu_dead, relu_live)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")
    assert os.path.getsize(OUT) < 2 ** 20


if __name__ == "__main__":
    main()
