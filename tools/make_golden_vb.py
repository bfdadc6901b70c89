#!/usr/bin/env python3
"""Generate tests/golden/g19_vb_terms.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_vb.py [reference Diffusion_Stage dir]     (default: oracle/make_golden.py's REF; a few seconds)

What it does
  1. stubs what the reference's modules need but this image lacks (oracle.make_golden._stub_modules), imports
     models.gaussian_diffusion;
  2. for every mean type x variance type x clip_denoised and the (B, T) of tests/helpers_vb.py's FIXTURE_CASES, with STUB MODELS that
     return a fixed tensor (2C channels for the learned types): GaussianDiffusion._vb_terms_bpd's "output", and - by the same lines,
     normal_kl, discretized_gaussian_log_likelihood, mean_flat, _predict_eps_from_xstart on p_mean_variance's dict - the kl, the
     decoder nll, the x0 error and the epsilon error of calc_bpd_loop: "terms" [B, 5] in the order of dc_vb_terms' slots 0-4;
  3. GaussianDiffusion._prior_bpd on the same x0, and calc_bpd_loop on helpers_vb's 25-step schedule for LOOP_TYPES, with th.randn_like
     replaced by helpers_vb.loop_noise(t) for the duration of the call so that a test can noise with the same draws.
  Everything is stored twice: as the reference computes it in float32, and the same calls on float64 tensors (the tables still pass
  through .float(), as _extract_into_tensor casts them) - the reference's own fp32-vs-fp64 gap, which the tests add to their bounds.

Inputs are regenerated from their seeds (tests/helpers_vb.py make_case / loop_inputs) by the tests; the file pins them by float64
digests (synthetic.array_digest) instead of storing them.  Only data is written; no reference source text is copied.
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g19_vb_terms.npz")


def main():
    import helpers_vb as H
    from oracle.make_golden import REF, _stub_modules
    from diffusion_conductor_amd.synthetic import array_digest
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    _stub_modules()
    sys.path.insert(0, ref)
    rgd = importlib.import_module("models.gaussian_diffusion")
    torch.set_num_threads(1)

    def diffusion(betas, mt, vt):
        return rgd.GaussianDiffusion(betas=betas, model_mean_type=getattr(rgd.ModelMeanType, mt), model_var_type=getattr(rgd.ModelVarType, vt),
                                     loss_type=rgd.LossType.MSE)

    def terms(gd, fixed, x0, xt, t, noise, clip):
        """[B, 5]: _vb_terms_bpd's output, then kl, decoder nll, x0 error, epsilon error by the lines of :980-995 and :1149-1151."""
        model = lambda *a, **k: fixed      # noqa: E731
        with torch.no_grad():
            vb = gd._vb_terms_bpd(model, x_start=x0, x_t=xt, t=t, clip_denoised=clip)
            true_mean, _, true_lv = gd.q_posterior_mean_variance(x_start=x0, x_t=xt, t=t)
            out = gd.p_mean_variance(model, xt, t, clip_denoised=clip)
            kl = rgd.mean_flat(rgd.normal_kl(true_mean, true_lv, out["mean"], out["log_variance"])) / np.log(2.0)
            nll = rgd.mean_flat(-rgd.discretized_gaussian_log_likelihood(x0, means=out["mean"], log_scales=0.5 * out["log_variance"])) / np.log(2.0)
            xs = rgd.mean_flat((vb["pred_xstart"] - x0) ** 2)
            ms = rgd.mean_flat((gd._predict_eps_from_xstart(xt, t, vb["pred_xstart"]) - noise) ** 2)
        return torch.stack([vb["output"], kl, nll, xs, ms], dim=1).numpy()

    out = {"S": H.S, "loop_S": H.LOOP_S, "seeds": np.array([H.CASE_SEED, H.LOOP_NOISE_SEED])}
    betas = H.linear_betas(H.S)
    assert np.array_equal(betas, rgd.get_named_beta_schedule("linear", H.S))
    for (B, T), ts in H.FIXTURE_CASES.items():
        for mt in H.MEAN_TYPES:
            for vt in H.VAR_TYPES:
                gd = diffusion(betas, mt, vt)
                for clip in (True, False):
                    c = H.make_case(B, T, 26, mt, vt, clip, ts)
                    fixed = c["model_out"] if c["var_values"] is None else np.concatenate([c["model_out"], c["var_values"]], axis=1)
                    tag = f"c_B{B}_T{T}_{mt}_{vt}_clip{int(clip)}"
                    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
                        x0, xt, nz, fx = (torch.from_numpy(a).to(dt) for a in (c["x0"], c["xt"], c["noise"], fixed))
                        out[f"{tag}_{name}"] = terms(gd, fx, x0, xt, torch.tensor(ts), nz, clip)
                    out[f"{tag}_digest"] = np.stack([array_digest(c[k]) for k in ("x0", "xt", "model_out", "noise")])
                    assert H.band(H.case_oracle(c, mt, vt, clip)[2])[0] == 0, tag
                if mt == "START_X" and vt == "FIXED_SMALL":
                    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
                        out[f"prior_B{B}_T{T}_{name}"] = gd._prior_bpd(torch.from_numpy(c["x0"]).to(dt)).numpy()
        print(f"B={B} T={T}: largest fp32-vs-fp64 gap of a slot, relative:",
              max(float(np.max(np.abs(out[k] - out[k[:-3] + "f64"]) / np.abs(out[k[:-3] + "f64"]).clip(1e-30))) for k in out if k.startswith(f"c_B{B}_T{T}_") and k.endswith("f32")))

    lb = H.linear_betas(H.LOOP_S)
    assert np.array_equal(lb, rgd.get_named_beta_schedule("linear", H.LOOP_S))
    keep = torch.randn_like
    for mt, vt in H.LOOP_TYPES:
        gd = diffusion(lb, mt, vt)
        x0, fixed = H.loop_inputs(mt, vt)
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            steps = iter(range(H.LOOP_S - 1, -1, -1))
            torch.randn_like = lambda x, **k: torch.from_numpy(H.loop_noise(next(steps))).to(x.dtype)
            try:
                fx = torch.from_numpy(fixed).to(dt)
                r = gd.calc_bpd_loop(lambda *a, **k: fx, torch.from_numpy(x0).to(dt), clip_denoised=True)
            finally:
                torch.randn_like = keep
            assert next(steps, None) is None
            for key, v in r.items():
                out[f"loop_{mt}_{vt}_{key}_{name}"] = v.numpy()
        out[f"loop_{mt}_{vt}_digest"] = np.stack([array_digest(x0), array_digest(fixed)])
        print(f"loop {mt} {vt}: total_bpd", out[f"loop_{mt}_{vt}_total_bpd_f32"])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.3f} MB")
    assert os.path.getsize(OUT) < (1 << 20), "over the size limit for a committed file"


if __name__ == "__main__":
    main()
