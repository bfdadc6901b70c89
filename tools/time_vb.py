#!/usr/bin/env python3
"""Time one step of the variational bound on the MI355X with device events.

Run:  python tools/time_vb.py [--B 32] [--T 1800] [--iters 20] [--rounds 5] [--loop_steps 1000] [--out profiles/vb_timing.json]

At [B, T, 26], FIXED_SMALL / START_X on the 1000-step linear schedule, with the seeded synthetic denoiser, it times, after a warm-up of
every part, `iters` back-to-back calls between two events, `rounds` times, the parts taken in turn within a round:
  vb_terms             native.vb_terms behind a model evaluation (two launches: the partial sums, the combine) and its coefficients
  vb_terms_torch       the same five numbers by GaussianDiffusion.vb_terms_torch - the plain-torch definitions on the same GPU, which is
                       what a caller has without the kernel (p_mean_variance's dict built from the same model output, not timed apart)
  model                the model evaluation inside the step (MotionTransformer.forward on the set conditioning)
  q_sample_seeded      the step's noising with the library's draws
and then the wall clock of a whole calc_bpd_loop of `loop_steps` timesteps (evenly spaced when fewer than the schedule's), ending in the
one copy of the results to the host.  The kernel's numbers are checked against the plain-torch ones before anything is timed.
DC_VB_GROUPS=1 in the environment gives the same figures with ONE workgroup per clip.  Writes the figures as JSON; promises no ratio."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=1800)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--loop_steps", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vb_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from diffusion_conductor_amd import MotionTransformer, native
    from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule
    from diffusion_conductor_amd.synthetic import batch_mel, synthetic_motion, synthetic_state_dict
    dev = torch.device("cuda:0")
    B, T, S = a.B, a.T, 1000
    model = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device=dev, no_clip=True, music_model_path=None)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_state_dict().items()}, strict=True)
    model = model.to(dev).eval()
    gd = GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=ModelMeanType.START_X,
                           model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)
    x0 = torch.from_numpy(synthetic_motion(B, T, seed=31).reshape(B, T, 26)).to(dev)
    with torch.no_grad():
        xf_proj, xf_out = model.encode_music(torch.from_numpy(batch_mel(B, 3 * T, 128, seed=32)).to(dev), dev)
    mk = {"xf_proj": xf_proj, "xf_out": xf_out}
    t_host = torch.full((B,), 500, dtype=torch.long)
    t_dev = t_host.to(dev)
    qa, qs = native.q_sample_coefficients(gd.alphas_cumprod, t_host)
    x_t, nz = native.q_sample(x0, qa, qs, noise_seed=(5, 500, 0), return_noise=True)
    with torch.no_grad():
        mo = model(x_t, t_host, **mk)
    coef = native.vb_coefficients(gd.betas, gd.model_var_type, t_host)

    def kernel():
        return native.vb_terms(x0, x_t, mo, native.vb_coefficients(gd.betas, gd.model_var_type, t_host), "START_X", "FIXED_SMALL", True, noise=nz)

    def plain():
        pred = mo.clamp(-1, 1)
        mean, var, lv = gd.q_posterior_mean_variance(x_start=pred, x_t=x_t, t=t_dev)
        return gd.vb_terms_torch(x0, x_t, t_dev, {"mean": mean, "log_variance": lv, "pred_xstart": pred}, nz)

    got, want = kernel().cpu().numpy(), plain().cpu().numpy()
    assert np.allclose(got[:, :5], want[:, :5], rtol=1e-4, atol=1e-6), (got[:2], want[:2])
    del coef
    parts = [("vb_terms", kernel), ("vb_terms_torch", plain), ("model", lambda: model(x_t, t_host, **mk)),
             ("q_sample_seeded", lambda: native.q_sample(x0, qa, qs, noise_seed=(5, 500, 0), return_noise=True))]
    with torch.no_grad():
        for _, fn in parts:
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
        ts = None if a.loop_steps >= S else sorted({int(v) for v in np.floor(np.linspace(0, S - 1, a.loop_steps) + 0.5)})
        gd.calc_bpd_loop(model, x0, model_kwargs=mk, noise_seed=9, timesteps=[0, 500, 999])      # warm-up
        torch.cuda.synchronize()
        loop = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = gd.calc_bpd_loop(model, x0, model_kwargs=mk, noise_seed=9, timesteps=ts)
            vb = r["vb"].cpu()
            loop.append(time.perf_counter() - t0)
    groups = os.environ.get("DC_VB_GROUPS", "default")
    print(f"B={B} T={T} (workgroups per clip: {groups}): ms per call over {a.rounds} rounds of {a.iters} calls")
    for name, v in ms.items():
        print(f"  {name:18s} median {np.median(v):8.4f}   min {min(v):8.4f}   max {max(v):8.4f}")
    print(f"  calc_bpd_loop, {vb.shape[1]} timesteps: median {np.median(loop):.3f} s   min {min(loop):.3f}   max {max(loop):.3f}   (3 runs, wall clock)")
    res = {"B": B, "T": T, "groups": groups,
           "device_ms": {k: {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in ms.items()},
           "loop_timesteps": int(vb.shape[1]), "loop_s": {"median": round(float(np.median(loop)), 3), "min": round(min(loop), 3), "max": round(max(loop), 3)},
           "mean_vb_bits_t0": float(vb[:, -1].mean()), "device": torch.cuda.get_device_name(0), "iters": a.iters, "rounds": a.rounds}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
