#!/usr/bin/env python3
"""Generate tests/golden/g14_training_losses.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_losses.py [reference Diffusion_Stage dir]     (default: oracle/make_golden.py's REF; ~2 min)

What it does
  1. stubs what the reference's trainer module needs but this image lacks (oracle.make_golden._stub_modules for cv2 / mmcv), then
     imports models.gaussian_diffusion, models.transformer and trainers.ddpm_trainer;
  2. (a) GaussianDiffusion.training_losses with a STUB MODEL that returns a fixed tensor, for START_X and EPSILON, at the (B, T) of
     CASES_A with ragged lengths (1 and T among them), per-clip timesteps (0 and S - 1 among them) and explicit noise: stores the
     q_sample tables at those timesteps, x_t, every term, and the scalars of DDPMTrainer.backward_G - called UNBOUND on a namespace
     that carries the attributes it reads (DDPMTrainer.__init__ loads a hard-coded checkpoint) with the reference's
     MotionEncoder_STGCN on the seeded synthetic weights;
  3. (b) the same with the reference MotionTransformer on the seeded synthetic weights in eval mode, `text=` mel and ragged `length`,
     at CASES_B; at T = 1800 `pred` is also stored on the three 32-frame windows G12 uses.
  The per-clip numbers ("terms" [B, 8] in the layout of dc_motion_loss_terms, "latent_l1" [B]) are the reference's own: the same
  two functions run on one clip at a time (every clip has the same element count, so the batch scalars are their means).

Inputs are regenerated from their seeds (synthetic.py) by the tests; the file pins them by float64 digests (synthetic.array_digest)
instead of storing them.  Only data is written; no reference source text is copied.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g14_training_losses.npz")
S = 1000
# (B, T): lengths, timesteps, scale of the stub model's fixed output (0.005: the elbow velocity stays under the 2e-4 clamp)
CASES_A = {(1, 2): ([1], [0], 0.5), (3, 5): ([1, 5, 3], [0, S - 1, 417], 0.5), (3, 33): ([33, 1, 17], [S - 1, 0, 250], 0.5),
           (2, 65): ([1, 65], [S - 1, 0], 0.005)}
CASES_B = {(3, 64): ([64, 1, 17], [0, S - 1, 500]), (2, 1800): ([1800, 1234], [300, S - 1])}
MOTION_SEED, NOISE_SEED, STUB_SEED, MEL_SEED = 21, 22, 23, 24
WINDOWS_T1800 = np.r_[0:32, 884:916, 1768:1800]
MEAN_TYPES = ("START_X", "EPSILON")


def case_inputs(B, T):
    """x0 [B, T, 13, 2], noise [B, T, 13, 2], the stub model's unit-scale output [B, T, 26] and the mel [B, 3 T, 128] of one case, from
    their seeds (tests/helpers_losses.py regenerates them the same way)."""
    from diffusion_conductor_amd.synthetic import batch_mel, batch_noise, synthetic_motion
    first = 100 * T + B
    x0 = synthetic_motion(B, T, seed=MOTION_SEED, first=first)
    noise = batch_noise(B, T, 26, seed=NOISE_SEED, first=first).reshape(B, T, 13, 2)
    stub = batch_noise(B, T, 26, seed=STUB_SEED, first=first)
    return x0, noise, stub, (lambda: batch_mel(B, 3 * T, 128, seed=MEL_SEED, first=first))


def _import_reference(ref):
    from oracle.make_golden import _stub_modules
    _stub_modules()
    sys.path.insert(0, ref)
    return tuple(importlib.import_module(m) for m in ("models.gaussian_diffusion", "models.transformer", "trainers.ddpm_trainer"))


def main():
    from oracle.make_golden import REF
    from diffusion_conductor_amd.synthetic import array_digest, synthetic_motion_encoder_state_dict, synthetic_state_dict
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    rgd, rtf, rtr = _import_reference(ref)
    torch.set_num_threads(8)

    enc = rtr.MotionEncoder_STGCN()
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic_motion_encoder_state_dict(seed=0).items()}, strict=True)
    enc.eval()
    sd = synthetic_state_dict()
    model = rtf.MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device="cpu", music_model_path=None,
                                  no_clip=True)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.eval()

    def diffusion(mean_type):
        return rgd.GaussianDiffusion(betas=rgd.get_named_beta_schedule("linear", S), model_mean_type=getattr(rgd.ModelMeanType, mean_type),
                                     model_var_type=rgd.ModelVarType.FIXED_SMALL, loss_type=rgd.LossType.MSE)

    def backward_g(terms, lengths, T):
        ns = types.SimpleNamespace(device="cpu", motion_encoder=enc, mse_criterion=torch.nn.MSELoss(reduction="none"),
                                   l1_criterion=torch.nn.L1Loss(), fake_noise=terms["pred"], real_noise=terms["target"],
                                   velocity=terms["velocity"], velocity_elbow=terms["velocity_elbow"], velocity_head=terms["velocity_head"],
                                   src_mask=model.generate_src_mask(T, lengths))
        ns.mean_flat = lambda t: rtr.DDPMTrainer.mean_flat(ns, t)
        with torch.no_grad():
            rtr.DDPMTrainer.backward_G(ns)
        return {k: float(getattr(ns, k)) for k in ("loss_mot_rec", "loss_mot_feat", "loss_velocity", "loss_velocity_elbow",
                                                   "loss_velocity_head", "loss")}

    def run(gd, fn, x0, t, noise, lengths, kwargs=None):
        """training_losses + backward_G on the batch, then on every clip alone with the batch's own prediction as a stub."""
        B, T = x0.shape[:2]
        with torch.no_grad():
            x_t = gd.q_sample(torch.from_numpy(x0), torch.tensor(t), noise=torch.from_numpy(noise))
            terms = gd.training_losses(fn, torch.from_numpy(x0), torch.tensor(t), model_kwargs=kwargs or {}, noise=torch.from_numpy(noise))
        sc = backward_g(terms, lengths, T)
        per, feat = np.zeros((B, 8), np.float32), np.zeros(B, np.float32)
        for b in range(B):
            with torch.no_grad():
                one = gd.training_losses(lambda *a, **k: terms["pred"][b:b + 1], torch.from_numpy(x0[b:b + 1]), torch.tensor(t[b:b + 1]),
                                         noise=torch.from_numpy(noise[b:b + 1]))
            assert torch.equal(one["target"], terms["target"][b:b + 1])
            s1 = backward_g(one, lengths[b:b + 1], T)
            per[b, :6] = [float(one["mse"][0]), s1["loss_mot_rec"] * lengths[b], float(one["velocity_body"]), float(one["velocity_elbow"]),
                          float(one["velocity_head"]), float(one["velocity"])]
            feat[b] = s1["loss_mot_feat"]
        out = {"x_t": x_t.numpy(), "mse": terms["mse"].numpy(), "terms": per, "latent_l1": feat, "pred": terms["pred"].numpy(),
               "scalars": np.array([sc[k] for k in SCALAR_KEYS], np.float64)}
        for k in ("velocity_body", "velocity_elbow", "velocity_head", "velocity"):
            out[k] = np.float32(terms[k])
        return out

    out = {"S": S, "scalar_keys": np.array(SCALAR_KEYS), "latent_T1800_frames": WINDOWS_T1800,
           "seeds": np.array([MOTION_SEED, NOISE_SEED, STUB_SEED, MEL_SEED])}
    for (B, T), (lengths, t, scale) in CASES_A.items():
        x0, noise, stub, _ = case_inputs(B, T)
        fixed = torch.from_numpy((scale * stub).astype(np.float32))
        tag = f"a_B{B}_T{T}"
        out.update({f"{tag}_length": np.array(lengths), f"{tag}_t": np.array(t), f"{tag}_stub_scale": np.float32(scale),
                    f"{tag}_digest": np.stack([array_digest(x0), array_digest(noise), array_digest(stub)])})
        for mt in MEAN_TYPES:
            gd = diffusion(mt)
            r = run(gd, lambda *a, **k: fixed, x0, t, noise, lengths)
            r.pop("pred")          # (the stub's own tensor)
            out.update({f"{tag}_{mt}_{k}": v for k, v in r.items()})
        out[f"{tag}_sqrt_abar"] = gd.sqrt_alphas_cumprod[np.array(t)].astype(np.float32)
        out[f"{tag}_sqrt_1m_abar"] = gd.sqrt_one_minus_alphas_cumprod[np.array(t)].astype(np.float32)
        print(tag, {k: out[f"{tag}_START_X_{k}"] for k in ("mse", "velocity_elbow", "scalars")})
    for (B, T), (lengths, t) in CASES_B.items():
        x0, noise, _, mel_fn = case_inputs(B, T)
        mel = mel_fn()
        tag = f"b_B{B}_T{T}"
        out.update({f"{tag}_length": np.array(lengths), f"{tag}_t": np.array(t),
                    f"{tag}_digest": np.stack([array_digest(x0), array_digest(noise), array_digest(mel)])})
        for mt in MEAN_TYPES:
            r = run(diffusion(mt), model, x0, t, noise, lengths, {"text": torch.from_numpy(mel), "length": torch.LongTensor(lengths)})
            r.pop("x_t")
            if T == 1800:
                r["pred_windows"] = r["pred"][:, WINDOWS_T1800]
            out.update({f"{tag}_{mt}_{k}": v for k, v in r.items()})
            print(tag, mt, {k: r[k] for k in ("mse", "scalars")})
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.3f} MB")
    assert os.path.getsize(OUT) < (1 << 20), "over the size limit for a committed file"


SCALAR_KEYS = ("loss_mot_rec", "loss_mot_feat", "loss_velocity", "loss_velocity_elbow", "loss_velocity_head", "loss")

if __name__ == "__main__":
    main()
