#!/usr/bin/env python3
"""GPU box: sha256 of the DDIM-50 result of the benchmark batch (bs x 1800, seeded synthetic inputs) for the library selected by
DC_DDIM_LIB - two builds whose lines agree produce bit-identical poses.  usage: python tools/ab_equal.py [bs]
(DC_NO_EFF=1: the full-attention kernels; DC_RAGGED=1: clip lengths T, T - 37, T - 74, ... instead of T everywhere)
python tools/ab_equal.py --sites: one sha256 per (site of the step update, option set) of a DDIM-25 loop - the final sample, three
snapshots and the status word.  Sites: tests/test_gpu_known.py's SHAPES, a guided conditioning and a windows plan (guided and not);
DC_DISABLE_GRAPH=1 runs the same through the eager loop."""
import hashlib
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import bench  # noqa: E402
from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule  # noqa: E402
from diffusion_conductor_amd.synthetic import batch_music_features, batch_noise  # noqa: E402



def sites():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import numpy as np
    import test_gpu_known as K        # the sites' shapes, inputs and masks are the test's own
    from helpers import make_diffusion, make_model, xf_pair
    from diffusion_conductor_amd.harness import window_weights
    from diffusion_conductor_amd.synthetic import batch_step_noise
    S, P = K.S, K.P
    print(f"# {os.path.basename(os.environ.get('DC_DDIM_LIB', 'default'))}, {'eager' if os.environ.get('DC_DISABLE_GRAPH') else 'captured'} loop")
    models = {}

    def inputs(B, T, rows):      # as K._setup makes them, `rows` feature rows of their own length
        xfp, xfo = xf_pair(rows[0], rows[1], first=60)
        return dict(B=B, T=T, length=[T] * B, xfp=xfp, xfo=xfo, x=torch.from_numpy(batch_noise(B, T, first=60)),
                    known=0.5 * torch.from_numpy(batch_noise(B, T, first=260)), eps=torch.from_numpy(batch_noise(B, T, first=460)))
    todo = [(name, key, K._setup(name), {}) for name, (key, *_rest) in K.SHAPES.items()]
    todo.append(("guided", "fp16", inputs(2, 256, (2, 256)), dict(guidance_scale=2.5)))
    win = dict(window_starts=[0, 64, 128], window_weights=window_weights(224, 96, [0, 64, 128]))
    todo.append(("windows", "fp16", inputs(2, 224, (6, 96)), win))
    todo.append(("windows_guided", "fp16", inputs(2, 224, (6, 96)), dict(win, guidance_scale=2.5)))
    for name, key, d, extra in todo:
        if key not in models:
            models[key] = make_model("fp16", no_eff=True) if key == "no_eff" else make_model(key)
            models[key].check_numerics = False      # (the status word is hashed, not acted on)
        m, B, T = models[key], d["B"], d["T"]
        z = torch.from_numpy(batch_step_noise(S, B, T, first=60)).cuda()
        kn = dict(known=d["known"].cuda(), known_mask=K._mask("prefix", B, T).cuda(), known_noise=d["eps"].cuda())
        options = [("plain", {}), ("eps_clip", dict(clip_denoised=True)), ("eta_tensor", dict(eta=0.5, step_noise=z)),
                   ("eta_seeded", dict(eta=0.5, step_noise_seed=11)), ("dpmpp2m", dict(solver="dpmpp2m")), ("known", kn)]
        mk = {"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda()}
        if "window_starts" not in extra:
            mk["length"] = torch.LongTensor(d["length"])
        for oname, kw in options:
            if oname == "eps_clip" and key == "no_eff":
                continue      # (EPSILON x full attention x eta = 0: the library refuses it)
            gd = K._eps_diffusion() if oname == "eps_clip" else make_diffusion(S)
            res = gd.ddim_sample_loop(m, (B, T, P), noise=d["x"].cuda(), progress=False, idxs=[0, S // 2, S - 2], model_kwargs=mk,
                                      **dict(dict(clip_denoised=False), **kw), **extra)
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for it in (S, 0, S // 2, S - 2):
                h.update(res[it].cpu().numpy().tobytes())
            st = m._native.status()
            h.update(np.int32(st).tobytes())
            print(f"{name:<16} {oname:<11} sha256 {h.hexdigest()[:16]} status {st} |x0| {float(res[S].abs().mean()):.6f}", flush=True)


if "--sites" in sys.argv:
    sites()
    sys.exit(0)
B, T, S = int(sys.argv[1]) if len(sys.argv) > 1 else 32, 1800, 50
dev = torch.device("cuda", 0)
model = bench.build_model(os.environ.get("DC_PREC", "fp16"), bool(os.environ.get("DC_NO_EFF")), dev)
gd = GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=ModelMeanType.START_X,
                       model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)
xf = torch.from_numpy(batch_music_features(B, T)).to(dev)
xfp = torch.nn.functional.linear(xf, model.proj.weight, model.proj.bias).contiguous()
noise = torch.from_numpy(batch_noise(B, T)).to(dev)
nat = model.set_conditioning(xfp, xf, [T - 37 * i for i in range(B)] if os.environ.get("DC_RAGGED") else [T] * B)
out, _ = nat.ddim_loop(noise, gd.native_coefficients())
out2, _ = nat.ddim_loop(noise, gd.native_coefficients())
torch.cuda.synchronize()
assert nat.status() == 0 and torch.equal(out, out2)
print(f"{os.path.basename(os.environ.get('DC_DDIM_LIB', 'default'))}: bs={B} sha256 {hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]}"
      f" |x0| {float(out.abs().mean()):.6f}")
