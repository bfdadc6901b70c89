#!/usr/bin/env python3
"""Generate tests/golden/g12_motion_metrics.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_stgcn.py [reference Diffusion_Stage dir]     (default: oracle/make_golden.py's REF; ~1 min)

What it does
  1. stubs what the reference's evaluation script needs but this image lacks (oracle.make_golden._stub_modules for cv2 / mmcv,
     plus librosa) and neutralises the script's module-level torch.cuda.set_device(1), then imports
     tools/eval_new_metrics.py: its MotionEncoder_STGCN and Evaluator;
  2. loads the seeded synthetic weights (synthetic.synthetic_motion_encoder_state_dict) with load_state_dict(strict=True), eval();
  3. stores the reference latents features(x)[-1] of seeded motions at T in {1, 2, 3, 17, 90, 1800} (at T = 1800 the frames of
     three 32-frame windows - start, middle, end - to keep the file small);
  4. for N_PAIRS real / generated clip pairs at T = 90 (a full-rank 90-D covariance from 64 N_PAIRS = 384 samples): their
     latents, the reference Evaluator's get_scores() and get_diversity_scores() after torch.manual_seed(s) (an Evaluator built
     without its __init__, which loads a hard-coded checkpoint), and the Sync Error the way tools/eval_old_metrics.py:90-100,
     171-197 accumulates it.

Weights and motions are regenerated from their seeds (synthetic.py) by the tests; the file pins them by key list, shapes and
float64 digests (synthetic.array_digest) instead of storing them.  Only data is written; no reference source text is copied.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g12_motion_metrics.npz")
LATENT_TS = (1, 2, 3, 17, 90, 1800)
N_PAIRS, T_PAIRS = 6, 90
MOTION_SEED, PAIR_SEED, GEN_SEED = 11, 12, 13
WINDOWS_T1800 = np.r_[0:32, 884:916, 1768:1800]      # each holds a 30-frame tile edge of k_stgcn_block
DIV_SEEDS = (0, 1, 7)


def _import_reference(ref):
    from oracle.make_golden import _stub_modules
    _stub_modules()
    sys.modules.setdefault("librosa", types.ModuleType("librosa"))   # only the beat tracker (BC, not pinned here) uses it
    sys.path.insert(0, ref)
    set_device = torch.cuda.set_device
    torch.cuda.set_device = lambda *a, **k: None                     # the script selects GPU 1 at import time
    try:
        spec = importlib.util.spec_from_file_location("ref_eval_new_metrics", os.path.join(ref, "tools", "eval_new_metrics.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        torch.cuda.set_device = set_device
    return mod


def main():
    from oracle.make_golden import REF
    from diffusion_conductor_amd.motion_encoder import motion_encoder_shapes
    from diffusion_conductor_amd.synthetic import (array_digest, synthetic_generated_motion, synthetic_motion,
                                                   synthetic_motion_encoder_state_dict)
    ref = sys.argv[1] if len(sys.argv) > 1 else REF
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    R = _import_reference(ref)
    torch.set_num_threads(8)

    sd = synthetic_motion_encoder_state_dict(seed=0)
    enc = R.MotionEncoder_STGCN()
    enc.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    enc.eval()
    ref_keys = list(enc.state_dict().keys())
    assert ref_keys == list(motion_encoder_shapes()), "param spec order differs from the reference module's"

    def latent(m):
        with torch.no_grad():
            return enc.features(torch.from_numpy(m).unsqueeze(0))[-1][0].numpy()    # the scripts' per-clip call

    out = {"keys": np.array(ref_keys), "shapes": np.array([str(tuple(v.shape)) for v in enc.state_dict().values()]),
           "weight_digest": np.stack([array_digest(v) for v in sd.values()]), "motion_seed": MOTION_SEED,
           "pair_seed": PAIR_SEED, "gen_seed": GEN_SEED, "latent_T1800_frames": WINDOWS_T1800}
    for T in LATENT_TS:
        m = synthetic_motion(2, T, seed=MOTION_SEED, first=100 * T)
        out[f"motion_digest_T{T}"] = array_digest(m)
        lat = np.stack([latent(m[i]) for i in range(2)])
        with torch.no_grad():
            assert lat.shape == (2, 64, T)
            fwd = enc(torch.from_numpy(m)).numpy()
        assert np.allclose(fwd.transpose(0, 2, 1), lat, rtol=1e-5, atol=1e-5)
        out[f"latent_T{T}"] = lat[:, :, WINDOWS_T1800] if T == 1800 else lat

    # real / generated pairs: the generated motion is the real one plus a smooth perturbation of growing size
    real = synthetic_motion(N_PAIRS, T_PAIRS, seed=PAIR_SEED)
    gen = synthetic_generated_motion(real, seed=GEN_SEED)
    ev = object.__new__(R.Evaluator)              # no __init__: it loads a hard-coded checkpoint
    ev.motion_encoder = enc
    ev.real_motion_latent_list, ev.generated_motion_latent_list = [], []
    total_latent_loss = 0
    se_clip = []
    for i in range(N_PAIRS):
        with torch.no_grad():
            rf = enc.features(torch.from_numpy(real[i]).unsqueeze(0))[-1]
            gf = enc.features(torch.from_numpy(gen[i]).unsqueeze(0))[-1]
        ev.real_motion_latent_list.append(rf[0])
        ev.generated_motion_latent_list.append(gf[0])
        cur = np.mean(((gf - rf) ** 2).numpy())     # mse_loss_latent (eval_old_metrics.py:90-100)
        se_clip.append(cur)
        total_latent_loss += cur
    se = total_latent_loss / N_PAIRS
    fgd, feat_dist = ev.get_scores()
    div = []
    for s in DIV_SEEDS:
        torch.manual_seed(s)
        div.append(ev.get_diversity_scores())
        torch.manual_seed(s)
        out[f"perm_seed{s}"] = torch.randperm(N_PAIRS).numpy()
    out.update(real_motion_digest=array_digest(real), gen_motion_digest=array_digest(gen),
               real_latent=np.stack([t.numpy() for t in ev.real_motion_latent_list]),
               gen_latent=np.stack([t.numpy() for t in ev.generated_motion_latent_list]),
               fgd=np.float64(fgd), feat_dist=np.asarray(feat_dist), diversity=np.asarray(div), div_seeds=np.array(DIV_SEEDS),
               se=np.asarray(se), se_clip=np.asarray(se_clip))
    print(f"fgd {fgd!r} ({type(fgd).__name__}), feat_dist {feat_dist!r}, diversity {div}, SE {se!r}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
