"""The checker of sampling a long piece's windows in one loop (include/dc_ddim.h, dc_sampler_set_conditioning_windows; DESIGN.md
section 4.10): oracle.ddim_sample_loop's loop on ONE tensor in piece space [B, L, P], written with the oracle's own unchanged
denoiser_forward and tables.  Per step one forward call per window on rows [s_k, s_k + T) of the piece tensor with that window's
features, then in fp32, one rounding per operation,

    out[f] = sum_k w[k][f - s_k] raw_k[f - s_k]      over the windows that cover frame f, ascending k, the accumulator starting
                                                      from the first product

(guided: the conditional and the unconditional outputs are blended each, then out = c + (w - 1)(c - u)), then the update lines of the
oracle in their order - on the full schedule (helpers_guided's lines) or on a list of timesteps with the solver's history term
(helpers_solver's) - then helpers_known.replace_known.  The reference samples one window, so there is no fixture: the lines above are
the definition.  Also here: the probe of the launch rule with the windows option (tests/form_probe_windows.cpp) and the shapes of
tests/test_gpu_windows.py, shared with tests/test_host_windows.py, which pins their launch forms."""
import json
import os
import shutil
import subprocess

import torch

from helpers import ROOT, O, _cache
from helpers_guided import null_pair
from helpers_known import known_levels, replace_known
from helpers_solver import solver_rows

# name -> (model key, pieces B, window T, overlap, L, W, guidance scale or None); the internal batch is W B x T (x 2 guided)
SHAPES = {"layer16": ("fp16", 1, 256, 64, 448, 2, None),
          "narrow": ("fp16", 24, 256, 64, 640, 3, None),
          "wide_aligned": ("fp16", 40, 256, 64, 832, 4, None),
          "wide_flat": ("fp16", 22, 300, 60, 1260, 5, None),
          "group_96": ("fp16", 1, 96, 32, 160, 2, None),
          "no_eff": ("no_eff", 1, 96, 32, 160, 2, None),
          "bf16": ("bf16", 1, 256, 64, 448, 2, None),
          "mixed": ("mixed", 1, 256, 64, 448, 2, None),
          "three_cover": ("fp16", 1, 256, 128, 600, 4, None),
          "odd": ("fp16", 1, 255, 63, 447, 2, None),          # 11 622 piece elements, no multiple of 4: k_windows_update's scalar path
          "guided": ("fp16", 1, 256, 64, 448, 2, 2.0)}


def blend_windows(raws, starts, weights, L):
    """raws: W tensors [B, T, P]; weights fp32 [W, T] -> [B, L, P], the sum over the covering windows as the kernel takes it."""
    B, T, P = raws[0].shape
    acc = torch.zeros(B, L, P, dtype=raws[0].dtype)
    seen = torch.zeros(L, dtype=torch.bool)
    for k, s in enumerate(starts):
        prod = weights[k].to(raws[k].dtype).view(1, T, 1) * raws[k]
        acc[:, s:s + T] = torch.where(seen[s:s + T].view(1, T, 1), acc[:, s:s + T] + prod, prod)
        seen[s:s + T] = True
    assert bool(seen.all())
    return acc


def ddim_windows_loop(p, noise, xf_proj, xf_out, starts, weights, S, w=None, null=None, known=None, mask=None, eps=None, eta=0.0,
                      idxs=(), clip_denoised=False, eps_model=False, step_noise=None, no_eff=False, timesteps=None, order=1):
    """noise [B, L, P]; xf_proj, xf_out [W * B, T, 64] window-major; starts [W]; weights fp32 [W, T] (numpy or torch).  w: None, or the
    guidance scale.  timesteps: None - the full schedule S-1 .. 0 -, or a decreasing list with the solver `order`.  known, mask, eps,
    step_noise[it] and the snapshots are in piece space.  Returns the final piece, or {iteration: piece} + {n: final} with `idxs`."""
    B, L, P = noise.shape
    W, T = len(starts), xf_proj.shape[1]
    weights = torch.as_tensor(weights, dtype=torch.float32)
    assert xf_proj.shape[0] == W * B and tuple(weights.shape) == (W, T)
    if timesteps is None:
        co5 = torch.from_numpy(O.ddim_step_coefficients(O.ddim_tables(O.linear_beta_schedule(S)), eta)).to(noise.dtype)
        lv, (a0, b0) = known_levels(S)
        ts = list(reversed(range(S)))
        rows = [(co5[i, 0], co5[i, 1], co5[i, 2], co5[i, 3], co5[i, 4], lv[i, 0], lv[i, 1], 0.0) for i in ts]
    else:
        co, (a0, b0) = solver_rows(S, timesteps, eta, order)
        ts = [int(i) for i in timesteps]
        rows = [(r[0], r[1], r[2], r[3], r[4], r[2], r[5], r[6]) for r in co.to(noise.dtype)]
    if w is not None:
        npj, nout = null if null is not None else null_pair(p)
        u_proj = npj.to(noise.dtype).view(1, 1, 64).expand(B, T, 64).contiguous()
        u_out = nout.to(noise.dtype).view(1, 1, 64).expand(B, T, 64).contiguous()
        wm1 = torch.tensor(float(w), dtype=torch.float32) - 1.0
    length = [T] * B
    img = replace_known(noise, known, mask, eps, a0, b0)
    prev = torch.zeros_like(noise)
    result, n = {}, len(ts)
    with torch.no_grad():
        for it, i in enumerate(ts):
            t = torch.tensor([i] * B)
            cs, us = [], []
            for k, s in enumerate(starts):
                x_k = img[:, s:s + T].contiguous()
                cs.append(O.denoiser_forward(p, x_k, t, length, xf_proj[k * B:(k + 1) * B], xf_out[k * B:(k + 1) * B], 8, 8, no_eff))
                if w is not None:
                    us.append(O.denoiser_forward(p, x_k, t, length, u_proj, u_out, 8, 8, no_eff))
            out = blend_windows(cs, starts, weights, L)
            if w is not None:
                u = blend_windows(us, starts, weights, L)
                out = out + wm1 * (out - u)
            sr, srm1, c_x0, c_eps, sigma, ka, kb, kappa = rows[it]
            x0 = sr * img - srm1 * out if eps_model else out
            if clip_denoised:
                x0 = x0.clamp(-1, 1)
            e = (sr * img - x0) / srm1
            mean = x0 * c_x0 + c_eps * e
            if eta != 0.0:
                mean = mean + (0.0 if it == n - 1 else 1.0) * sigma * torch.as_tensor(step_noise[it]).to(noise.dtype)
            if timesteps is not None:
                mean = mean + kappa * (x0 - prev)
                prev = x0
            img = replace_known(mean, known, mask, eps, ka, kb)
            if it in idxs:
                result[it] = img
    if len(idxs) == 0:
        return img
    result[n] = img
    return result


def windows_probe(tmp_path_factory):
    """tests/form_probe_windows.cpp, compiled once per session with the host compiler: run(*cases) -> one dict per case."""
    import pytest

    from diffusion_conductor_amd import native
    if "form_probe_windows" not in _cache:
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
        if not os.path.exists(cxx):
            pytest.skip("no C++ compiler")
        exe = str(tmp_path_factory.mktemp("form_windows") / "form_probe_windows")
        subprocess.run([cxx, "-std=c++17", "-O1", "-I", native.CSRC, os.path.join(ROOT, "tests", "form_probe_windows.cpp"), "-o", exe], check=True)
        _cache["form_probe_windows"] = exe

    def run(*cases):
        env = {k: v for k, v in os.environ.items() if not k.startswith("DC_")}
        out = subprocess.run([_cache["form_probe_windows"]], input="\n".join(cases) + "\n", env=env, check=True, capture_output=True,
                             text=True).stdout
        res = [json.loads(ln) for ln in out.splitlines()]
        assert len(res) == len(cases)
        return res
    return run
