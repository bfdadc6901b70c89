"""The checker of sampling around known values (include/dc_ddim.h, dc_sampler_set_known): oracle.ddim_sample_loop's loop, written
with the oracle's own unchanged denoiser_forward / ddim_tables / ddim_step_coefficients, plus the replacement rule in fp32 -

    at every noise level abar:   x[known] = sqrt(abar) known + sqrt(1 - abar) eps        (eps: ONE fixed draw per element)

applied to x_T at abar_{S-1} and to every x_{t-1} a step writes at abar_prev[t] (1 at t = 0: the final sample IS `known` there).
The reference has no DDIM loop with known values to record, so there is no fixture: the rule above is the definition."""
import numpy as np
import torch

from helpers import O


def known_levels(S):
    """fp32 (sqrt(abar_prev[t]), sqrt(1 - abar_prev[t])) per timestep [S, 2] and the loop's starting pair (sqrt(abar_{S-1}),
    sqrt(1 - abar_{S-1})), from the oracle's fp64 tables cast to fp32 first - as ddim_step_coefficients treats its entries."""
    tb = O.ddim_tables(O.linear_beta_schedule(S))
    a, ap = torch.from_numpy(tb["alphas_cumprod"]).float(), torch.from_numpy(tb["alphas_cumprod_prev"]).float()
    return torch.stack([torch.sqrt(ap), torch.sqrt(1 - ap)], 1), (torch.sqrt(a[S - 1]), torch.sqrt(1 - a[S - 1]))


def replace_known(x, known, mask, eps, ca, cb):
    if mask is None:
        return x
    return torch.where(mask != 0, ca * known + cb * eps, x)


def ddim_known_loop(p, noise, xf_proj, xf_out, length, S, known=None, mask=None, eps=None, eta=0.0, idxs=(), clip_denoised=False,
                    eps_model=False, step_noise=None, no_eff=False):
    """O.ddim_sample_loop with the replacement rule.  mask [B, T, P] (nonzero = known) or None; returns the final sample, or
    {iteration: sample} + {S: final} when `idxs` is given.  The update's lines are the oracle's, in its order."""
    co = torch.from_numpy(O.ddim_step_coefficients(O.ddim_tables(O.linear_beta_schedule(S)), eta)).to(noise.dtype)
    lv, (a0, b0) = known_levels(S)
    img = replace_known(noise, known, mask, eps, a0, b0)
    B = noise.shape[0]
    result, it = {}, 0
    with torch.no_grad():
        for i in reversed(range(S)):
            t = torch.tensor([i] * B)
            out = O.denoiser_forward(p, img, t, length, xf_proj, xf_out, 8, 8, no_eff)
            sr, srm1, c_x0, c_eps, sigma = co[i]
            x0 = sr * img - srm1 * out if eps_model else out
            if clip_denoised:
                x0 = x0.clamp(-1, 1)
            e = (sr * img - x0) / srm1
            mean = x0 * c_x0 + c_eps * e
            if eta != 0.0:
                img = mean + (0.0 if i == 0 else 1.0) * sigma * torch.as_tensor(step_noise[it]).to(noise.dtype)
            else:
                img = mean
            img = replace_known(img, known, mask, eps, lv[i, 0], lv[i, 1])
            if it in idxs:
                result[it] = img
            it += 1
    if len(idxs) == 0:
        return img
    result[it] = img
    return result


def prefix_mask(B, T, P, lens):
    """[B, T, P] fp32: the first lens[b] frames of clip b are known."""
    m = torch.zeros(B, T, P)
    for b, n in enumerate(lens):
        m[b, :n] = 1
    return m


def unknown_rel_l2(a, ref, mask):
    """rel-L2 over the UNKNOWN elements of one clip (a, ref, mask: [T, P])."""
    u = (mask == 0).numpy()
    a = np.asarray(a.detach().cpu(), np.float64)[u]
    r = np.asarray(ref.detach().cpu(), np.float64)[u]
    return float(np.linalg.norm(a - r) / max(np.linalg.norm(r), 1e-30))
