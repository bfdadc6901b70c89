"""The checker of sampling on a sub-sequence of timesteps, first or second order (include/dc_ddim.h, dc_solver_table /
dc_sampler_solver_loop): oracle.ddim_sample_loop's loop restated on the sub-schedule in the oracle's own
arithmetic - its unchanged denoiser_forward and ddim_tables, ddim_step_coefficients' expressions (fp64 table entry cast to fp32,
fp32 torch arithmetic, in ddim_sample's order) with (abar_t, abar_{t-1}) replaced by (abar[t_i], abar[t_{i+1}]), 1 behind the last -
plus the history term of the second-order multistep update (DPM-Solver++ 2M on the predicted x0):

    x_{i+1} = [the first-order update] + kappa_i (x0_i - x0_{i-1}),      kappa_i = 0 at i = 0 and at i = n - 1,
    lambda(a) = 1/2 ln(a / (1 - a)),  h_i = lambda(a'_i) - lambda(a_i),  r_i = h_{i-1} / h_i,
    kappa_i = (sqrt(a'_i) - sqrt(1 - a'_i) sqrt(a_i) / sqrt(1 - a_i)) / (2 r_i)        in fp64, rounded once to fp32,

x0_i being the prediction the update itself used (after guidance, the EPSILON conversion and clipping); known values are replaced
behind it (helpers_known.replace_known), guidance combines in front of everything (helpers_guided).  The reference has neither a
sub-sequence nor a second order, so there is no fixture: the lines above are the definition."""
import numpy as np
import torch

from helpers import O
from helpers_guided import null_pair
from helpers_known import replace_known


def solver_rows(S, timesteps, eta=0.0, order=1):
    """fp32 torch [n, 8]: (sqrt_recip, sqrt_recipm1, sqrt(a'), sqrt(1 - a' - sigma^2), sigma, sqrt(1 - a'), kappa, 0) per ITERATION, and
    the loop's starting pair (sqrt(a_0), sqrt(1 - a_0))."""
    tb = O.ddim_tables(O.linear_beta_schedule(S))
    ts = np.asarray(timesteps, np.int64)
    ac = tb["alphas_cumprod"]
    a64, an64 = ac[ts], np.append(ac[ts[1:]], 1.0)
    a, an = torch.from_numpy(a64).float(), torch.from_numpy(an64).float()
    sigma = eta * torch.sqrt((1 - an) / (1 - a)) * torch.sqrt(1 - a / an)
    kappa = np.zeros(len(ts))
    if order == 2:
        lam = lambda v: 0.5 * np.log(v / (1.0 - v))
        for i in range(1, len(ts) - 1):
            h, hb = lam(an64[i]) - lam(a64[i]), lam(a64[i]) - lam(a64[i - 1])
            kappa[i] = (np.sqrt(an64[i]) - np.sqrt(1 - an64[i]) * np.sqrt(a64[i]) / np.sqrt(1 - a64[i])) / (2.0 * hb / h)
    co = torch.stack([torch.from_numpy(tb["sqrt_recip_alphas_cumprod"][ts]).float(),
                      torch.from_numpy(tb["sqrt_recipm1_alphas_cumprod"][ts]).float(), torch.sqrt(an),
                      torch.sqrt(1 - an - sigma ** 2), sigma, torch.sqrt(1 - an), torch.from_numpy(kappa).float(),
                      torch.zeros(len(ts))], dim=1)
    return co, (torch.sqrt(a[0]), torch.sqrt(1 - a[0]))


def solver_loop(p, noise, xf_proj, xf_out, length, S, timesteps, order=1, w=None, null=None, known=None, mask=None, eps=None,
                eta=0.0, idxs=(), clip_denoised=False, eps_model=False, step_noise=None, no_eff=False, perturb=None):
    """The loop over `timesteps` (decreasing) of the S-step schedule.  w: None, or the guidance scale (two forward calls per step).
    perturb = (seed, rel): every evaluation's output is multiplied by 1 + rel N(0, 1), seeded - the probe that measures how a
    solver carries evaluation errors to the final sample (tools/solver_amplification.py).  Returns the final sample, or
    {iteration: sample} + {n: final} when `idxs` is given."""
    co, (a0, b0) = solver_rows(S, timesteps, eta, order)
    co, a0, b0 = co.to(noise.dtype), a0.to(noise.dtype), b0.to(noise.dtype)
    B, T = noise.shape[0], noise.shape[1]
    if w is not None:
        npj, nout = null if null is not None else null_pair(p)
        u_proj = npj.to(noise.dtype).view(1, 1, 64).expand(B, T, 64).contiguous()
        u_out = nout.to(noise.dtype).view(1, 1, 64).expand(B, T, 64).contiguous()
        wm1 = (torch.tensor(float(w), dtype=torch.float32) - 1.0).to(noise.dtype)
    gen = torch.Generator().manual_seed(int(perturb[0])) if perturb else None
    img = replace_known(noise, known, mask, eps, a0, b0)
    prev = torch.zeros_like(noise)
    result, n = {}, len(timesteps)
    with torch.no_grad():
        for it, i in enumerate(timesteps):
            t = torch.tensor([int(i)] * B)
            out = O.denoiser_forward(p, img, t, length, xf_proj, xf_out, 8, 8, no_eff)
            if w is not None:
                u = O.denoiser_forward(p, img, t, length, u_proj, u_out, 8, 8, no_eff)
                out = out + wm1 * (out - u)
            if perturb:
                out = out * (1.0 + perturb[1] * torch.randn(out.shape, generator=gen, dtype=torch.float64).to(out.dtype))
            sr, srm1, c_x0, c_eps, sigma, c_kn, kappa, _ = co[it]
            x0 = sr * img - srm1 * out if eps_model else out
            if clip_denoised:
                x0 = x0.clamp(-1, 1)
            e = (sr * img - x0) / srm1
            mean = x0 * c_x0 + c_eps * e
            if eta != 0.0:
                mean = mean + (0.0 if it == n - 1 else 1.0) * sigma * torch.as_tensor(step_noise[it]).to(noise.dtype)
            img = mean + kappa * (x0 - prev)
            prev = x0
            img = replace_known(img, known, mask, eps, c_x0, c_kn)
            if it in idxs:
                result[it] = img
    if len(idxs) == 0:
        return img
    result[n] = img
    return result
