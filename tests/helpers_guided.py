"""The checker of classifier-free guidance (include/dc_ddim.h, dc_sampler_set_conditioning_guided): oracle.ddim_sample_loop's loop,
written with the oracle's own unchanged denoiser_forward / ddim_tables / ddim_step_coefficients.  Per step TWO forward calls on the same
x_t - with the caller's features, and with the null pair broadcast over every frame - combined in fp32 before anything else of the update,

    out = c + (w - 1) (c - u)

then the oracle's update lines in their order, then helpers_known.replace_known.  The reference trains for guidance (transformer.py:389,
451-459) and never samples with it, so there is no fixture: the formula above is the definition."""
import torch

from helpers import O
from helpers_known import known_levels, replace_known


def null_pair(p):
    """(null_proj[64], null_out[64]): the all-masked limit of the reference's token dropout - proj(0) = proj.bias, and 0."""
    return p["proj.bias"].detach().clone().float(), torch.zeros(64)


def ddim_guided_loop(p, noise, xf_proj, xf_out, length, S, w, null=None, known=None, mask=None, eps=None, eta=0.0, idxs=(),
                     clip_denoised=False, eps_model=False, step_noise=None, no_eff=False):
    """O.ddim_sample_loop with guidance scale `w` (and helpers_known's replacement rule).  Returns the final sample, or
    {iteration: sample} + {S: final} when `idxs` is given."""
    co = torch.from_numpy(O.ddim_step_coefficients(O.ddim_tables(O.linear_beta_schedule(S)), eta)).to(noise.dtype)
    lv, (a0, b0) = known_levels(S)
    npj, nout = null if null is not None else null_pair(p)
    B, T = noise.shape[0], noise.shape[1]
    u_proj = npj.to(noise.dtype).view(1, 1, 64).expand(B, T, 64).contiguous()
    u_out = nout.to(noise.dtype).view(1, 1, 64).expand(B, T, 64).contiguous()
    wm1 = torch.tensor(float(w), dtype=torch.float32) - 1.0
    img = replace_known(noise, known, mask, eps, a0, b0)
    result, it = {}, 0
    with torch.no_grad():
        for i in reversed(range(S)):
            t = torch.tensor([i] * B)
            c = O.denoiser_forward(p, img, t, length, xf_proj, xf_out, 8, 8, no_eff)
            u = O.denoiser_forward(p, img, t, length, u_proj, u_out, 8, 8, no_eff)
            out = c + wm1 * (c - u)
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
