"""Drop-in for the sampling half of the reference's ``GaussianDiffusion``.

Mirrors Diffusion_Stage/models/gaussian_diffusion.py: ``get_named_beta_schedule`` (:228-245),
the enums (:275-308), the constructor tables (:328-379) and the DDIM entry points
``ddim_sample`` (:783-831), ``ddim_sample_loop`` (:871-915) and
``ddim_sample_loop_progressive`` (:917-965), with the reference's argument names.

Fast path: when ``model`` is this package's MotionTransformer and no host callback
(``denoised_fn`` / ``cond_fn``) is given, the whole loop runs inside libdc_ddim.so as a replayed
hipGraph - for ``model_mean_type`` START_X (how DDPMTrainer.generate_music_motion calls it) or
EPSILON, with or without ``clip_denoised`` (the reference's default is True) and for any ``eta``
(the per-iteration noise the reference draws with ``th.randn_like`` is drawn up front, or taken
from the extension keyword ``step_noise=`` so that runs can be reproduced).  A host callback
(``denoised_fn``, ``cond_fn`` with the reference's ``condition_score``, :581-603), the
``PREVIOUS_X`` parameterisation (:510-514), a learned-variance model (2C output channels,
:472-486) or the progressive generator run the same update rule step by step with the model
call still going through the native denoiser; ``p_mean_variance`` (:442-536) is provided whole.

The FORWARD VALUE of the training objective is here as an evaluator: ``q_sample`` (:398-416) and
``training_losses`` (:1002-1090) for the MSE loss types, under ``no_grad`` - with this package's
MotionTransformer on a GPU the noising and the reductions are the kernels of csrc/dc_loss.hip, with
any other callable or device the same definitions in plain torch.

So is the VARIATIONAL BOUND as a score: ``normal_kl`` (:162-188), ``approx_standard_normal_cdf``,
``discretized_gaussian_log_likelihood`` (:191-225), ``mean_flat``, ``q_mean_variance`` (:381-396),
``_vb_terms_bpd`` (:967-1000), ``_prior_bpd`` (:1092-1108) and ``calc_bpd_loop`` (:1110-1165), for all
three mean types and all four variance types.  On GPU tensors what follows each model evaluation is
one fused pass (dc_vb_terms); on the host, or with ``denoised_fn``, the same definitions in plain torch.

Gradients, the optimiser, the bound as a TRAINING objective (``LossType.KL`` / ``RESCALED_KL`` and the
learned-variance term of ``training_losses``), ancestral ``p_sample`` and the loss-aware schedule
samplers stay out of scope and are not provided.
"""
from __future__ import annotations

import os
import warnings

import enum
import math

import numpy as np
import torch as th

from . import native
from .denoiser import MotionTransformer


def get_named_beta_schedule(schedule_name, num_diffusion_timesteps):
    """gaussian_diffusion.py:228-245."""
    if schedule_name == "linear":
        scale = 1000 / num_diffusion_timesteps
        return np.linspace(scale * 0.0001, scale * 0.02, num_diffusion_timesteps, dtype=np.float64)
    if schedule_name == "cosine":
        return betas_for_alpha_bar(num_diffusion_timesteps,
                                   lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2)
    raise NotImplementedError(f"unknown beta schedule: {schedule_name}")


def betas_for_alpha_bar(num_diffusion_timesteps, alpha_bar, max_beta=0.999):
    """gaussian_diffusion.py:248-266."""
    betas = []
    for i in range(num_diffusion_timesteps):
        t1 = i / num_diffusion_timesteps
        t2 = (i + 1) / num_diffusion_timesteps
        betas.append(min(1 - alpha_bar(t2) / alpha_bar(t1), max_beta))
    return np.array(betas)


def spaced_timesteps(alphas_cumprod, n, spacing="uniform"):
    """A decreasing list of at most `n` timesteps of the training schedule `alphas_cumprod` [S] to sample on (no counterpart in the
    reference, whose loops walk every timestep; improved-diffusion's SpacedDiffusion picks such lists).  It always starts at S - 1.
    `spacing`:
      "uniform"  round(k (S - 1) / (n - 1)), k = 0 .. n-1: equal strides in the timestep number, both ends included.  On a linear
                 beta schedule the last stride then spans most of the log-SNR range (1000 steps, n = 25: 3.6 units of lambda out
                 of 9.6), and the second-order solver ("dpmpp2m"), whose error constants assume comparable strides in lambda, is
                 WORSE than DDIM below about 50 steps on the closed-form model of tests/test_host_solver.py.  Use it with "ddim".
      "logsnr"   n targets equally spaced in lambda = 1/2 ln(abar / (1 - abar)) between lambda(abar_{S-1}) and lambda(abar_0), each
                 replaced by the nearest timestep, duplicates dropped (the list can be shorter than n).  The spacing the
                 second-order solver is analysed for.
    n = 1 gives [S - 1]; n = S the full sequence S-1 .. 0 with either spacing."""
    ac = np.asarray(alphas_cumprod, np.float64).reshape(-1)
    S, n = int(ac.shape[0]), int(n)
    if not 1 <= n <= S:
        raise ValueError(f"steps must be in [1, {S}], got {n}")
    if spacing not in ("uniform", "logsnr"):
        raise ValueError(f"spacing must be 'uniform' or 'logsnr', got {spacing!r}")
    if n == 1:
        return [S - 1]
    if n == S:
        return list(range(S - 1, -1, -1))
    if spacing == "uniform":
        ts = {int(math.floor(k * (S - 1) / (n - 1) + 0.5)) for k in range(n)}
    else:
        lam = 0.5 * np.log(ac / (1.0 - ac))
        targets = np.linspace(lam[S - 1], lam[0], n)
        ts = {int(t) for t in np.abs(lam[None, :] - targets[:, None]).argmin(axis=1)}
    return sorted(ts, reverse=True)


class ModelMeanType(enum.Enum):
    PREVIOUS_X = enum.auto()
    START_X = enum.auto()
    EPSILON = enum.auto()


class ModelVarType(enum.Enum):
    LEARNED = enum.auto()
    FIXED_SMALL = enum.auto()
    FIXED_LARGE = enum.auto()
    LEARNED_RANGE = enum.auto()


class LossType(enum.Enum):
    MSE = enum.auto()
    RESCALED_MSE = enum.auto()
    KL = enum.auto()
    RESCALED_KL = enum.auto()

    def is_vb(self):
        return self == LossType.KL or self == LossType.RESCALED_KL


def _extract(arr, timesteps, broadcast_shape, device=None):
    """_extract_into_tensor (gaussian_diffusion.py:1168-1181) without the per-call H2D copy of the
    whole table: the needed scalars are gathered on the host.  `device` (default: the timesteps' own): where the result goes -
    timesteps kept on the host then cost no wait for the device."""
    t = timesteps.detach().cpu().numpy()
    res = th.from_numpy(np.asarray(arr)[t]).float().to(timesteps.device if device is None else device)
    while len(res.shape) < len(broadcast_shape):
        res = res[..., None]
    return res.expand(broadcast_shape)


def mean_flat(tensor):
    """gaussian_diffusion.py:155-159: the mean over all non-batch dimensions."""
    return tensor.mean(dim=list(range(1, len(tensor.shape))))


def normal_kl(mean1, logvar1, mean2, logvar2):
    """gaussian_diffusion.py:162-188: the KL divergence between two gaussians; shapes broadcast, scalars are accepted."""
    tensor = None
    for obj in (mean1, logvar1, mean2, logvar2):
        if isinstance(obj, th.Tensor):
            tensor = obj
            break
    assert tensor is not None, "at least one argument must be a Tensor"
    logvar1, logvar2 = [x if isinstance(x, th.Tensor) else th.tensor(x).to(tensor) for x in (logvar1, logvar2)]
    return 0.5 * (-1.0 + logvar2 - logvar1 + th.exp(logvar1 - logvar2) + ((mean1 - mean2) ** 2) * th.exp(-logvar2))


def approx_standard_normal_cdf(x):
    """gaussian_diffusion.py:191-196: the tanh approximation of the standard normal's cumulative distribution function."""
    return 0.5 * (1.0 + th.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * th.pow(x, 3))))


def discretized_gaussian_log_likelihood(x, *, means, log_scales):
    """gaussian_diffusion.py:199-225: the log-likelihood (nats) of a Gaussian discretised to bins of 2/255 around `x` in [-1, 1]; the
    two outermost bins are open-ended, and a probability is clamped at 1e-12."""
    assert x.shape == means.shape == log_scales.shape
    centered_x = x - means
    inv_stdv = th.exp(-log_scales)
    cdf_plus = approx_standard_normal_cdf(inv_stdv * (centered_x + 1.0 / 255.0))
    cdf_min = approx_standard_normal_cdf(inv_stdv * (centered_x - 1.0 / 255.0))
    log_cdf_plus = th.log(cdf_plus.clamp(min=1e-12))
    log_one_minus_cdf_min = th.log((1.0 - cdf_min).clamp(min=1e-12))
    cdf_delta = cdf_plus - cdf_min
    log_probs = th.where(x < -0.999, log_cdf_plus, th.where(x > 0.999, log_one_minus_cdf_min, th.log(cdf_delta.clamp(min=1e-12))))
    assert log_probs.shape == x.shape
    return log_probs


class GaussianDiffusion:
    def __init__(self, *, betas, model_mean_type, model_var_type, loss_type, rescale_timesteps=False):
        self.model_mean_type = model_mean_type
        self.model_var_type = model_var_type
        self.loss_type = loss_type
        self.rescale_timesteps = rescale_timesteps
        betas = np.array(betas, dtype=np.float64)
        self.betas = betas
        assert len(betas.shape) == 1, "betas must be 1-D"
        assert (betas > 0).all() and (betas <= 1).all()
        self.num_timesteps = int(betas.shape[0])
        alphas = 1.0 - betas
        self.alphas_cumprod = np.cumprod(alphas, axis=0)
        self.alphas_cumprod_prev = np.append(1.0, self.alphas_cumprod[:-1])
        self.alphas_cumprod_next = np.append(self.alphas_cumprod[1:], 0.0)
        self.sqrt_alphas_cumprod = np.sqrt(self.alphas_cumprod)
        self.sqrt_one_minus_alphas_cumprod = np.sqrt(1.0 - self.alphas_cumprod)
        self.log_one_minus_alphas_cumprod = np.log(1.0 - self.alphas_cumprod)
        self.sqrt_recip_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod)
        self.sqrt_recipm1_alphas_cumprod = np.sqrt(1.0 / self.alphas_cumprod - 1)
        # posterior q(x_{t-1} | x_t, x_0) (gaussian_diffusion.py:363-379): read by the PREVIOUS_X parameterisation, the learned-range
        # variance and p_mean_variance's "mean" - never by the captured loop
        self.posterior_variance = betas * (1.0 - self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_log_variance_clipped = np.log(np.append(self.posterior_variance[1], self.posterior_variance[1:])) \
            if self.num_timesteps > 1 else np.log(np.maximum(self.posterior_variance, 1e-20))
        self.posterior_mean_coef1 = betas * np.sqrt(self.alphas_cumprod_prev) / (1.0 - self.alphas_cumprod)
        self.posterior_mean_coef2 = (1.0 - self.alphas_cumprod_prev) * np.sqrt(alphas) / (1.0 - self.alphas_cumprod)
        self._native_coef = None

    # ---- helpers ------------------------------------------------------------------------
    def _scale_timesteps(self, t):
        if self.rescale_timesteps:
            return t.float() * (1000.0 / self.num_timesteps)
        return t

    def _predict_eps_from_xstart(self, x_t, t, pred_xstart):
        return (_extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape, x_t.device) * x_t - pred_xstart) / \
            _extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape, x_t.device)

    def _predict_xstart_from_eps(self, x_t, t, eps):
        return _extract(self.sqrt_recip_alphas_cumprod, t, x_t.shape, x_t.device) * x_t - \
            _extract(self.sqrt_recipm1_alphas_cumprod, t, x_t.shape, x_t.device) * eps

    def _predict_xstart_from_xprev(self, x_t, t, xprev):
        """gaussian_diffusion.py:545-553: (xprev - coef2 * x_t) / coef1."""
        assert x_t.shape == xprev.shape
        return _extract(1.0 / self.posterior_mean_coef1, t, x_t.shape, x_t.device) * xprev - \
            _extract(self.posterior_mean_coef2 / self.posterior_mean_coef1, t, x_t.shape, x_t.device) * x_t

    def q_posterior_mean_variance(self, x_start, x_t, t):
        """gaussian_diffusion.py:418-440."""
        assert x_start.shape == x_t.shape
        mean = _extract(self.posterior_mean_coef1, t, x_t.shape) * x_start + _extract(self.posterior_mean_coef2, t, x_t.shape) * x_t
        return mean, _extract(self.posterior_variance, t, x_t.shape), _extract(self.posterior_log_variance_clipped, t, x_t.shape)

    def _model_output(self, model, x, t, model_kwargs):
        """The model call of p_mean_variance (gaussian_diffusion.py:466-476): returns (mean-parameter output, variance values or None).
        A learned-variance model emits 2C channels along dim 1, split as th.split(model_output, C, dim=1) (:474)."""
        if model_kwargs is None:
            model_kwargs = {}
        B, C = x.shape[:2]
        assert t.shape == (B,)
        model_output = model(x, self._scale_timesteps(t), **model_kwargs)
        if self.model_var_type in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE):
            assert model_output.shape == (B, 2 * C, *x.shape[2:])
            return th.split(model_output, C, dim=1)
        return model_output, None

    def _xstart_of(self, model_output, x, t, clip_denoised, denoised_fn):
        """pred_xstart of p_mean_variance (gaussian_diffusion.py:497-521) for the three parameterisations."""
        if self.model_mean_type == ModelMeanType.PREVIOUS_X:
            pred = self._predict_xstart_from_xprev(x_t=x, t=t, xprev=model_output)
        elif self.model_mean_type == ModelMeanType.START_X:
            pred = model_output
        elif self.model_mean_type == ModelMeanType.EPSILON:
            pred = self._predict_xstart_from_eps(x_t=x, t=t, eps=model_output)
        else:
            raise NotImplementedError(self.model_mean_type)
        if denoised_fn is not None:
            pred = denoised_fn(pred)
        if clip_denoised:
            pred = pred.clamp(-1, 1)
        assert pred.shape == x.shape
        return pred

    def _pred_xstart(self, model, x, t, clip_denoised, denoised_fn, model_kwargs):
        """The part of p_mean_variance (gaussian_diffusion.py:442-536) DDIM reads: pred_xstart."""
        model_output, _ = self._model_output(model, x, t, model_kwargs)
        return self._xstart_of(model_output, x, t, clip_denoised, denoised_fn)

    def p_mean_variance(self, model, x, t, clip_denoised=True, denoised_fn=None, model_kwargs=None):
        """gaussian_diffusion.py:442-536, whole: {"mean", "variance", "log_variance", "pred_xstart"}.  (DDIM reads pred_xstart only:
        ddim_sample takes the short way through _pred_xstart.)"""
        model_output, var_values = self._model_output(model, x, t, model_kwargs)
        if self.model_var_type == ModelVarType.LEARNED:
            log_variance = var_values
            variance = th.exp(log_variance)
        elif self.model_var_type == ModelVarType.LEARNED_RANGE:
            min_log = _extract(self.posterior_log_variance_clipped, t, x.shape)
            max_log = _extract(np.log(self.betas), t, x.shape)
            frac = (var_values + 1) / 2                       # the model's [-1, 1] covers [min_var, max_var]
            log_variance = frac * max_log + (1 - frac) * min_log
            variance = th.exp(log_variance)
        else:
            var, logvar = {
                ModelVarType.FIXED_LARGE: (np.append(self.posterior_variance[1], self.betas[1:]),
                                           np.log(np.append(self.posterior_variance[1], self.betas[1:]))),
                ModelVarType.FIXED_SMALL: (self.posterior_variance, self.posterior_log_variance_clipped),
            }[self.model_var_type]
            variance, log_variance = _extract(var, t, x.shape), _extract(logvar, t, x.shape)
        pred_xstart = self._xstart_of(model_output, x, t, clip_denoised, denoised_fn)
        if self.model_mean_type == ModelMeanType.PREVIOUS_X:
            mean = model_output
        else:
            mean, _, _ = self.q_posterior_mean_variance(x_start=pred_xstart, x_t=x, t=t)
        assert mean.shape == log_variance.shape == pred_xstart.shape == x.shape
        return {"mean": mean, "variance": variance, "log_variance": log_variance, "pred_xstart": pred_xstart}

    def condition_score(self, cond_fn, p_mean_var, x, t, model_kwargs=None):
        """gaussian_diffusion.py:581-603 (Song et al. 2020): the prediction the model would have made had its score been conditioned
        by cond_fn = grad log p(y | x).  "mean" is recomputed only when the input carries one (DDIM does not read it)."""
        alpha_bar = _extract(self.alphas_cumprod, t, x.shape)
        eps = self._predict_eps_from_xstart(x, t, p_mean_var["pred_xstart"])
        eps = eps - (1 - alpha_bar).sqrt() * cond_fn(x, self._scale_timesteps(t), **(model_kwargs or {}))
        out = dict(p_mean_var)
        out["pred_xstart"] = self._predict_xstart_from_eps(x, t, eps)
        if "mean" in out:
            out["mean"], _, _ = self.q_posterior_mean_variance(x_start=out["pred_xstart"], x_t=x, t=t)
        return out

    # ---- the denoising objective, forward value ------------------------------------------
    def q_sample(self, x_start, t, noise=None, noise_seed=None):
        """gaussian_diffusion.py:398-416: x_t = sqrt(abar_t) x_start + sqrt(1 - abar_t) noise, per-clip t [B].  On a GPU tensor this is
        dc_q_sample, on the host the same fp32 expression in torch - the reference's bits either way.
        `noise_seed` (extension, GPU only): seed, or (seed, iteration, first_element) - the library's own draws in place of
        th.randn_like (native.step_noise's for (seed, iteration), from element first_element on)."""
        x = th.as_tensor(x_start)
        if noise is not None and noise_seed is not None:
            raise ValueError("noise= and noise_seed= exclude each other")
        if noise is None and noise_seed is None:
            noise = th.randn_like(x)
        if x.is_cuda:
            a, s = native.q_sample_coefficients(self.alphas_cumprod, t)
            xc = x.to(th.float32).contiguous()
            if noise is not None:
                assert noise.shape == x.shape
                return native.q_sample(xc, a, s, noise=noise.to(device=x.device, dtype=th.float32).contiguous())
            return native.q_sample(xc, a, s, noise_seed=noise_seed)
        if noise is None:
            raise ValueError("noise_seed= draws on the device; on the host pass noise=")
        assert noise.shape == x.shape
        return _extract(self.sqrt_alphas_cumprod, t, x.shape) * x + _extract(self.sqrt_one_minus_alphas_cumprod, t, x.shape) * noise

    BODY_JOINTS_IDX = (10, 11, 12, 13, 22, 23, 24, 25)      # gaussian_diffusion.py:1075-1077
    ELBOW_JOINTS_IDX = (14, 15, 16, 17, 18, 19, 20, 21)
    HEAD_JOINTS_IDX = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)

    @classmethod
    def loss_terms_torch(cls, pred, target, length=None):
        """native.motion_loss_terms in plain torch (fp32, any device): [B, 8] per clip - mse, masked reconstruction sum, velocity body /
        elbow / head, velocity, 0, 0 (include/dc_ddim.h, dc_motion_loss_terms)."""
        B, T = pred.shape[:2]
        d2 = (target - pred) ** 2
        ln = th.full((B,), T, dtype=th.long) if length is None else th.as_tensor(length).long().cpu().reshape(B)
        if bool((ln < 1).any()) or bool((ln > T).any()):
            raise ValueError(f"length must be inside [1, {T}], got {ln.tolist()}")
        mask = (th.arange(T)[None, :] < ln[:, None]).to(pred)
        vp = pred[:, 1:] - pred[:, :-1]
        vt = target[:, 1:] - target[:, :-1]
        cols = [d2.mean(dim=(1, 2)), (d2.mean(dim=-1) * mask).sum(dim=1)]
        cols += [(vp[:, :, list(idx)] ** 2).mean(dim=(1, 2)) for idx in (cls.BODY_JOINTS_IDX, cls.ELBOW_JOINTS_IDX, cls.HEAD_JOINTS_IDX)]
        cols += [((vt - vp) ** 2).mean(dim=(1, 2)), th.zeros_like(cols[0]), th.zeros_like(cols[0])]
        return th.stack(cols, dim=1)

    def training_losses(self, model, x_start, t, model_kwargs=None, noise=None, noise_seed=None):
        """gaussian_diffusion.py:1002-1090 as an evaluator (no_grad): the reference's keys with the reference's shapes - "mse" [B],
        "velocity_body", "velocity_elbow", "velocity_head", "velocity" (0-dim), "target" and "pred" [B, T, 26] - plus "terms" [B, 8],
        the per-clip numbers they are means of (include/dc_ddim.h, dc_motion_loss_terms; its masked reconstruction sum reads
        model_kwargs["length"], all T without one).  x_start [B, T, 13, 2] as in the reference; [B, T, 26] is accepted as well.
        The target is x_start (START_X), the noise (EPSILON) or the posterior mean (PREVIOUS_X).
        `noise_seed` (extension, GPU only): as q_sample.  With this package's MotionTransformer on a GPU the noising and the
        reductions are libdc_ddim's kernels; with any other callable or device the same definitions in plain torch.
        NotImplementedError: LossType.KL / RESCALED_KL and learned variances (the variational bound as a training objective is out of
        scope; calc_bpd_loop scores it).
        ValueError: T < 2 - the velocity means run over no elements there and the reference returns NaN."""
        if self.loss_type.is_vb():
            raise NotImplementedError(f"{self.loss_type}: the variational bound is out of scope; LossType.MSE / RESCALED_MSE only")
        if self.model_var_type in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE):
            raise NotImplementedError(f"{self.model_var_type}: a learned variance adds the variational-bound term, which is out of scope")
        if self.loss_type not in (LossType.MSE, LossType.RESCALED_MSE):
            raise NotImplementedError(self.loss_type)
        mk = {} if model_kwargs is None else model_kwargs
        x = th.as_tensor(x_start)
        if x.dim() not in (3, 4) or x[0, 0].numel() != 26:
            raise ValueError(f"x_start must be [B, T, 13, 2] or [B, T, 26], got {tuple(x.shape)}")
        B, T = int(x.shape[0]), int(x.shape[1])
        if T < 2:
            raise ValueError(f"T = {T}: the velocity terms are means over T - 1 frames; the reference returns NaN for them at T = 1")
        on_gpu = x.is_cuda and isinstance(model, MotionTransformer)
        with th.no_grad():
            x = x.to(th.float32).contiguous()
            t = th.as_tensor(t).to(x.device).long()
            drawn = None
            if on_gpu and noise is None and noise_seed is not None:
                a, s = native.q_sample_coefficients(self.alphas_cumprod, t)
                if self.model_mean_type == ModelMeanType.EPSILON:
                    x_t, drawn = native.q_sample(x, a, s, noise_seed=noise_seed, return_noise=True)
                else:
                    x_t = native.q_sample(x, a, s, noise_seed=noise_seed)
            else:
                if noise is None and noise_seed is not None:
                    raise ValueError("noise_seed= draws on the device (a MotionTransformer on a GPU); pass noise= here")
                drawn = th.randn_like(x) if noise is None else th.as_tensor(noise).to(device=x.device, dtype=th.float32).reshape(x.shape).contiguous()
                x_t = self.q_sample(x, t, noise=drawn)
            model_output = model(x_t, self._scale_timesteps(t), **mk)
            if self.model_mean_type == ModelMeanType.PREVIOUS_X:
                target = self.q_posterior_mean_variance(x_start=x, x_t=x_t, t=t)[0]
            elif self.model_mean_type == ModelMeanType.START_X:
                target = x
            elif self.model_mean_type == ModelMeanType.EPSILON:
                target = drawn
            else:
                raise NotImplementedError(self.model_mean_type)
            target = target.reshape(B, T, 26).contiguous()
            pred = th.as_tensor(model_output).to(th.float32).reshape(B, T, 26).contiguous()
            length = mk.get("length")
            terms = native.motion_loss_terms(pred, target, length) if on_gpu else self.loss_terms_torch(pred, target, length)
        return {"mse": terms[:, 0], "velocity_body": terms[:, 2].mean(), "velocity_elbow": terms[:, 3].mean(),
                "velocity_head": terms[:, 4].mean(), "velocity": terms[:, 5].mean(), "target": target, "pred": pred, "terms": terms}

    # ---- the variational bound, as a score ------------------------------------------------
    def q_mean_variance(self, x_start, t):
        """gaussian_diffusion.py:381-396: (mean, variance, log_variance) of q(x_t | x_0)."""
        mean = _extract(self.sqrt_alphas_cumprod, t, x_start.shape) * x_start
        return mean, _extract(1.0 - self.alphas_cumprod, t, x_start.shape), _extract(self.log_one_minus_alphas_cumprod, t, x_start.shape)

    def vb_terms_torch(self, x_start, x_t, t, out, noise=None):
        """native.vb_terms in plain torch (fp32, any device) from `out` = p_mean_variance's dict: [B, 8] per clip - output, kl,
        decoder_nll (bits), xstart_mse, mse (0 without `noise`), 0, 0, 0 (include/dc_ddim.h, dc_vb_terms)."""
        true_mean, _, true_log_variance_clipped = self.q_posterior_mean_variance(x_start=x_start, x_t=x_t, t=t)
        kl = mean_flat(normal_kl(true_mean, true_log_variance_clipped, out["mean"], out["log_variance"])) / np.log(2.0)
        decoder_nll = -discretized_gaussian_log_likelihood(x_start, means=out["mean"], log_scales=0.5 * out["log_variance"])
        assert decoder_nll.shape == x_start.shape
        decoder_nll = mean_flat(decoder_nll) / np.log(2.0)
        cols = [th.where((t == 0), decoder_nll, kl), kl, decoder_nll, mean_flat((out["pred_xstart"] - x_start) ** 2)]
        zero = th.zeros_like(kl)
        cols.append(zero if noise is None else mean_flat((self._predict_eps_from_xstart(x_t, t, out["pred_xstart"]) - noise) ** 2))
        return th.stack(cols + [zero, zero, zero], dim=1)

    def _vb_terms_bpd(self, model, x_start, x_t, t, clip_denoised=True, model_kwargs=None, *, denoised_fn=None, noise=None):
        """gaussian_diffusion.py:967-1000: {"output": [N] NLLs (t == 0) or KLs in bits, "pred_xstart"}, plus the extension key "terms"
        [N, 8] (include/dc_ddim.h, dc_vb_terms: output, kl, decoder_nll, xstart_mse, mse, 0, 0, 0).  On GPU tensors the model call is
        followed by ONE fused pass over x_start, x_t and the model's output (native.vb_terms); on the host, or with `denoised_fn`
        (extension: p_mean_variance's), the same definitions in plain torch.  `noise` (extension): the draw x_t was noised with - fills
        "terms"[:, 4], calc_bpd_loop's epsilon error.  `t` may stay on the host beside GPU tensors: nothing then waits for the device."""
        x = th.as_tensor(x_start)
        t = th.as_tensor(t).long()
        with th.no_grad():
            if not x.is_cuda or denoised_fn is not None:
                t = t.to(x.device)
                out = self.p_mean_variance(model, x_t, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn, model_kwargs=model_kwargs)
                terms = self.vb_terms_torch(x, x_t, t, out, noise)
                return {"output": terms[:, 0], "pred_xstart": out["pred_xstart"], "terms": terms}
            x = x.to(th.float32).contiguous()
            xt = th.as_tensor(x_t).to(device=x.device, dtype=th.float32).contiguous()
            t_host = t.cpu()
            # (this package's denoiser reads its timesteps on the host; any other callable gets them where the reference puts them)
            model_output, var_values = self._model_output(model, xt, t_host if isinstance(model, MotionTransformer) else t.to(x.device),
                                                          model_kwargs)
            model_output = th.as_tensor(model_output).to(th.float32).contiguous()
            coef = native.vb_coefficients(self.betas, self.model_var_type, t_host)
            terms = native.vb_terms(x, xt, model_output.reshape(x.shape), coef, self.model_mean_type, self.model_var_type, clip_denoised,
                                    var_values=None if var_values is None else var_values.to(th.float32).contiguous().reshape(x.shape),
                                    noise=None if noise is None else th.as_tensor(noise).to(device=x.device, dtype=th.float32).contiguous())
            pred_xstart = self._xstart_of(model_output.reshape(xt.shape), xt, t_host, clip_denoised, None)
        return {"output": terms[:, 0], "pred_xstart": pred_xstart, "terms": terms}

    def _prior_bpd(self, x_start):
        """gaussian_diffusion.py:1092-1108: the prior term of the bound, KL(q(x_T | x_0) || N(0, I)) in bits per dimension, [N]."""
        x = th.as_tensor(x_start)
        B = int(x.shape[0])
        if x.is_cuda:
            S = self.num_timesteps
            return native.prior_kl(x.to(th.float32).contiguous(), np.full(B, np.float32(self.sqrt_alphas_cumprod[S - 1])),
                                   np.full(B, np.float32(self.log_one_minus_alphas_cumprod[S - 1])))
        t = th.tensor([self.num_timesteps - 1] * B, device=x.device)
        qt_mean, _, qt_log_variance = self.q_mean_variance(x, t)
        return mean_flat(normal_kl(mean1=qt_mean, logvar1=qt_log_variance, mean2=0.0, logvar2=0.0)) / np.log(2.0)

    def calc_bpd_loop(self, model, x_start, clip_denoised=True, model_kwargs=None, *, noise_seed=None, timesteps=None):
        """gaussian_diffusion.py:1110-1165: the whole variational bound in bits per dimension - ONE model evaluation per timestep of the
        schedule, from S - 1 down to 0.  Returns "total_bpd" [N], "prior_bpd" [N], "vb" [N, S], "xstart_mse" [N, S], "mse" [N, S]
        (columns in the loop's order: column 0 is t = S - 1).  With GPU tensors the noising is dc_q_sample and what follows each
        evaluation is dc_vb_terms; nothing in the loop waits for the device.
        `noise_seed` (extension, GPU only): step t's noise is the library's draw (seed, iteration = t) in place of th.randn_like.
        `timesteps` (extension): evaluate only these timesteps; the K columns are in descending order of t, and "total_bpd" is None -
        the sum needs every term."""
        x = th.as_tensor(x_start)
        B, S = int(x.shape[0]), self.num_timesteps
        if timesteps is None:
            ts = list(range(S))[::-1]
        else:
            ts = sorted({int(v) for v in np.asarray(timesteps).reshape(-1)}, reverse=True)
            if not ts or ts[0] >= S or ts[-1] < 0:
                raise ValueError(f"timesteps must be inside [0, {S}), got {ts}")
        if noise_seed is not None and not x.is_cuda:
            raise ValueError("noise_seed= draws on the device; on the host the noise is th.randn_like's")
        if x.is_cuda:
            x = x.to(th.float32).contiguous()
        terms = []
        for t in ts:
            t_batch = th.full((B,), t, dtype=th.long)      # on the host: the tables are gathered there
            if x.is_cuda:
                a, s = native.q_sample_coefficients(self.alphas_cumprod, t_batch)
                if noise_seed is not None:
                    x_t, noise = native.q_sample(x, a, s, noise_seed=(noise_seed, t, 0), return_noise=True)
                else:
                    noise = th.randn_like(x)
                    x_t = native.q_sample(x, a, s, noise=noise)
            else:
                noise = th.randn_like(x)
                x_t = self.q_sample(x_start=x, t=t_batch, noise=noise)
            terms.append(self._vb_terms_bpd(model, x_start=x, x_t=x_t, t=t_batch, clip_denoised=clip_denoised, model_kwargs=model_kwargs,
                                            noise=noise)["terms"])
        terms = th.stack(terms, dim=1)      # [N, K, 8]
        vb, prior_bpd = terms[:, :, 0], self._prior_bpd(x)
        return {"total_bpd": vb.sum(dim=1) + prior_bpd if timesteps is None else None, "prior_bpd": prior_bpd, "vb": vb,
                "xstart_mse": terms[:, :, 3], "mse": terms[:, :, 4]}

    # ---- DDIM ---------------------------------------------------------------------------
    def ddim_sample(self, model, x, t, clip_denoised=True, denoised_fn=None, cond_fn=None, model_kwargs=None,
                    eta=0.0, noise=None):
        """gaussian_diffusion.py:783-831.  `noise` (extension): the draw to use in place of th.randn_like(x)."""
        pred_xstart = self._pred_xstart(model, x, t, clip_denoised, denoised_fn, model_kwargs)
        if cond_fn is not None:
            pred_xstart = self.condition_score(cond_fn, {"pred_xstart": pred_xstart}, x, t, model_kwargs=model_kwargs)["pred_xstart"]
        eps = self._predict_eps_from_xstart(x, t, pred_xstart)
        alpha_bar = _extract(self.alphas_cumprod, t, x.shape)
        alpha_bar_prev = _extract(self.alphas_cumprod_prev, t, x.shape)
        sigma = eta * th.sqrt((1 - alpha_bar_prev) / (1 - alpha_bar)) * th.sqrt(1 - alpha_bar / alpha_bar_prev)
        mean_pred = pred_xstart * th.sqrt(alpha_bar_prev) + th.sqrt(1 - alpha_bar_prev - sigma ** 2) * eps
        sample = mean_pred
        if eta != 0.0:
            noise = th.randn_like(x) if noise is None else noise.to(x)
            nonzero_mask = (t != 0).float().view(-1, *([1] * (len(x.shape) - 1)))
            sample = mean_pred + nonzero_mask * sigma * noise
        return {"sample": sample, "pred_xstart": pred_xstart}

    def _refuse_epsilon_full_attention(self, model, eta):
        """EPSILON model x full attention (`no_eff`) x eta = 0 is outside the 1e-3 parity bound on some loops (2.3e-4 ... 1.26e-3 over 14
        randomized loops of tools/fuzz_sampler.py: the attention's scores, weights and values stay plain fp16 even in the split
        evaluations, and a deterministic EPSILON chain keeps every evaluation's error in x_t).  Refused instead of returned; the library
        refuses the captured loop likewise (DC_ERR_UNSUPPORTED)."""
        import os
        if (isinstance(model, MotionTransformer) and getattr(getattr(model, "cfg", None), "no_eff", False) and self.model_mean_type == ModelMeanType.EPSILON
                and float(eta) == 0.0 and not os.environ.get("DC_ALLOW_EPSILON_NO_EFF_ETA0")):
            raise ValueError("an EPSILON model with full attention (no_eff) at eta = 0 is outside the 1e-3 parity bound of this "
                             "implementation (up to 1.3e-3); use linear attention, or eta > 0")

    def _fast_path_ok(self, model, denoised_fn, cond_fn):
        return (isinstance(model, MotionTransformer)
                and self.model_mean_type in (ModelMeanType.START_X, ModelMeanType.EPSILON)
                and self.model_var_type in (ModelVarType.FIXED_SMALL, ModelVarType.FIXED_LARGE)
                and denoised_fn is None and cond_fn is None and not self.rescale_timesteps)

    def native_coefficients(self, eta=None):
        """eta None: the [S, 4] table of dc_ddim_coefficients (eta = 0); a float: the [S, 8] table of dc_ddim_coefficients_ex."""
        key = None if eta is None else float(eta)
        if self._native_coef is None:
            self._native_coef = {}
        if key not in self._native_coef:
            self._native_coef[key] = native.ddim_coefficients(self.alphas_cumprod, key)
        return self._native_coef[key]

    def native_coefficients_known(self, eta=0.0):
        """The [S, 8] table of dc_ddim_coefficients_known (loops around known values)."""
        key = ("known", float(eta))
        if self._native_coef is None:
            self._native_coef = {}
        if key not in self._native_coef:
            self._native_coef[key] = native.ddim_coefficients_known(self.alphas_cumprod, float(eta))[0]
        return self._native_coef[key]

    @staticmethod
    def _known_tensors(img, known, known_mask, known_noise, known_noise_seed):
        """The three fp32 [B, T, P] device tensors of NativeSampler.set_known from the keywords of ddim_sample_loop, or None."""
        if known is None and known_mask is None:
            if known_noise is not None:
                raise ValueError("known_noise= without known= and known_mask=")
            return None
        if known is None:
            raise ValueError("known_mask= without known=: a mask needs the values it marks")
        if known_mask is None:
            raise ValueError("known= without known_mask=: say which elements are known")
        shape = tuple(img.shape)

        def full(t, name):
            t = th.as_tensor(t).to(device=img.device, dtype=th.float32)
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
            return t.contiguous()
        m = th.as_tensor(known_mask).to(device=img.device)
        if m.dim() == 2:
            m = m.unsqueeze(-1)
        if m.dim() != 3 or tuple(m.shape[:2]) != shape[:2] or m.shape[2] not in (1, shape[2]):
            raise ValueError(f"known_mask must be {shape[:2]}, {shape[:2] + (1,)} or {shape}, got {tuple(th.as_tensor(known_mask).shape)}")
        m = (m != 0).to(th.float32).expand(shape).contiguous()
        if known_noise is None:
            g = None
            if known_noise_seed is not None:
                g = th.Generator()
                g.manual_seed(int(known_noise_seed))
            known_noise = th.randn(shape, generator=g)
        return full(known, "known"), m, full(known_noise, "known_noise")

    def _check_guidance(self, model, guidance_scale, denoised_fn, cond_fn, stepped=False):
        """guidance_scale= runs inside the captured loop only: ValueError where the loop would step through ddim_sample."""
        if guidance_scale is None:
            return
        why = ("the progressive generator" if stepped else "denoised_fn" if denoised_fn is not None else "cond_fn" if cond_fn is not None else
               "the PREVIOUS_X parameterisation" if self.model_mean_type == ModelMeanType.PREVIOUS_X else
               "a learned-variance model" if self.model_var_type in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE) else
               None if self._fast_path_ok(model, denoised_fn, cond_fn) else "this model / rescale_timesteps")
        if why is not None:
            raise ValueError(f"guidance_scale= is combined inside the captured loop; {why} steps through ddim_sample, where the caller "
                             "combines the two evaluations")
        if not math.isfinite(float(guidance_scale)):
            raise ValueError(f"guidance_scale must be finite, got {guidance_scale!r}")

    def _check_takes(self, model, takes, shape, model_kwargs, denoised_fn, cond_fn, stepped=False):
        """takes= runs inside the native loop only, over takes x the musics of model_kwargs: ValueError otherwise."""
        if int(takes) != takes or int(takes) < 1:
            raise ValueError(f"takes must be an integer >= 1, got {takes!r}")
        takes = int(takes)
        if takes == 1:
            return 1
        if stepped or not self._fast_path_ok(model, denoised_fn, cond_fn):
            raise ValueError("takes= share their conditioning inside the native loop; "
                             f"{'the progressive generator' if stepped else 'this call'} steps through ddim_sample - tile the music instead")
        mk = model_kwargs or {}
        ref = mk.get("xf_proj") if mk.get("xf_proj") is not None else mk.get("text")
        if ref is not None and int(shape[0]) != takes * int(ref.shape[0]):
            raise ValueError(f"shape[0]={shape[0]} must be takes x musics = {takes} x {int(ref.shape[0])}")
        return takes

    def _check_windows(self, model, window_starts, window_weights, shape, model_kwargs, takes, denoised_fn, cond_fn, stepped=False):
        """window_starts= / window_weights= blend the windows of longer pieces inside the native loop: None when neither was given
        (today's loop), else (starts, weights fp32 [W, T], L) after the checks the host can make; ValueError where the call would step
        through ddim_sample, with takes, and for features or a plan that do not fit `shape` = (B, L, P)."""
        if window_starts is None and window_weights is None:
            return None
        if window_starts is None or window_weights is None:
            raise ValueError("window_starts= and window_weights= come together (harness.window_weights makes the weights of a plan)")
        if stepped or not self._fast_path_ok(model, denoised_fn, cond_fn):
            raise ValueError("window_starts= blends the windows inside the native loop's update; "
                             f"{'the progressive generator' if stepped else 'this call'} steps through ddim_sample, where there is no such step")
        if takes != 1:
            raise ValueError("windows do not combine with takes")
        starts = [int(s) for s in np.asarray(window_starts).reshape(-1)]
        weights = np.ascontiguousarray(np.asarray(window_weights.cpu() if th.is_tensor(window_weights) else window_weights), np.float32)
        B, L = int(shape[0]), int(shape[1])
        mk = model_kwargs or {}
        ref = mk.get("xf_proj") if mk.get("xf_proj") is not None else mk.get("text")
        if weights.ndim != 2 or weights.shape[0] != len(starts):
            raise ValueError(f"window_weights must be [W, T] for the {len(starts)} window_starts, got {weights.shape}")
        T = int(weights.shape[1])
        if ref is not None and int(ref.shape[0]) != len(starts) * B:
            raise ValueError(f"the features hold {int(ref.shape[0])} rows, not W x B = {len(starts)} x {B} windows (window-major)")
        if mk.get("xf_proj") is not None and int(mk["xf_proj"].shape[1]) != T:
            raise ValueError(f"the features hold windows of {int(mk['xf_proj'].shape[1])} frames, the weights of {T}")
        ln = mk.get("length")
        if ln is not None and any(int(v) != T for v in (ln.tolist() if hasattr(ln, "tolist") else ln)):
            raise ValueError("windows are full: model_kwargs['length'] must be left out (or all T) with window_starts=")
        native.windows_check(starts, weights, T, L)
        return starts, weights, L

    def _solver_timesteps(self, model, steps, spacing, timesteps, solver, eta, denoised_fn, cond_fn, stepped=False):
        """The list of a loop on a sub-sequence (steps= / timesteps= / solver=), or None when none of them was given (today's loop).
        Such a loop runs natively only: ValueError where the call would step through ddim_sample, as for guidance_scale=."""
        if steps is None and timesteps is None and solver == "ddim":
            return None
        if solver not in native.SOLVER_ORDER:
            raise ValueError(f"solver must be one of {sorted(native.SOLVER_ORDER)}, got {solver!r}")
        why = ("the progressive generator" if stepped else "denoised_fn" if denoised_fn is not None else "cond_fn" if cond_fn is not None else
               "the PREVIOUS_X parameterisation" if self.model_mean_type == ModelMeanType.PREVIOUS_X else
               "a learned-variance model" if self.model_var_type in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE) else
               None if self._fast_path_ok(model, denoised_fn, cond_fn) else "this model / rescale_timesteps")
        if why is not None:
            raise ValueError(f"steps= / timesteps= / solver= run inside the native loop; {why} steps through ddim_sample, which walks "
                             "every timestep with the first-order update")
        if solver == "dpmpp2m" and float(eta) != 0.0:
            raise ValueError("solver='dpmpp2m' is deterministic: eta must be 0")
        if timesteps is None:
            return spaced_timesteps(self.alphas_cumprod, self.num_timesteps if steps is None else steps, spacing)
        ts = [int(t) for t in np.asarray(timesteps).reshape(-1)]
        if steps is not None and int(steps) != len(ts):
            raise ValueError(f"steps={steps} beside a list of {len(ts)} timesteps")
        if not ts or any(not 0 <= t < self.num_timesteps for t in ts) or any(b >= a for a, b in zip(ts, ts[1:])):
            raise ValueError(f"timesteps must be a strictly decreasing list inside [0, {self.num_timesteps})")
        return ts

    def _native_loop(self, model, img, mk, clip_denoised, eta, snap, step_noise, smooth=None, step_noise_seed=None, known=None,
                     guidance_scale=None, timesteps=None, solver="ddim", takes=1, windows=None):
        """The captured loop on `model`'s sampler; returns (out, snaps).  Numeric health is checked once per call
        (`model.check_numerics`): a non-finite x0 under precision="auto" falls back to the bf16-range mode in a fresh sampler.
        `timesteps` (a list) runs dc_sampler_solver_loop on it with `solver`'s table; None the loop over every timestep."""
        flags = (native.UPDATE_CLIP_DENOISED if clip_denoised else 0) | \
            (native.UPDATE_EPSILON if self.model_mean_type == ModelMeanType.EPSILON else 0)
        z, zseed = None, None
        if eta != 0.0:
            if step_noise is not None:
                shape = (self.num_timesteps if timesteps is None else len(timesteps),) + tuple(img.shape)
                z = step_noise.to(device=img.device, dtype=th.float32).contiguous()
                assert tuple(z.shape) == shape, f"step_noise must be {shape}"
            elif step_noise_seed is not None:
                zseed = step_noise_seed
            else:
                # the reference draws th.randn_like(x) once per step (gaussian_diffusion.py:822); so does the library, at the head
                # of each step, from a seed taken off torch's default generator (torch.manual_seed makes a run reproducible) -
                # never the whole [S, B, T, P] tensor up front (6 GB at S = 1000, bs = 32).  Ranks of a sharded run that seed
                # torch alike must pass step_noise_seed=(seed, lo*T*P) instead, or every shard would add the same draws.
                zseed = int(th.randint(0, 2 ** 62, (1,)).item())
        plain = flags == 0 and eta == 0.0
        # (An EPSILON model's final sample carries what the evaluations left in x_t: the library runs EVERY evaluation of such a loop on
        # split operands - in the fp16 and bf16 precisions, linear and (fp16) full attention alike (dc_ddim.h, dc_sampler_set_precise_tail; the bf16
        # precision's split evaluations take the FiLM GEMM's operands in fp16).)
        if timesteps is not None:      # (the rows carry the known slots: one table serves loops with and without known values)
            coef = native.solver_table(self.alphas_cumprod, timesteps, eta, native.SOLVER_ORDER[solver])[0]
        else:
            coef = self.native_coefficients(None if plain else eta) if known is None else self.native_coefficients_known(eta)
        retried = False
        while True:
            tk = {} if takes == 1 else {"takes": takes}      # (one take: the model is called as before)
            if windows is not None:      # (_check_windows: the windows are full, the lengths stay out)
                nat = model.set_conditioning(mk["xf_proj"], mk["xf_out"], None, guided=guidance_scale is not None, windows=windows)
                if guidance_scale is not None:
                    nat.set_guidance_scale(guidance_scale)
            elif guidance_scale is None:
                nat = model.set_conditioning(mk["xf_proj"], mk["xf_out"], mk.get("length"), **tk)
            else:        # (inside the retry loop: precision="auto"'s re-run on a fresh sampler keeps the scale)
                nat = model.set_conditioning(mk["xf_proj"], mk["xf_out"], mk.get("length"), guided=True, **tk)
                nat.set_guidance_scale(guidance_scale)
            nat.set_smoothing(*(smooth if smooth else (0, 0)))
            nat.set_known(*(known if known is not None else (None, None, None)))
            if timesteps is not None:
                out, snaps = nat.solver_loop(img, timesteps, coef, snap, flags, z, zseed)
            else:
                out, snaps = nat.ddim_loop(img, coef, snap, flags, z, zseed)
            if not getattr(model, "check_numerics", True):
                return out, snaps
            st = nat.status()
            if st == 0:
                return out, snaps
            if (st & native.STATUS_TIMEOUT) and not retried:
                # small batches: the clip's workgroups exchange their combine slices inside a layer launch and one of them gave up
                # waiting (the GPU is shared with other work, so they were not co-resident).  Whatever else that void run reported
                # does not count; reading the status has latched the form without the exchange on this sampler: run the loop again
                warnings.warn("libdc_ddim: in-launch combine exchange timed out (GPU shared?); this sampler continues without the exchange")
                retried = True
                continue
            if not model.numerics_fallback(st):
                raise FloatingPointError(native.describe_status(st, model.active_precision))

    def ddim_sample_loop(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None, cond_fn=None,
                         model_kwargs=None, device=None, progress=False, eta=0.0, idxs=[], step_noise=None, smooth=None,
                         step_noise_seed=None, known=None, known_mask=None, known_noise=None, known_noise_seed=None,
                         guidance_scale=None, steps=None, spacing="uniform", timesteps=None, solver="ddim", takes=1,
                         window_starts=None, window_weights=None):
        """gaussian_diffusion.py:871-915.  Returns the final sample, or when `idxs` is non-empty a
        dict {iteration: sample} for the listed iterations plus {num_timesteps: final}.
        `steps`, `spacing`, `timesteps`, `solver` (extension, native loop only; none given = today's loop over every timestep, bit for
        bit): sample on a sub-sequence of the schedule's timesteps - `timesteps`, a strictly decreasing list, or `steps` of them picked
        by spaced_timesteps(alphas_cumprod, steps, spacing) - with the first-order update (solver="ddim") or the second-order
        multistep one (solver="dpmpp2m": DPM-Solver++ 2M on the predicted x0, eta = 0 only, no extra model evaluation; use
        spacing="logsnr" with it, see spaced_timesteps).  The model sees the original timestep numbers.  `idxs` then count iterations
        of that loop, the final key is len(timesteps), and `step_noise` is [n, B, T, P].  Neither exists in the reference.  ValueError
        with denoised_fn, cond_fn, PREVIOUS_X or a learned variance (they step through ddim_sample), and for dpmpp2m with eta != 0.
        `step_noise` (extension, eta > 0): [S, B, T, P], the draw for iteration i in place of th.randn_like.
        `step_noise_seed` (extension, eta > 0, native loop only): seed of the library's own per-step draws, or (seed, first_element)
        for a shard that holds clips [lo, hi) of a larger batch (first_element = lo*T*P: the rows the whole batch's draw gives them).
        `smooth` (extension): (window, order) of the Savitzky-Golay filter tools/visualization.py:126 applies to the result,
        folded into the loop's final write (native loop only).
        `known`, `known_mask`, `known_noise` (extension, native loop only): sample AROUND known values.  `known` [B, T, P]; `known_mask`
        [B, T], [B, T, 1] or [B, T, P], nonzero = this element is known; `known_noise` [B, T, P], ONE fixed draw per element (None:
        drawn once from torch's default generator, or from `known_noise_seed`).  At every noise level abar the known elements are held
        at sqrt(abar) known + sqrt(1 - abar) known_noise - x_T and every x_{t-1}, snapshots included - so the final sample equals
        `known` bit for bit there (before `smooth`); eta > 0 noise, clipping and the EPSILON update act on the other elements only
        (include/dc_ddim.h, dc_sampler_set_known).
        `guidance_scale` (extension, native loop only; None = no guidance, today's loop bit for bit): classifier-free guidance at
        scale w - every step evaluates the model on the music and on the model's null_conditioning() and continues from
        c + (w - 1)(c - u) (include/dc_ddim.h, dc_sampler_set_conditioning_guided; the reference trains for it, transformer.py:389,
        451-459, and never samples with it).  ValueError with denoised_fn, cond_fn, PREVIOUS_X or a learned variance.
        `takes` (extension, native loop only; 1 = today's loop): samples per music.  `model_kwargs` holds B musics and `shape[0]` must be
        takes * B (ValueError otherwise): clip j * B + b of `noise`, of the result and of every other [.., T, P] argument is take j of
        music b.  The takes share each step's FiLM tiles (include/dc_ddim.h, dc_sampler_set_conditioning_takes); the result equals the
        loop over the music tiled `takes` times, bit for bit.  ValueError where the loop would step through ddim_sample.
        `window_starts`, `window_weights` (extension, native loop only; neither given = today's loop): sample pieces LONGER than the
        model's window in one loop.  `shape` is (B, L, P) - and so are `noise`, the result, `idxs` snapshots, `step_noise` per
        iteration and the known tensors -; `model_kwargs` holds the features of the W x B windows, [W * B, T, 64], window-major (row
        k * B + b: window k of piece b, frames [window_starts[k], window_starts[k] + T) of it); `window_weights` fp32 [W, T] are the
        blend weights (harness.window_weights).  At every step the model's predictions are blended over the windows that cover a
        frame before the update (include/dc_ddim.h, dc_sampler_set_conditioning_windows).  ValueError for a plan the library
        refuses, with takes, and where the loop would step through ddim_sample."""
        self._check_guidance(model, guidance_scale, denoised_fn, cond_fn)
        takes = self._check_takes(model, takes, shape, model_kwargs, denoised_fn, cond_fn)
        windows = self._check_windows(model, window_starts, window_weights, shape, model_kwargs, takes, denoised_fn, cond_fn)
        ts = self._solver_timesteps(model, steps, spacing, timesteps, solver, eta, denoised_fn, cond_fn)
        n_iter = self.num_timesteps if ts is None else len(ts)
        self._refuse_epsilon_full_attention(model, eta)
        if self._fast_path_ok(model, denoised_fn, cond_fn):
            if device is None:
                device = next(model.parameters()).device
            assert isinstance(shape, (tuple, list))
            img = noise if noise is not None else th.randn(*shape, device=device)
            img = img.to(device=device, dtype=th.float32).contiguous()
            mk = model_kwargs or {}
            if mk.get("xf_proj") is None or mk.get("xf_out") is None:
                mk = dict(mk)
                mk["xf_proj"], mk["xf_out"] = model.encode_music(mk["text"], device)
            snap = sorted(int(i) for i in set(idxs) if 0 <= int(i) < n_iter)
            kn = self._known_tensors(img, known, known_mask, known_noise, known_noise_seed)
            out, snaps = self._native_loop(model, img, mk, bool(clip_denoised), float(eta), snap, step_noise, smooth, step_noise_seed, kn,
                                            guidance_scale, ts, solver, takes, windows)
            if len(idxs) == 0:
                return out
            result = {it: snaps[k] for k, it in enumerate(snap)}
            result[n_iter] = out
            return result
        if known is not None or known_mask is not None or known_noise is not None:
            raise NotImplementedError("known= / known_mask= are replaced inside the native loop's update; with host callbacks "
                                      "(denoised_fn, cond_fn) or another model there is no step to replace them in")
        if smooth:
            raise NotImplementedError("smooth= is folded into the native loop's final write; with host callbacks apply evaluate.smooth_motion")
        final, i, result = None, 0, {}
        for sample in self.ddim_sample_loop_progressive(model, shape, noise=noise, clip_denoised=clip_denoised,
                                                        denoised_fn=denoised_fn, cond_fn=cond_fn,
                                                        model_kwargs=model_kwargs, device=device,
                                                        progress=progress, eta=eta, step_noise=step_noise):
            final = sample
            if i in idxs:
                result[i] = sample["sample"]
            i += 1
        result[i] = final["sample"]
        if len(idxs) == 0:
            return final["sample"]
        return result

    # the north-star wording calls the entry point `GaussianDiffusion.sample`
    sample = ddim_sample_loop

    def ddim_sample_loop_progressive(self, model, shape, noise=None, clip_denoised=True, denoised_fn=None,
                                     cond_fn=None, model_kwargs=None, device=None, progress=False, eta=0.0,
                                     step_noise=None, guidance_scale=None, steps=None, spacing="uniform", timesteps=None, solver="ddim",
                                     takes=1, window_starts=None, window_weights=None):
        """gaussian_diffusion.py:917-965: yields {"sample","pred_xstart"} after every step.  `guidance_scale`, `steps`, `timesteps`,
        `solver`, `takes`, `window_starts`, `window_weights`: the defaults only - this generator steps through ddim_sample (ValueError otherwise; ddim_sample_loop guides, and
        samples on a sub-sequence, inside the captured loop)."""
        self._check_guidance(model, guidance_scale, denoised_fn, cond_fn, stepped=True)
        self._check_takes(model, takes, shape, model_kwargs, denoised_fn, cond_fn, stepped=True)
        self._check_windows(model, window_starts, window_weights, shape, model_kwargs, takes, denoised_fn, cond_fn, stepped=True)
        self._solver_timesteps(model, steps, spacing, timesteps, solver, eta, denoised_fn, cond_fn, stepped=True)
        self._refuse_epsilon_full_attention(model, eta)
        if device is None:
            device = next(model.parameters()).device
        assert isinstance(shape, (tuple, list))
        img = noise if noise is not None else th.randn(*shape, device=device)
        indices = list(range(self.num_timesteps))[::-1]
        if progress:
            from tqdm.auto import tqdm
            indices = tqdm(indices)
        # The update of an EPSILON / PREVIOUS_X model, and a conditioned score, keep what the evaluations' 16-bit operands left in x_t
        # (fp16, EPSILON, eta = 0: 1.5e-3 on plain operands): these loops evaluate the native denoiser on split operands
        precise = isinstance(model, MotionTransformer) and (self.model_mean_type != ModelMeanType.START_X or cond_fn is not None)
        before = model.precise_forward if precise else None
        if precise:
            model.precise_forward = True
        try:
            for it, i in enumerate(indices):
                t = th.full((shape[0],), i, device=device, dtype=th.long)
                with th.no_grad():
                    out = self.ddim_sample(model, img, t, clip_denoised=clip_denoised, denoised_fn=denoised_fn,
                                           cond_fn=cond_fn, model_kwargs=model_kwargs, eta=eta,
                                           noise=None if step_noise is None else step_noise[it])
                    yield out
                    img = out["sample"]
        finally:
            if precise:
                model.precise_forward = before
