"""Shared by tests/test_host_vb.py, tests/test_gpu_vb.py and tools/make_golden_vb.py: the cases of the variational bound, their
inputs from seeds, and the float64 oracle of the five slots of dc_vb_terms (include/dc_ddim.h) with the bound each slot may miss it by.

Inputs.  The decoder likelihood is meaningful in fp32 in two regimes only.  With z = (x0 - mean) / sigma: for |z| <= 2.5 fp32 and fp64
agree to 3e-4 per element, for |z| >= 8 both clamp the probability to 1e-12; between them fp32 tanh's last bit decides whether
cdf_plus - cdf_min is 0 or 6e-8, which is 11 nats.  `make_case` therefore BUILDS every element into one of the two regimes (both in
every clip) by solving for x_t (or, at t = 0 where the mean does not read x_t, for the model's output), and `band` counts the elements
in between: the tests assert it is 0 before any kernel runs.

Oracle.  pred_xstart and the two posterior means are AFFINE fp32 expressions of the inputs (products and sums, never contracted): their
bits are the same in numpy float32, in torch and in the kernel, so `stages_fp32` forms them in fp32 and `oracle` takes everything
behind them - differences, squares, exp, tanh, log, the means - in float64.  (m1 - m2 cancels: its error relative to the RESULT is
(|m1| + |m2|) / |m1 - m2| roundings, which no count of roundings covers and which is the reference's own number.)

Bounds, per element, with u = 2^-24 and K = 32 the roundings on an element's path behind those stages (counted in csrc/dc_loss.hip:
kl 17, nll at most 33 of which the learned-range log-variance's 5 are shared; an expf / logf / tanhf counts 2, HIP documents 1 ULP):
  kl    K u 1/2 (1 + |lv2 - lv1| + e^(lv1 - lv2) + (m1 - m2)^2 e^-lv2)
  nll   min(K u (1 / delta + |log delta|), 27.64), delta the oracle's clamped probability (27.64 > -log 1e-12: the clamp's range);
        tighter where BOTH cdf arguments are beyond +-7 on one side: tanh's argument is then beyond 0.798 (7 + 0.0447 7^3) = 17.8, and
        fp32 tanh is exactly +-1 from 9.02 on (where 1 - 2 e^-2x rounds to 1), so both cdfs are exactly 0 or exactly 1, the kernel's
        probability is exactly 0 (clamped: log 1e-12) or exactly 1 (log 1 = 0), and the element misses the oracle by the clamp
        constant's and logf's roundings only: K u (1 + |log delta|)
  x0    e = pred - x0: one rounding, squared, one more: 3 u e^2 (1 + 2 u)
  eps   de = eps - noise with eps = num / rm1 one rounding of its own: |d de| <= u (|eps| + |de|), through the square
        2 |de| |d de| + |d de|^2 + u de^2
A clip's bound is the mean of its elements' bounds plus (chain + DEPTH + 3) u times the mean of the elements' magnitudes (the serial
chain, the tree and the combine of csrc/dc_loss.hip, the division by n, by log 2 and the final rounding).  K comes from that count, not
from what the kernel returns.
"""
import math

import numpy as np

from diffusion_conductor_amd.synthetic import _rng

S = 1000
MEAN_TYPES = ("START_X", "EPSILON", "PREVIOUS_X")
VAR_TYPES = ("FIXED_SMALL", "FIXED_LARGE", "LEARNED", "LEARNED_RANGE")
K_ROUNDINGS = 32                                          # DC_VB_K of csrc/dc_loss.hip's header
THREADS, DEPTH, SPAN, MAX_GROUPS = 256, 8, 2048, 32       # DC_LOSS_THREADS, block_tree, DC_VB_SPAN, DC_VB_MAX_GROUPS
U = 2.0 ** -24
LOG2 = math.log(2.0)
NLL_CAP = 27.64
INNER, SATURATED, SATURATED_EXACT = 2.5, 8.0, 7.0

# the fixture's cases (tools/make_golden_vb.py): (B, T) with per-clip timesteps; P = 26
FIXTURE_CASES = {(3, 5): [0, S - 1, 417], (4, 33): [1, 0, 250, S - 1]}
LOOP_S, LOOP_B, LOOP_T = 25, 3, 5                         # the fixture's calc_bpd_loop: a 25-step linear schedule
LOOP_TYPES = (("START_X", "FIXED_SMALL"), ("START_X", "FIXED_LARGE"), ("EPSILON", "LEARNED_RANGE"), ("PREVIOUS_X", "LEARNED"))
CASE_SEED, LOOP_NOISE_SEED = 61, 62


def groups(n):
    return min(MAX_GROUPS, max(1, math.ceil(math.ceil(n / 2) / SPAN)))


def chain(n):
    """The longest chain of additions behind one of dc_vb_terms' sums over a clip of n elements."""
    g = groups(n)
    per = math.ceil(math.ceil(n / 2) / g)
    return math.ceil(per / THREADS) + 1 + (g - 1)


def prior_chain(n):
    return math.ceil(math.ceil(n / 2) / THREADS) + 1


def tables(betas):
    """The float64 tables of GaussianDiffusion.__init__ (gaussian_diffusion.py:328-379) dc_vb_coefficients reads, by name."""
    b = np.asarray(betas, np.float64)
    ac = np.cumprod(1.0 - b)
    prev = np.append(1.0, ac[:-1])
    pv = b * (1.0 - prev) / (1.0 - ac)
    plv = np.log(np.append(pv[1], pv[1:])) if len(b) > 1 else np.log(np.maximum(pv, 1e-20))
    c1, c2 = b * np.sqrt(prev) / (1.0 - ac), (1.0 - prev) * np.sqrt(1.0 - b) / (1.0 - ac)
    return {"c1": c1, "c2": c2, "plv": plv, "FIXED_SMALL": plv, "FIXED_LARGE": np.log(np.append(pv[1], b[1:])) if len(b) > 1 else plv,
            "LEARNED_RANGE": np.log(b), "LEARNED": np.zeros_like(b), "rc": np.sqrt(1.0 / ac), "rm1": np.sqrt(1.0 / ac - 1),
            "r1": 1.0 / c1, "r21": c2 / c1, "sqrt_ac": np.sqrt(ac), "log_1m_ac": np.log(1.0 - ac)}


def coefficients(betas, var_type, t):
    """What dc_vb_coefficients must return: fp32 [B, 12], (float) of the float64 entries."""
    tb, t = tables(betas), np.asarray(t).reshape(-1)
    out = np.zeros((len(t), 12), np.float32)
    for k, name in enumerate(("c1", "c2", "plv", var_type, "rc", "rm1")):
        out[:, k] = tb[name][t].astype(np.float32)
    out[:, 6] = t == 0
    out[:, 7], out[:, 8] = tb["r1"][t].astype(np.float32), tb["r21"][t].astype(np.float32)
    return out


def linear_betas(n):
    scale = 1000 / n
    return np.linspace(scale * 0.0001, scale * 0.02, n, dtype=np.float64)


def stages_fp32(x0, xt, mo, coef, mean_type, clip):
    """(pred_xstart, true mean m1, model mean m2) [B, n] in float32, operation by operation as p_mean_variance and
    q_posterior_mean_variance form them (gaussian_diffusion.py:418-440, 497-530)."""
    x0, xt, mo, coef = (np.asarray(a, np.float32) for a in (x0, xt, mo, coef))
    B = x0.shape[0]
    x0, xt, mo = x0.reshape(B, -1), xt.reshape(B, -1), mo.reshape(B, -1)
    c = lambda k: coef[:, k:k + 1]      # noqa: E731
    if mean_type == "START_X":
        pred = mo
    elif mean_type == "EPSILON":
        pred = c(4) * xt - c(5) * mo
    else:
        pred = c(7) * mo - c(8) * xt
    if clip:
        pred = np.clip(pred, np.float32(-1), np.float32(1))
    m2 = mo if mean_type == "PREVIOUS_X" else c(0) * pred + c(1) * xt
    m1 = c(0) * x0 + c(1) * xt
    assert pred.dtype == m1.dtype == m2.dtype == np.float32
    return pred, m1, m2


def log_variance(coef, var_type, vv, shape):
    """The model's log-variance [B, n] in float64 (gaussian_diffusion.py:472-503)."""
    coef = np.asarray(coef, np.float64)
    if var_type == "LEARNED":
        return np.asarray(vv, np.float64).reshape(shape)
    if var_type == "LEARNED_RANGE":
        frac = (np.asarray(vv, np.float64).reshape(shape) + 1) / 2
        return frac * coef[:, 3:4] + (1 - frac) * coef[:, 2:3]
    return np.broadcast_to(coef[:, 3:4], shape)


def _cdf(x):
    return 0.5 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def oracle(x0, xt, pred, m1, m2, coef, var_type, vv=None, noise=None, n_chain=None):
    """float64 [B, 5] (output, kl, decoder_nll in bits, xstart_mse, mse) from the fp32 stages, the bound [B, 5] each slot of
    dc_vb_terms may differ from it by, and z [B, n] = (x0 - m2) / sigma."""
    B = np.asarray(x0).shape[0]
    x0f = np.asarray(x0, np.float32).reshape(B, -1)
    x0, xt, pred, m1, m2 = (np.asarray(a, np.float64).reshape(B, -1) for a in (x0, xt, pred, m1, m2))
    n = x0.shape[1]
    cf = np.asarray(coef, np.float64)
    lv1, lv2 = cf[:, 2:3], log_variance(coef, var_type, vv, x0.shape)
    d = m1 - m2
    parts = np.stack([np.ones_like(d), np.abs(lv2 - lv1), np.exp(lv1 - lv2), d * d * np.exp(-lv2)])
    kl = 0.5 * (-1.0 + lv2 - lv1 + parts[2] + parts[3])
    kl_mag, kl_el = 0.5 * parts.sum(axis=0), K_ROUNDINGS * U * 0.5 * parts.sum(axis=0)
    sigma = np.exp(0.5 * lv2)
    cen = x0 - m2
    z = cen / sigma
    cp, cm = _cdf((cen + 1.0 / 255.0) / sigma), _cdf((cen - 1.0 / 255.0) / sigma)
    prob = np.where(x0f < np.float32(-0.999), cp, np.where(x0f > np.float32(0.999), 1.0 - cm, cp - cm))
    delta = np.maximum(prob, 1e-12)
    nll = -np.log(delta)
    nll_el = np.minimum(K_ROUNDINGS * U * (1.0 / delta + np.abs(np.log(delta))), NLL_CAP)
    ap, am = (cen + 1.0 / 255.0) / sigma, (cen - 1.0 / 255.0) / sigma
    exact = (np.minimum(np.abs(ap), np.abs(am)) >= SATURATED_EXACT) & (ap * am > 0)
    nll_el = np.where(exact, K_ROUNDINGS * U * (1.0 + np.abs(np.log(delta))), nll_el)
    e = pred - x0
    xs, xs_el = e * e, 3 * U * e * e * (1 + 2 * U)
    if noise is not None:
        num = (np.asarray(coef, np.float32)[:, 4:5] * xt.astype(np.float32) - pred.astype(np.float32)).astype(np.float64)      # fp32 stage
        eps = num / cf[:, 5:6]
        de = eps - np.asarray(noise, np.float64).reshape(B, -1)
        dde = U * (np.abs(eps) + np.abs(de))
        ms, ms_el = de * de, 2 * np.abs(de) * dde + dde * dde + U * de * de
    else:
        ms, ms_el = np.zeros_like(e), np.zeros_like(e)
    red = ((chain(n) if n_chain is None else n_chain) + DEPTH + 3) * U
    val = np.stack([kl.mean(axis=1) / LOG2, nll.mean(axis=1) / LOG2, xs.mean(axis=1), ms.mean(axis=1)], axis=1)
    bnd = np.stack([(kl_el.mean(axis=1) + red * kl_mag.mean(axis=1)) / LOG2, (nll_el.mean(axis=1) + red * np.abs(nll).mean(axis=1)) / LOG2,
                    xs_el.mean(axis=1) + red * xs.mean(axis=1), ms_el.mean(axis=1) + red * ms.mean(axis=1)], axis=1)
    t0 = cf[:, 6] != 0
    out = np.concatenate([np.where(t0, val[:, 1], val[:, 0])[:, None], val], axis=1)
    bound = np.concatenate([np.where(t0, bnd[:, 1], bnd[:, 0])[:, None], bnd], axis=1)
    return out, bound, z


def band(z):
    """How many elements lie between the two regimes, and the shares (inner, saturated)."""
    a = np.abs(z)
    return int(((a > INNER) & (a < SATURATED)).sum()), float((a <= INNER).mean()), float((a >= SATURATED).mean())


def prior_oracle(x0, a, logvar):
    """float64 [B] of dc_prior_kl and its bound: a x0 is the fp32 stage; behind it x^2, three sums, (-1 - lv), expf: 7 roundings."""
    B = np.asarray(x0).shape[0]
    x = np.asarray(x0, np.float32).reshape(B, -1)
    a32, lv = np.asarray(a, np.float32).reshape(B, 1), np.asarray(logvar, np.float64).reshape(B, 1)
    m = (a32 * x).astype(np.float64)
    mag = 0.5 * (1.0 + np.abs(lv) + np.exp(lv) + m * m)
    kl = 0.5 * (-1.0 - lv + np.exp(lv) + m * m)
    red = (prior_chain(x.shape[1]) + DEPTH + 3) * U
    return kl.mean(axis=1) / LOG2, (7 * U + red) * mag.mean(axis=1) / LOG2


def make_case(B, T, P, mean_type, var_type, clip, t, betas=None, seed=CASE_SEED):
    """One constructed case: {"x0", "xt", "model_out", "var_values" (None for a fixed variance), "noise"} fp32 [B, T, P], "coef"
    [B, 12], "t".  30 % of x0 sits at +-1 (the two open-ended bins), the rest inside (-0.8, 0.8); about a fifth of the elements is
    saturated (10 <= |z| <= 14), the others inner (|z| <= 2); pred_xstart is drawn in (-1.2, 1.2) so that clipping acts."""
    betas = linear_betas(S) if betas is None else betas
    t = np.asarray(t).reshape(-1)
    assert len(t) == B
    n = T * P
    rng = _rng(seed, f"vb{mean_type}{var_type}{int(clip)}", 1000 * n + B)
    coef = coefficients(betas, var_type, t)
    c = coef.astype(np.float64)
    x0 = rng.uniform(-0.8, 0.8, (B, n))
    edge = rng.random((B, n))
    x0 = np.where(edge < 0.15, -1.0, np.where(edge < 0.30, 1.0, x0)).astype(np.float32).astype(np.float64)
    vv = None
    if var_type == "LEARNED":
        vv = rng.uniform(-10.0, -6.0, (B, n)).astype(np.float32)
    elif var_type == "LEARNED_RANGE":
        vv = rng.uniform(-1.0, 1.0, (B, n)).astype(np.float32)
    sigma = np.exp(0.5 * log_variance(coef, var_type, vv, (B, n)))
    sat = rng.random((B, n)) < 0.2
    sat[:, 0], sat[:, 1:2] = True, False      # both regimes in every clip, however short
    mag = np.where(sat, rng.uniform(10.0, 14.0, (B, n)), rng.uniform(0.0, 2.0, (B, n)))
    sign = np.where(x0 >= 0, 1.0, -1.0)      # the mean moves towards 0: at t = 0 pred_xstart = x0 - z sigma stays inside [-1, 1]
    z = sign * mag
    mean = x0 - z * sigma
    xt = rng.standard_normal((B, n))
    pred = rng.uniform(-1.2, 1.2, (B, n))
    c1, c2 = c[:, 0:1], c[:, 1:2]
    if mean_type == "PREVIOUS_X":
        mo = mean
    else:
        first = c[:, 6:7] != 0      # t = 0: coef2 = 0, the mean is pred_xstart itself
        pred = np.where(first, mean, pred)
        eff = np.clip(pred, -1, 1) if clip else pred
        xt = np.where(first, xt, (mean - c1 * eff) / np.where(first, 1.0, c2))
        mo = pred if mean_type == "START_X" else (c[:, 4:5] * xt.astype(np.float32) - pred) / c[:, 5:6]
    shape = (B, T, P)
    return {"x0": x0.astype(np.float32).reshape(shape), "xt": xt.astype(np.float32).reshape(shape),
            "model_out": mo.astype(np.float32).reshape(shape), "var_values": None if vv is None else vv.reshape(shape),
            "noise": rng.standard_normal((B, n)).astype(np.float32).reshape(shape), "coef": coef, "t": t}


def case_oracle(case, mean_type, var_type, clip, with_noise=True):
    pred, m1, m2 = stages_fp32(case["x0"], case["xt"], case["model_out"], case["coef"], mean_type, clip)
    out, bound, z = oracle(case["x0"], case["xt"], pred, m1, m2, case["coef"], var_type, case["var_values"],
                           case["noise"] if with_noise else None)
    return out, bound, z, pred


def loop_noise(t, B=LOOP_B, T=LOOP_T):
    """Step t's draw of the fixture's calc_bpd_loop (in place of th.randn_like), [B, T, 26]."""
    return _rng(LOOP_NOISE_SEED, "vbloop", t).standard_normal((B, T, 26), dtype=np.float32)


def loop_inputs(mean_type, var_type):
    """x0 [B, T, 26] and the stub model's fixed output ([B, 2 T, 26] for the learned types: mean half, then variance half)."""
    rng = _rng(CASE_SEED, f"loop{mean_type}{var_type}", 0)
    x0 = rng.uniform(-0.8, 0.8, (LOOP_B, LOOP_T, 26))
    edge = rng.random(x0.shape)
    x0 = np.where(edge < 0.15, -1.0, np.where(edge < 0.30, 1.0, x0)).astype(np.float32)
    if mean_type == "START_X":      # a prediction a few bins off: inner at t = 0 (sigma = 0.04 on the 25-step schedule)
        out = x0 + rng.uniform(-0.06, 0.06, x0.shape).astype(np.float32)
    else:
        out = rng.standard_normal(x0.shape).astype(np.float32)
    if var_type in ("LEARNED", "LEARNED_RANGE"):
        vv = rng.uniform(-4.0, -1.0, x0.shape) if var_type == "LEARNED" else rng.uniform(-1.0, 1.0, x0.shape)
        out = np.concatenate([out, vv.astype(np.float32)], axis=1)
    return x0, out.astype(np.float32)


def loop_oracle(mean_type, var_type):
    """The oracle of the fixture's calc_bpd_loop with loop_noise's draws: (want, bound) [B, LOOP_S, 5] with the columns in the loop's
    order (column 0 is t = LOOP_S - 1), and (prior, its bound) [B].  x_t is q_sample's bits: float32 products and sum."""
    betas = linear_betas(LOOP_S)
    tb, ac = tables(betas), np.cumprod(1.0 - betas)
    x0, fixed = loop_inputs(mean_type, var_type)
    mo, vv = (fixed, None) if fixed.shape[1] == LOOP_T else (fixed[:, :LOOP_T], fixed[:, LOOP_T:])
    want, bound = (np.zeros((LOOP_B, LOOP_S, 5)) for _ in range(2))
    for col, t in enumerate(range(LOOP_S - 1, -1, -1)):
        coef = coefficients(betas, var_type, [t] * LOOP_B)
        nz = loop_noise(t)
        xt = np.float32(np.sqrt(ac[t])) * x0 + np.float32(np.sqrt(1.0 - ac[t])) * nz
        pred, m1, m2 = stages_fp32(x0, xt, mo, coef, mean_type, True)
        want[:, col], bound[:, col], _ = oracle(x0, xt, pred, m1, m2, coef, var_type, vv, nz)
    pw, pb = prior_oracle(x0, np.full(LOOP_B, np.float32(tb["sqrt_ac"][-1])), np.full(LOOP_B, np.float32(tb["log_1m_ac"][-1])))
    return want, bound, pw, pb


def total_bound(want, bound, pw, pb):
    """The sum over the columns and the prior: every term's own bound, plus one rounding per addition of the running magnitude."""
    return bound[:, :, 0].sum(axis=1) + pb + (want.shape[1] + 1) * U * (np.abs(want[:, :, 0]).sum(axis=1) + np.abs(pw))
