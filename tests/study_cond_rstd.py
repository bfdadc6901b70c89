#!/usr/bin/env python3
"""CPU study behind k_cond_rstd's shifted features (dc_kernels.hip; not collected by pytest).

The conditioning pre-pass takes the variance of linear(x) over its 512 outputs - text_norm's, in front of the cross-attention keys
and values - as a quadratic form of the 64 music features, var = x^T Gc x + 2 gv^T x + c.  This script emulates, in fp32 and against
fp64,
  (q) that form in the kernel's FMA order (u_i = 2 gv_i + sum_j Gc_ij x_j over j, var += u_i x_i over i),
  (s) the same form of the shifted features z = x + u, u the least-squares solution of Wc u = bc in fp32 and the constants made from
      r = bc - Wc u (centre_linear of dc_api.hip): what k_cond_rstd computes,
  (d) the direct form: linear(x) in fp32, mean and variance over the 512 outputs in two passes (nn.LayerNorm, DC_COND_512=1),
on the seeded checkpoint (x = delta N(0,1)) and on one whose linear.bias lies in the column space of linear.weight (bias = W u,
x = -u + delta N(0,1): linear(x) = delta W n), for delta = 1 ... 0, 512 tokens each.  Printed per row: the mean variance and the worst
relative error of rstd = 1 / sqrt(var + 1e-5) of each form.  (A linear.weight without full column rank keeps u = 0: (s) is (q) there.)
(An FMA is emulated as one fp64 product-and-sum rounded to fp32: exact but for rare double roundings.)
usage: python tests/study_cond_rstd.py"""
import numpy as np
import torch

from helpers import colspace_state_dict, state_dict_np

EPS = 1e-5
f32 = np.float32


def fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def gram_of(w, b, shifted):
    """centre_linear of dc_api.hip: fp64 on the host, stored as fp32.  -> Gc, gv, c, shift"""
    w, b = w.astype(np.float64), b.astype(np.float64)
    wc, bc = w - w.mean(0, keepdims=True), b - b.mean()
    shift = np.linalg.solve(wc.T @ wc, wc.T @ bc).astype(f32) if shifted else np.zeros(64, f32)
    r = bc - wc @ shift.astype(np.float64)
    return (wc.T @ wc / 512).astype(f32), (wc.T @ r / 512).astype(f32), f32(r @ r / 512), shift


def quadratic(x, G, gv, c):
    n = x.shape[0]
    var = np.full(n, c, f32)
    for i in range(64):
        u = np.full(n, f32(2) * gv[i], f32)
        for j in range(64):
            u = fma(np.full(n, G[i, j], f32), x[:, j], u)
        var = fma(u, x[:, i], var)
    return var


def direct(x, w, b):
    y = torch.nn.functional.linear(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b))
    return y.var(-1, unbiased=False).numpy()


def exact(x, w, b):
    y = x.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    return y.var(-1)


def rstd(v):
    return 1.0 / np.sqrt(np.maximum(v.astype(np.float64), 0.0) + EPS)


def main():
    sd0 = {k: np.asarray(v) for k, v in state_dict_np().items()}
    sd1, u = colspace_state_dict()
    rng = np.random.default_rng(5)
    noise = rng.standard_normal((512, 64)).astype(f32)
    print(f"{'checkpoint':<13}{'delta':>8}{'mean var':>11}{'quadratic':>11}{'shifted':>11}{'direct':>11}")
    for name, sd, centre in (("seeded", sd0, np.zeros(64, f32)), ("column-space", sd1, -u)):
        w, b = sd["linear.weight"], sd["linear.bias"]
        G, gv, c, _ = gram_of(w, b, False)
        Gs, gvs, cs, shift = gram_of(w, b, True)
        for delta in (1.0, 1e-1, 1e-2, 1e-3, 1e-4, 0.0):
            x = (centre + f32(delta) * noise).astype(f32)
            ref = rstd(exact(x, w, b))
            vq = quadratic(x, G, gv, c)
            vs = quadratic(x + shift, Gs, gvs, cs)
            vd = direct(x, w, b)
            err = [float(np.max(np.abs(rstd(v) / ref - 1.0))) for v in (vq, vs, vd)]
            print(f"{name:<13}{delta:>8.0e}{exact(x, w, b).mean():>11.2e}{err[0]:>11.1e}{err[1]:>11.1e}{err[2]:>11.1e}")


if __name__ == "__main__":
    main()
