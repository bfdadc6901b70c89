"""Sampling on a sub-sequence of timesteps with a first- or second-order update, the host half (no GPU): dc_solver_table against an
fp64 restatement and against dc_ddim_coefficients_known, sampler.spaced_timesteps, the order of the two solvers on a model with a
closed form, the argument errors, and the checker of the GPU tests (helpers_solver.solver_loop) against the oracle's own loop."""
import numpy as np
import pytest
import torch

from helpers import O, batch_noise, make_diffusion, oracle_params, xf_pair
from helpers_solver import solver_loop, solver_rows

from diffusion_conductor_amd import native
from diffusion_conductor_amd.sampler import spaced_timesteps


def _ac(S):
    return native.linear_beta_schedule(S)["alphas_cumprod"]


def _rows_fp64(ac, ts, eta, order):
    """dc_solver_table restated in fp64 numpy from the header's formulas: [n, 9]."""
    ts = np.asarray(ts)
    a, an = ac[ts], np.append(ac[ts[1:]], 1.0)
    sigma = eta * np.sqrt((1 - an) / (1 - a)) * np.sqrt(1 - a / an)
    lam = 0.5 * np.log(ac / (1 - ac))
    kappa = np.zeros(len(ts))
    for i in range(1, len(ts) - 1):
        if order == 2:
            h, hb = lam[ts[i + 1]] - lam[ts[i]], lam[ts[i]] - lam[ts[i - 1]]
            kappa[i] = (np.sqrt(an[i]) - np.sqrt(1 - an[i]) * np.sqrt(a[i] / (1 - a[i]))) * h / (2 * hb)
    return np.stack([np.sqrt(1 / a), np.sqrt(1 / a - 1), np.sqrt(an), np.sqrt(np.maximum(1 - an - sigma ** 2, 0)), sigma, np.sqrt(1 - an),
                     np.sqrt(a), np.sqrt(1 - a), kappa], 1)


@pytest.mark.parametrize("S", [25, 1000])
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_full_sequence_rows_are_the_known_table(S, eta):
    ac = _ac(S)
    ck, start = native.ddim_coefficients_known(ac, eta)
    rows, start2 = native.solver_table(ac, list(range(S - 1, -1, -1)), eta, 1)
    assert rows.shape == (S, native.SOLVER_ROW) and rows.dtype == np.float32
    assert np.array_equal(rows[:, :8].view(np.uint32), ck[::-1].view(np.uint32))          # slots 0..7, t = S-1 .. 0: bit for bit
    assert not rows[:, 8:].any() and np.array_equal(start, start2)
    if eta == 0.0:      # order 2 on the full sequence: the same first-order slots, kappa beside them
        r2, _ = native.solver_table(ac, list(range(S - 1, -1, -1)), 0.0, 2)
        assert np.array_equal(r2[:, :8].view(np.uint32), rows[:, :8].view(np.uint32)) and (r2[1:-1, 8] > 0).all()


@pytest.mark.parametrize("spacing", ["uniform", "logsnr"])
@pytest.mark.parametrize("order,eta", [(1, 0.0), (1, 0.5), (2, 0.0)])
def test_table_against_fp64(spacing, order, eta):
    """Slots 0..7 are fp32 arithmetic on fp32-rounded abar: slots 0, 1, 2, 6 are good to a few ulp (3e-7 relative); the four that
    take sqrt(1 - a) of an fp32 a near 1 (3, 5, 7, and sigma, which is eta times such a root times factors <= 1) carry its rounding,
    6e-8 / (2 sqrt(1 - a)) <= 3e-6 absolute at 1 - a >= 1e-4.  kappa is fp64 rounded once: half an ulp, 6e-8 relative."""
    ac = _ac(1000)
    for n in (2, 3, 10, 25):
        ts = spaced_timesteps(ac, n, spacing)
        rows, start = native.solver_table(ac, ts, eta, order)
        want = _rows_fp64(ac, ts, eta, order)
        assert np.allclose(rows[:, [0, 1, 2, 6]], want[:, [0, 1, 2, 6]], rtol=3e-7, atol=0)
        assert np.allclose(rows[:, [3, 4, 5, 7]], want[:, [3, 4, 5, 7]], rtol=3e-7, atol=3e-6)
        assert np.allclose(rows[:, 8], want[:, 8], rtol=1.2e-7, atol=0)
        assert not rows[:, 9:].any()
        assert rows[0, 8] == 0.0 and rows[-1, 8] == 0.0 and (order == 2 or not rows[:, 8].any())
        assert order == 1 or n < 3 or (rows[1:-1, 8] > 0).all()
        assert rows[-1, 2] == 1.0 and rows[-1, 5] == 0.0                                   # the last step lands on the clean sample
        assert np.array_equal(start, rows[0, 6:8])
        co, (a0, b0) = solver_rows(1000, ts, eta, order)                                   # the checker's rows: the same to an ulp
        assert np.allclose(co.numpy()[:, :7], rows[:, [0, 1, 2, 3, 4, 5, 8]], rtol=3e-7, atol=1e-9)
        assert np.allclose([a0, b0], start, rtol=2e-7)


@pytest.mark.parametrize("spacing", ["uniform", "logsnr"])
def test_spaced_timesteps(spacing):
    for S in (25, 1000):
        ac = _ac(S)
        assert spaced_timesteps(ac, 1, spacing) == [S - 1]
        assert spaced_timesteps(ac, S, spacing) == list(range(S - 1, -1, -1))
        for n in (2, 3, 10, 24, 25):
            ts = spaced_timesteps(ac, n, spacing)
            assert all(isinstance(t, int) for t in ts) and 2 <= len(ts) <= n
            assert ts[0] == S - 1 and ts[-1] == 0 and all(b < a for a, b in zip(ts, ts[1:]))
            if spacing == "uniform":
                assert ts == [int(np.floor(k * (S - 1) / (n - 1) + 0.5)) for k in range(n)][::-1]
    ac = _ac(1000)
    lam = 0.5 * np.log(ac / (1 - ac))
    ts = spaced_timesteps(ac, 25, "logsnr")
    assert len(ts) == 25 and np.ptp(np.diff(lam[ts])) <= 0.25 * np.mean(np.diff(lam[ts]))      # equal strides in lambda, to a timestep
    for bad in (0, 1001, -3):
        with pytest.raises(ValueError):
            spaced_timesteps(ac, bad, spacing)
    with pytest.raises(ValueError):
        spaced_timesteps(ac, 10, "cosine")


def _closed_form_error(ac, ts, order, s2=0.25):
    """|x_0 - exact| of the scalar fp64 recursion with the library's rows on data N(0, s2): the exact x0-predictor is
    sqrt(abar) s2 / (abar s2 + 1 - abar) x, the ODE's solution from x_T = 1 ends at s / sqrt(abar_T s2 + 1 - abar_T)."""
    rows = native.solver_table(ac, ts, 0.0, order)[0].astype(np.float64)
    x, prev = 1.0, 0.0
    for i, t in enumerate(ts):
        a = ac[t]
        pred = np.sqrt(a) * s2 / (a * s2 + 1 - a) * x
        c = rows[i]
        x = pred * c[2] + c[3] * (c[0] * x - pred) / c[1] + c[8] * (pred - prev)
        prev = pred
    return abs(x - np.sqrt(s2) / np.sqrt(ac[ts[0]] * s2 + 1 - ac[ts[0]]))


def test_second_order_on_a_closed_form_model():
    """With "logsnr" spacing on the 1000-step linear schedule the multistep update's error is at most a quarter of DDIM's at 10, 25 and
    50 evaluations, and falls at least 3 times from 25 to 50 (second order; DDIM's halves).  Nothing is asserted for "uniform"
    spacing, where 2M is worse than DDIM below about 50 steps on this model (sampler.spaced_timesteps)."""
    ac = _ac(1000)
    err = {(n, o): _closed_form_error(ac, spaced_timesteps(ac, n, "logsnr"), o) for n in (10, 25, 50) for o in (1, 2)}
    for n in (10, 25, 50):
        print(f"closed form, logsnr n={n}: DDIM {err[n, 1]:.3e}  2M {err[n, 2]:.3e}  ratio {err[n, 1] / err[n, 2]:.1f}")
        assert err[n, 2] <= err[n, 1] / 4
    print(f"25 -> 50: 2M falls {err[25, 2] / err[50, 2]:.1f} x, DDIM {err[25, 1] / err[50, 1]:.1f} x")
    assert err[25, 2] / err[50, 2] >= 3
    for n in (10, 25, 50):      # printed only
        ts = spaced_timesteps(ac, n, "uniform")
        print(f"closed form, uniform n={n}: DDIM {_closed_form_error(ac, ts, 1):.3e}  2M {_closed_form_error(ac, ts, 2):.3e}")


def test_argument_errors():
    ac = _ac(1000)
    ok = [999, 500, 0]
    native.solver_table(ac, ok, 0.5, 1)
    for ts in ([0, 500, 999], [999, 500, 500, 0], [1000, 500, 0], [999, 500, -1], []):      # increasing, repeated, out of range, n = 0
        with pytest.raises(native.DcError):
            native.solver_table(ac, ts, 0.0, 1)
    for order, eta in ((3, 0.0), (0, 0.0), (2, 0.5)):
        with pytest.raises(native.DcError):
            native.solver_table(ac, ok, eta, order)
    # the Python surface, in front of any device work
    gd = make_diffusion(1000)
    for kw in (dict(steps=25, denoised_fn=lambda x: x), dict(timesteps=ok, cond_fn=lambda x, t: x), dict(solver="dpmpp2m", denoised_fn=lambda x: x),
               dict(steps=25, solver="heun")):
        with pytest.raises(ValueError):
            gd.ddim_sample_loop(None, (1, 32, 26), **kw)
    with pytest.raises(ValueError):
        next(gd.ddim_sample_loop_progressive(None, (1, 32, 26), steps=25))


def test_checker_on_the_full_sequence_is_the_oracles_loop():
    """helpers_solver.solver_loop on t = S-1 .. 0 at order 1 is O.ddim_sample_loop (same forward, same scalars): equal to rounding."""
    S, B, T = 25, 1, 40
    p = oracle_params()
    xfp, xfo = xf_pair(B, T)
    x = torch.from_numpy(batch_noise(B, T))
    with torch.no_grad():
        want = O.ddim_sample_loop(p, x, xfp, xfo, [T], S)
    got = solver_loop(p, x, xfp, xfo, [T], S, list(range(S - 1, -1, -1)), 1)
    assert torch.allclose(got, want, rtol=0, atol=1e-5), float((got - want).abs().max())
