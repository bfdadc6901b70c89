"""The variational bound without a GPU: the host entry point dc_vb_coefficients, the argument refusals of dc_vb_terms / dc_prior_kl
(csrc/dc_loss.hip), and the plain-torch path of GaussianDiffusion._vb_terms_bpd / _prior_bpd / calc_bpd_loop against the reference's
numbers of tests/golden/g19_vb_terms.npz (tools/make_golden_vb.py: stub models that return a fixed tensor).

Tolerance.  The plain-torch path is the reference's fp32 expressions in the reference's order.  On the machine that wrote the fixture it
gives the reference's float32 numbers to the last bit.  On another CPU torch's vectorised exp / tanh / log differ in their last bits,
and a slot moves by rounding noise: a slot may differ from the reference's float32 number by what the fixture records for the
reference itself - |float32 - float64| of the same slot, one draw of that noise, which can be 0 - plus the bound derived in
tests/helpers_vb.py for fp32 arithmetic on these inputs (the one the kernel is held to).  The same bound is asserted against the
float64 oracle directly."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_vb as H
from helpers import golden

from diffusion_conductor_amd import native, sampler
from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType
from diffusion_conductor_amd.synthetic import array_digest

FAKE = [C.c_void_p(0x1000 * (k + 1)) for k in range(8)]      # non-NULL "device pointers": every call must return before reading one
INVALID = -1


@pytest.fixture(scope="module")
def g19():
    return dict(golden("g19_vb_terms.npz"))


def diffusion(mean_type="START_X", var_type="FIXED_SMALL", steps=H.S, loss_type=LossType.MSE):
    return GaussianDiffusion(betas=H.linear_betas(steps), model_mean_type=getattr(ModelMeanType, mean_type),
                             model_var_type=getattr(ModelVarType, var_type), loss_type=loss_type)


def allowed(g, key, bound):
    f32, f64 = g[key + "_f32"].astype(np.float64), g[key + "_f64"]
    return f32, np.abs(f32 - f64) + bound


@pytest.mark.parametrize("var_type", H.VAR_TYPES)
@pytest.mark.parametrize("steps", (H.S, H.LOOP_S, 2))
def test_vb_coefficients_are_float_of_the_float64_tables(var_type, steps):
    betas = H.linear_betas(steps) if steps > 2 else np.array([0.3, 0.9])
    t = np.array([0, 1, steps - 1, steps // 2, 0])
    got = native.vb_coefficients(betas, var_type, t)
    assert got.dtype == np.float32 and got.shape == (5, native.VB_COEF)
    assert np.array_equal(got, H.coefficients(betas, var_type, t))
    gd = GaussianDiffusion(betas=betas, model_mean_type=ModelMeanType.START_X, model_var_type=getattr(ModelVarType, var_type),
                           loss_type=LossType.MSE)
    for k, table in enumerate((gd.posterior_mean_coef1, gd.posterior_mean_coef2, gd.posterior_log_variance_clipped)):
        assert np.array_equal(got[:, k], table[t].astype(np.float32))
    assert np.array_equal(got[:, 4], gd.sqrt_recip_alphas_cumprod[t].astype(np.float32))
    assert np.array_equal(got[:, 5], gd.sqrt_recipm1_alphas_cumprod[t].astype(np.float32))
    assert got[:, 6].tolist() == [1, 0, 0, 0, 1] and not got[:, 9:].any()


@pytest.mark.parametrize("bad", ([-1], [H.S], [0, H.S + 5]))
def test_vb_coefficients_refuse_a_timestep_outside_the_schedule(bad):
    with pytest.raises(native.DcError, match="error -1"):
        native.vb_coefficients(H.linear_betas(H.S), "FIXED_SMALL", bad)


def test_vb_coefficients_refuse_bad_tables_and_types():
    with pytest.raises(native.DcError):
        native.vb_coefficients(np.array([0.1, 1.5]), "FIXED_SMALL", [0])
    with pytest.raises(native.DcError):
        native.vb_coefficients(np.array([0.1]), "FIXED_LARGE", [0])      # posterior_variance[1] does not exist
    with pytest.raises(native.DcError):
        native.vb_coefficients(H.linear_betas(50), 7, [0])
    with pytest.raises(ValueError):
        native.vb_coefficients(H.linear_betas(50), "FIXED", [0])


def test_device_entry_points_refuse_bad_arguments_before_any_device_call():
    L = native.lib()
    coef = H.coefficients(H.linear_betas(H.S), "FIXED_SMALL", [0, 5])
    one = np.ones(2, np.float32)
    fp = native._fptr

    def terms(x0=FAKE[0], xt=FAKE[1], mo=FAKE[2], vv=None, nz=FAKE[3], cf=fp(coef), mean=2, var=2, B=2, T=4, P=26, work=FAKE[4],
              out=FAKE[5]):
        return L.dc_vb_terms(x0, xt, mo, vv, nz, cf, mean, var, 1, B, T, P, work, out, None)

    def prior(x0=FAKE[0], a=fp(one), lv=fp(one), B=2, T=4, P=26, out=FAKE[5]):
        return L.dc_prior_kl(x0, a, lv, B, T, P, out, None)

    assert terms(x0=None) == INVALID and terms(xt=None) == INVALID and terms(mo=None) == INVALID and terms(cf=None) == INVALID
    assert terms(work=None) == INVALID and terms(out=None) == INVALID
    assert terms(B=0) == INVALID and terms(T=0) == INVALID and terms(P=0) == INVALID
    assert terms(T=1 << 20, P=1 << 11) == INVALID                 # T * P does not fit an int
    assert terms(mean=0) == INVALID and terms(mean=4) == INVALID and terms(var=0) == INVALID and terms(var=5) == INVALID
    assert terms(var=1) == INVALID and terms(var=4) == INVALID    # a learned variance without its values
    assert b"d_var_values" in L.dc_last_error()
    assert terms(vv=FAKE[6]) == INVALID                           # ... and values beside a fixed one
    assert prior(x0=None) == INVALID and prior(a=None) == INVALID and prior(lv=None) == INVALID and prior(out=None) == INVALID
    assert prior(B=0) == INVALID and prior(T=0) == INVALID and prior(P=0) == INVALID
    assert L.dc_vb_workspace_floats(0, 4, 26) == 0
    assert L.dc_vb_workspace_floats(3, 1800, 26) == 3 * H.groups(1800 * 26) * 4 and H.groups(1800 * 26) == 12
    assert H.groups(2048 * 2) == 1 and H.groups(2049 * 2) == 2 and H.groups(10 ** 7) == 32
    assert native.VB_TERMS == 8


@pytest.mark.parametrize("clip", (True, False))
@pytest.mark.parametrize("var_type", H.VAR_TYPES)
@pytest.mark.parametrize("mean_type", H.MEAN_TYPES)
def test_torch_path_with_the_stub_models_matches_the_reference(g19, mean_type, var_type, clip):
    gd = diffusion(mean_type, var_type)
    for (B, T), ts in H.FIXTURE_CASES.items():
        tag = f"c_B{B}_T{T}_{mean_type}_{var_type}_clip{int(clip)}"
        c = H.make_case(B, T, 26, mean_type, var_type, clip, ts)
        want_digest = g19[tag + "_digest"]
        for i, k in enumerate(("x0", "xt", "model_out", "noise")):
            assert np.allclose(array_digest(c[k]), want_digest[i], rtol=1e-12, atol=1e-9), (tag, k)
        ref, bound, z, pred = H.case_oracle(c, mean_type, var_type, clip)
        assert H.band(z)[0] == 0
        fixed = c["model_out"] if c["var_values"] is None else np.concatenate([c["model_out"], c["var_values"]], axis=1)
        seen = {}

        def model(x, t, **kw):
            seen.update(x=x, t=t, kw=kw)
            return torch.from_numpy(fixed)
        x0, xt, t = torch.from_numpy(c["x0"]), torch.from_numpy(c["xt"]), torch.tensor(ts)
        out = gd._vb_terms_bpd(model, x0, xt, t, clip_denoised=clip, model_kwargs={"length": None}, noise=torch.from_numpy(c["noise"]))
        assert torch.equal(seen["x"], xt) and torch.equal(seen["t"], t) and seen["kw"] == {"length": None}
        assert set(out) == {"output", "pred_xstart", "terms"} and tuple(out["terms"].shape) == (B, 8) and tuple(out["output"].shape) == (B,)
        assert np.array_equal(out["pred_xstart"].numpy().reshape(B, -1), pred)      # the affine stage, bit for bit
        assert torch.equal(out["output"], out["terms"][:, 0]) and not out["terms"][:, 5:].any()
        f32, tol = allowed(g19, tag, bound)
        got = out["terms"][:, :5].numpy().astype(np.float64)
        print(f"{tag}: largest |ours - reference| / allowed {np.max(np.abs(got - f32) / tol):.3f}; |ours - oracle| / the oracle's bound "
              f"{np.max(np.abs(got - ref) / bound):.3f}")
        assert (np.abs(got - f32) <= tol).all(), (tag, got, f32, tol)
        assert (np.abs(got - ref) <= bound).all(), (tag, got, ref, bound)      # (the bound the kernel is held to, on the host's fp32)
        # without the draw slot 4 stays 0 and the others do not move
        bare = gd._vb_terms_bpd(model, x0, xt, t, clip_denoised=clip)["terms"]
        assert torch.equal(bare[:, :4], out["terms"][:, :4]) and not bare[:, 4:].any()


def test_prior_bpd_matches_the_reference(g19):
    gd = diffusion()
    for (B, T), ts in H.FIXTURE_CASES.items():
        c = H.make_case(B, T, 26, "START_X", "FIXED_SMALL", False, ts)
        tb = H.tables(H.linear_betas(H.S))
        want, bound = H.prior_oracle(c["x0"], np.full(B, np.float32(tb["sqrt_ac"][-1])), np.full(B, np.float32(tb["log_1m_ac"][-1])))
        f32, tol = allowed(g19, f"prior_B{B}_T{T}", bound)
        got = gd._prior_bpd(torch.from_numpy(c["x0"])).numpy().astype(np.float64)
        assert got.shape == (B,) and (np.abs(got - f32) <= tol).all(), (got, f32, tol)
        assert (np.abs(got - want) <= bound).all(), (got, want, bound)


@pytest.mark.parametrize("mean_type,var_type", H.LOOP_TYPES)
def test_calc_bpd_loop_matches_the_reference(g19, monkeypatch, mean_type, var_type):
    gd = diffusion(mean_type, var_type, H.LOOP_S)
    x0, fixed = H.loop_inputs(mean_type, var_type)
    tag = f"loop_{mean_type}_{var_type}"
    assert np.allclose(np.stack([array_digest(x0), array_digest(fixed)]), g19[tag + "_digest"], rtol=1e-12, atol=1e-9)
    steps = iter(range(H.LOOP_S - 1, -1, -1))
    monkeypatch.setattr(sampler.th, "randn_like", lambda x, **k: torch.from_numpy(H.loop_noise(next(steps))).to(x.dtype))
    r = gd.calc_bpd_loop(lambda *a, **k: torch.from_numpy(fixed), torch.from_numpy(x0))
    assert next(steps, None) is None
    assert set(r) == {"total_bpd", "prior_bpd", "vb", "xstart_mse", "mse"}
    assert tuple(r["vb"].shape) == tuple(r["xstart_mse"].shape) == tuple(r["mse"].shape) == (H.LOOP_B, H.LOOP_S)
    assert tuple(r["total_bpd"].shape) == tuple(r["prior_bpd"].shape) == (H.LOOP_B,)
    assert torch.equal(r["total_bpd"], r["vb"].sum(dim=1) + r["prior_bpd"])
    want, bound, pw, pb = H.loop_oracle(mean_type, var_type)
    bounds = {"vb": bound[:, :, 0], "xstart_mse": bound[:, :, 3], "mse": bound[:, :, 4], "prior_bpd": pb, "total_bpd": H.total_bound(want, bound, pw, pb)}
    wants = {"vb": want[:, :, 0], "xstart_mse": want[:, :, 3], "mse": want[:, :, 4], "prior_bpd": pw, "total_bpd": want[:, :, 0].sum(axis=1) + pw}
    for key in r:
        f32, tol = allowed(g19, f"{tag}_{key}", bounds[key])
        got = r[key].numpy().astype(np.float64)
        assert (np.abs(got - f32) <= tol).all(), (key, np.max(np.abs(got - f32) / tol))
        assert (np.abs(got - wants[key]) <= bounds[key]).all(), (key, np.max(np.abs(got - wants[key]) / bounds[key]))


def test_calc_bpd_loop_on_a_subset_of_timesteps(monkeypatch):
    gd = diffusion("START_X", "FIXED_SMALL", H.LOOP_S)
    x0, fixed = H.loop_inputs("START_X", "FIXED_SMALL")
    model = lambda *a, **k: torch.from_numpy(fixed)      # noqa: E731
    monkeypatch.setattr(sampler.th, "randn_like", lambda x, **k: torch.zeros_like(x))      # (the columns then do not depend on the order)
    full = gd.calc_bpd_loop(model, torch.from_numpy(x0))
    sub = gd.calc_bpd_loop(model, torch.from_numpy(x0), timesteps=[0, 24, 7, 7])
    assert sub["total_bpd"] is None and tuple(sub["vb"].shape) == (H.LOOP_B, 3)
    cols = [H.LOOP_S - 1 - t for t in (24, 7, 0)]      # descending timesteps: the loop's order
    for key in ("vb", "xstart_mse", "mse"):
        assert torch.equal(sub[key], full[key][:, cols]), key
    assert torch.equal(sub["prior_bpd"], full["prior_bpd"])
    for bad in ([H.LOOP_S], [-1], []):
        with pytest.raises(ValueError):
            gd.calc_bpd_loop(model, torch.from_numpy(x0), timesteps=bad)
    with pytest.raises(ValueError, match="noise_seed"):
        gd.calc_bpd_loop(model, torch.from_numpy(x0), noise_seed=3)


def test_plain_functions_are_the_reference_definitions():
    x = torch.linspace(-3, 3, 13)
    assert torch.equal(sampler.mean_flat(torch.ones(2, 3, 4)), torch.ones(2))
    kl = sampler.normal_kl(x, -1.0, 0.0, torch.zeros(13))
    assert torch.allclose(kl, 0.5 * (-1.0 + 1.0 + np.exp(-1.0) + x ** 2), rtol=1e-6)
    with pytest.raises(AssertionError):
        sampler.normal_kl(0.0, 0.0, 0.0, 0.0)
    cdf = sampler.approx_standard_normal_cdf(x.double()).numpy()
    assert np.allclose(cdf, H._cdf(x.double().numpy()), rtol=1e-14) and abs(cdf[6] - 0.5) < 1e-15
    ll = sampler.discretized_gaussian_log_likelihood(torch.tensor([-1.0, 0.0, 1.0, 0.0]), means=torch.tensor([-1.0, 0.0, 1.0, 5.0]),
                                                     log_scales=torch.full((4,), -3.0))
    edge = float(np.log(H._cdf((1.0 / 255.0) / np.exp(-3.0))))      # an open-ended bin: everything up to half a bin past its centre
    assert torch.allclose(ll[[0, 2]], torch.tensor([edge, edge]), rtol=1e-5)
    assert ll[3] == torch.log(torch.tensor(1e-12))                                          # the clamp
    gd = diffusion(steps=50)
    m, v, lv = gd.q_mean_variance(torch.ones(2, 3), torch.tensor([0, 49]))
    assert torch.allclose(v, torch.exp(lv)) and torch.allclose(m[:, 0], torch.from_numpy(gd.sqrt_alphas_cumprod[[0, 49]]).float())


def test_training_losses_still_refuses_the_bound_as_an_objective():
    x0 = torch.zeros(1, 2, 26)
    with pytest.raises(NotImplementedError, match="out of scope"):
        diffusion(loss_type=LossType.KL).training_losses(lambda *a, **k: x0, x0, torch.tensor([0]))
    with pytest.raises(NotImplementedError, match="out of scope"):
        diffusion(var_type="LEARNED_RANGE").training_losses(lambda *a, **k: x0, x0, torch.tensor([0]))
