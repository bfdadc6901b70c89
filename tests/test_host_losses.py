"""The held-out denoising losses without a GPU: the host entry point dc_q_sample_coefficients, the argument refusals of the three
device entry points (csrc/dc_loss.hip), the plain-torch path of GaussianDiffusion.q_sample / training_losses and
metrics.denoising_loss_scalars, against the reference's numbers of tests/golden/g14_training_losses.npz
(tools/make_golden_losses.py: GaussianDiffusion.training_losses and DDPMTrainer.backward_G with a stub model that returns a fixed
tensor).

Tolerances.  x_t: bit-equal (two rounded products, one rounded sum, on both sides).  Loss terms against the reference's fp32 values:
3e-5 relative - both sides are fp32 sums of at most 65 * 26 = 1 690 non-negative terms, far below that.  The combination function on
the fixture's own per-clip terms against the backward_G scalars: 1e-6 relative."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers_losses import CASES_A, MEAN_TYPES, S, SCALAR_KEYS, case_inputs, check_digests, g14, rel, terms_fp64

from diffusion_conductor_amd import metrics, native
from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule

TERM_TOL, SCALAR_TOL = 3e-5, 1e-6
FAKE = C.c_void_p(0x1000)          # a non-NULL "device pointer": every call below must return before anything reads it


def diffusion(mean_type="START_X", loss_type=LossType.MSE, var_type=ModelVarType.FIXED_SMALL):
    return GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=getattr(ModelMeanType, mean_type),
                             model_var_type=var_type, loss_type=loss_type)


@pytest.mark.parametrize("B,T", CASES_A)
def test_q_sample_coefficients_are_the_reference_tables(B, T):
    g = g14()
    a, s = native.q_sample_coefficients(diffusion().alphas_cumprod, g[f"a_B{B}_T{T}_t"])
    assert a.dtype == np.float32 and np.array_equal(a, g[f"a_B{B}_T{T}_sqrt_abar"])
    assert np.array_equal(s, g[f"a_B{B}_T{T}_sqrt_1m_abar"])


@pytest.mark.parametrize("bad", ([-1], [S], [0, S + 5]))
def test_q_sample_coefficients_refuse_a_timestep_outside_the_schedule(bad):
    with pytest.raises(native.DcError, match="error -1"):
        native.q_sample_coefficients(diffusion().alphas_cumprod, bad)


def test_device_entry_points_refuse_bad_arguments_before_any_device_call():
    L = native.lib()
    one = np.ones(2, np.float32)
    fp, ip = native._fptr, native._iptr

    def q(x0=FAKE, noise=FAKE, a=fp(one), s=fp(one), B=2, T=4, P=26, it=0, zout=None, xt=C.c_void_p(0x2000)):
        return L.dc_q_sample(x0, noise, a, s, B, T, P, 0, it, 0, zout, xt, None)

    def terms(pred=FAKE, target=C.c_void_p(0x2000), length=None, B=2, T=4, P=26, out=C.c_void_p(0x3000)):
        lp = None if length is None else ip(np.asarray(length, np.int32))
        return L.dc_motion_loss_terms(pred, target, lp, B, T, P, out, None)

    def l1(a=FAKE, b=C.c_void_p(0x2000), B=2, T=4, out=C.c_void_p(0x3000)):
        return L.dc_latent_l1(a, b, B, T, out, None)

    INVALID = -1
    assert q(x0=None) == INVALID and q(xt=None) == INVALID and q(a=None) == INVALID and q(s=None) == INVALID
    assert q(B=0) == INVALID and q(T=0) == INVALID and q(P=0) == INVALID
    assert q(noise=None, it=-1) == INVALID                        # the seeded path needs an iteration
    assert q(zout=C.c_void_p(0x4000)) == INVALID                  # the draws' output beside a caller's noise tensor
    assert q(xt=FAKE) == INVALID                                  # in place over x0
    assert terms(pred=None) == INVALID and terms(target=None) == INVALID and terms(out=None) == INVALID
    assert terms(P=25) == INVALID and terms(P=28) == INVALID
    assert b"26" in L.dc_last_error()
    assert terms(T=1) == INVALID
    assert b"NaN" in L.dc_last_error()
    assert terms(B=0) == INVALID
    assert terms(length=[0, 4]) == INVALID and terms(length=[4, 5]) == INVALID and terms(length=[-3, 1]) == INVALID
    assert terms(pred=C.c_void_p(0x1004)) == INVALID              # float2 loads
    assert l1(a=None) == INVALID and l1(b=None) == INVALID and l1(out=None) == INVALID
    assert l1(B=0) == INVALID and l1(T=0) == INVALID and l1(a=C.c_void_p(0x1008)) == INVALID


@pytest.mark.parametrize("mean_type", MEAN_TYPES)
@pytest.mark.parametrize("B,T", CASES_A)
def test_torch_path_with_the_stub_model_matches_the_reference(B, T, mean_type):
    g, tag = g14(), f"a_B{B}_T{T}"
    x0, noise, stub = case_inputs(B, T)
    check_digests(tag, x0, noise, stub)
    gd = diffusion(mean_type)
    t, length = torch.from_numpy(g[f"{tag}_t"]), torch.from_numpy(g[f"{tag}_length"])
    x_t = gd.q_sample(torch.from_numpy(x0), t, noise=torch.from_numpy(noise))
    assert x_t.dtype == torch.float32 and np.array_equal(x_t.numpy(), g[f"{tag}_{mean_type}_x_t"])
    fixed = torch.from_numpy((g[f"{tag}_stub_scale"] * stub).astype(np.float32))
    seen = {}

    def model(x, ts, **kw):
        seen.update(x=x, ts=ts, kw=kw)
        return fixed
    out = gd.training_losses(model, torch.from_numpy(x0), t, model_kwargs={"length": length}, noise=torch.from_numpy(noise))
    assert np.array_equal(seen["x"].numpy().reshape(x0.shape), g[f"{tag}_{mean_type}_x_t"]) and torch.equal(seen["ts"], t)
    assert tuple(out["mse"].shape) == (B,) and tuple(out["terms"].shape) == (B, 8)
    assert tuple(out["pred"].shape) == tuple(out["target"].shape) == (B, T, 26)
    want_target = x0 if mean_type == "START_X" else noise
    assert np.array_equal(out["target"].numpy(), want_target.reshape(B, T, 26)) and torch.equal(out["pred"], fixed)
    errs = {"mse": rel(out["mse"], g[f"{tag}_{mean_type}_mse"]), "terms": rel(out["terms"][:, :6], g[f"{tag}_{mean_type}_terms"][:, :6])}
    for k in ("velocity_body", "velocity_elbow", "velocity_head", "velocity"):
        assert out[k].dim() == 0
        errs[k] = rel(out[k], g[f"{tag}_{mean_type}_{k}"])
    errs["fp64"] = rel(out["terms"][:, :6], terms_fp64(fixed, want_target, g[f"{tag}_length"])[:, :6])
    print(f"{tag} {mean_type}: relative errors {errs}")
    assert max(errs.values()) <= TERM_TOL, errs
    assert not out["terms"][:, 6:].any()
    # [B, T, 26] in place of [B, T, 13, 2] (extension): the same numbers
    flat = gd.training_losses(model, torch.from_numpy(x0.reshape(B, T, 26)), t, model_kwargs={"length": length},
                              noise=torch.from_numpy(noise.reshape(B, T, 26)))
    assert torch.equal(flat["terms"], out["terms"])


@pytest.mark.parametrize("B,T", CASES_A)
def test_combination_reproduces_backward_g(B, T):
    g, tag = g14(), f"a_B{B}_T{T}"
    assert tuple(g["scalar_keys"]) == SCALAR_KEYS
    for mean_type in MEAN_TYPES:
        terms, feat, want = g[f"{tag}_{mean_type}_terms"], g[f"{tag}_{mean_type}_latent_l1"], g[f"{tag}_{mean_type}_scalars"]
        sc = metrics.denoising_loss_scalars(terms, g[f"{tag}_length"], feat)
        errs = {k: abs(sc[k] - w) / abs(w) for k, w in zip(SCALAR_KEYS, want)}
        print(f"{tag} {mean_type}: {errs}")
        assert max(errs.values()) <= SCALAR_TOL, errs
        assert sc["feat_included"] is True
        # the elbow clamp (ddpm_trainer.py:245), in the regime this case is in
        if sc["velocity_elbow"] > metrics.ELBOW_CLAMP:
            assert sc["loss_velocity_elbow"] == metrics.ELBOW_CLAMP
        else:
            assert sc["loss_velocity_elbow"] == sc["velocity_elbow"] == float(np.mean(terms[:, 3].astype(np.float64)))
        no_feat = metrics.denoising_loss_scalars(terms, g[f"{tag}_length"])
        assert no_feat["loss_mot_feat"] is None and no_feat["feat_included"] is False
        assert no_feat["loss"] == pytest.approx(sc["loss"] - metrics.LAMBDA_FEAT * sc["loss_mot_feat"], rel=1e-12)


def test_both_regimes_of_the_elbow_clamp_are_in_the_fixture():
    g = g14()
    elbow = {bt: float(g[f"a_B{bt[0]}_T{bt[1]}_START_X_velocity_elbow"]) for bt in CASES_A}
    assert min(elbow.values()) < metrics.ELBOW_CLAMP < max(elbow.values()), elbow
    lo = metrics.denoising_loss_scalars(np.array([[1, 2, 0, 1e-4, 0, 0, 0, 0]], float), [2])
    hi = metrics.denoising_loss_scalars(np.array([[1, 2, 0, 3e-4, 0, 0, 0, 0]], float), [2])
    assert lo["loss"] == pytest.approx(1.0 - 0.1 * 1e-4, rel=1e-12) and hi["loss"] == pytest.approx(1.0 - 0.1 * 2e-4, rel=1e-12)
    with pytest.raises(ValueError):
        metrics.denoising_loss_scalars(np.zeros((2, 7)), [1, 1])
    with pytest.raises(ValueError):
        metrics.denoising_loss_scalars(np.zeros((2, 8)), [1, 0])


def test_previous_x_targets_the_posterior_mean():
    B, T = 3, 5
    x0, noise, stub = case_inputs(B, T)
    gd = diffusion("PREVIOUS_X")
    t = torch.tensor([1, S - 1, 417])
    fixed = torch.from_numpy(stub)
    out = gd.training_losses(lambda *a, **k: fixed, torch.from_numpy(x0), t, noise=torch.from_numpy(noise))
    x_t = gd.q_sample(torch.from_numpy(x0), t, noise=torch.from_numpy(noise))
    want = gd.q_posterior_mean_variance(x_start=torch.from_numpy(x0), x_t=x_t, t=t)[0].reshape(B, T, 26)
    assert torch.equal(out["target"], want)
    assert rel(out["terms"][:, :6], terms_fp64(fixed, want, [T] * B)[:, :6]) <= TERM_TOL      # no length: every frame counts


def test_what_is_out_of_scope_raises():
    x0, noise, stub = case_inputs(3, 5)
    t = torch.tensor([0, 1, 2])
    model = lambda *a, **k: torch.from_numpy(stub)      # noqa: E731
    for lt in (LossType.KL, LossType.RESCALED_KL):
        with pytest.raises(NotImplementedError):
            diffusion(loss_type=lt).training_losses(model, torch.from_numpy(x0), t)
    for vt in (ModelVarType.LEARNED, ModelVarType.LEARNED_RANGE):
        with pytest.raises(NotImplementedError):
            diffusion(var_type=vt).training_losses(model, torch.from_numpy(x0), t)
    with pytest.raises(ValueError, match="NaN"):
        diffusion().training_losses(model, torch.from_numpy(x0[:, :1]), t)
    with pytest.raises(ValueError, match="device"):
        diffusion().training_losses(model, torch.from_numpy(x0), t, noise_seed=3)
