"""The variational bound on the MI355X (csrc/dc_loss.hip dc_vb_terms / dc_prior_kl, sampler.py, harness.py, evaluate.py) against the
float64 oracle of tests/helpers_vb.py and the reference's numbers of tests/golden/g19_vb_terms.npz (tools/make_golden_vb.py).

Tolerances are DERIVED, per slot and per clip, from the inputs (helpers_vb's docstring): K = 32 roundings on an element's path behind the
affine fp32 stages, an expf / logf / tanhf counting 2, through each slot's own expression; plus (chain + DEPTH + 3) * 2^-24 of the mean
magnitude for the reduction, with chain = ceil(per / 256) + 1 + (G - 1) for the G = min(32, ceil(ceil(n / 2) / 2048)) workgroups of a
clip of n elements.  K is a count, not a fit: every test prints the worst |error| / bound it saw (measured figures: DESIGN.md
section 16).  Every constructed case lies in the two regimes in which the reference's own fp32 likelihood means something, and says
so before the GPU is asked (helpers_vb.band).  Against the reference's numbers the reference's own recorded |fp32 - fp64| is added.
"""
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import helpers_vb as H
from helpers import golden, make_model, xf_pair

from diffusion_conductor_amd import native, sampler
from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType
from diffusion_conductor_amd.synthetic import batch_mel, synthetic_motion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 3, 1), (3, 2, 26), (2, 2048, 2), (2, 2049, 2), (65, 5, 26), (2, 1800, 26))
MIX = (0, 1, H.S - 1, 417)
BETAS = H.linear_betas(H.S)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def mixed_timesteps(B, shift=0):
    return [MIX[(b + shift) % 4] for b in range(B)]


def run(case, mean_type, var_type, clip, noise=True, rows=None):
    sel = slice(None) if rows is None else rows
    return native.vb_terms(dev(case["x0"][sel]), dev(case["xt"][sel]), dev(case["model_out"][sel]), case["coef"][sel], mean_type, var_type, clip,
                           var_values=None if case["var_values"] is None else dev(case["var_values"][sel]),
                           noise=dev(case["noise"][sel]) if noise else None).cpu().numpy()


def check_against_oracle(got, case, mean_type, var_type, clip, noise=True, what=""):
    want, bound, z, _ = H.case_oracle(case, mean_type, var_type, clip, with_noise=noise)
    ratio = np.abs(got[:, :5].astype(np.float64) - want) / np.where(bound > 0, bound, 1.0)
    print(f"{what} {mean_type} {var_type} clip={clip}: worst |error| / bound per slot {np.round(ratio.max(axis=0), 4).tolist()}")
    assert (ratio <= 1.0).all(), (what, ratio.max(axis=0), got[:, :5], want)
    t0 = case["coef"][:, 6] != 0
    assert np.array_equal(got[:, 0], np.where(t0, got[:, 2], got[:, 1]))      # slot 0 IS one of the two, bit for bit
    assert not got[:, 5:].any() and np.isfinite(got).all()
    if not noise:
        assert not got[:, 4].any()
    return ratio.max(axis=0)


def constructed(B, T, P, mean_type="START_X", var_type="FIXED_SMALL", clip=True, shift=0):
    case = H.make_case(B, T, P, mean_type, var_type, clip, mixed_timesteps(B, shift))
    z = H.case_oracle(case, mean_type, var_type, clip)[2]
    n_band, inner, saturated = H.band(z)
    assert n_band == 0, f"{n_band} elements between the two regimes"      # a condition on the INPUTS, before the GPU is asked
    a = np.abs(z)
    assert ((a <= H.INNER).any(axis=1) & (a >= H.SATURATED).any(axis=1)).all()      # both regimes in every clip
    return case


def test_the_constants_of_the_kernel_header():
    assert native.lib() and native.VB_TERMS == 8 and H.K_ROUNDINGS == 32
    assert [H.groups(T * P) for _, T, P in SHAPES] == [1, 1, 1, 2, 1, 12]
    assert H.chain(2048 * 2) == 9 and H.chain(2049 * 2) == 7 and H.chain(1800 * 26) == 8 + 1 + 11 and H.chain(3) == 2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_terms_against_the_oracle_at_the_edges_of_the_reduction(shape):
    B, T, P = shape
    case = constructed(B, T, P, shift=SHAPES.index(shape))
    got = run(case, "START_X", "FIXED_SMALL", True)
    check_against_oracle(got, case, "START_X", "FIXED_SMALL", True, what=f"{shape}")
    assert np.array_equal(run(case, "START_X", "FIXED_SMALL", True), got)      # a rerun is bit-identical
    bare = run(case, "START_X", "FIXED_SMALL", True, noise=False)
    assert np.array_equal(bare[:, :4], got[:, :4]) and not bare[:, 4:].any()


@pytest.mark.parametrize("clip", (True, False))
@pytest.mark.parametrize("var_type", H.VAR_TYPES)
@pytest.mark.parametrize("mean_type", H.MEAN_TYPES)
def test_every_branch_against_the_oracle(mean_type, var_type, clip):
    for B, T, P in ((4, 7, 26), (4, 5, 5)):      # float2 loads; an odd element count: scalar loads of every tensor
        case = constructed(B, T, P, mean_type, var_type, clip)
        check_against_oracle(run(case, mean_type, var_type, clip), case, mean_type, var_type, clip, what=f"{(B, T, P)}")
        check_against_oracle(run(case, mean_type, var_type, clip, noise=False), case, mean_type, var_type, clip, noise=False, what="no noise")


@pytest.mark.parametrize("shape,clips", (((65, 5, 26), (0, 63, 64)), ((3, 2049, 2), (0, 2))), ids=("chunk", "two-groups"))
def test_a_clips_numbers_do_not_depend_on_the_batch(shape, clips):
    B, T, P = shape
    case = constructed(B, T, P, "EPSILON", "LEARNED_RANGE", True)
    whole = run(case, "EPSILON", "LEARNED_RANGE", True)
    back = run(case, "EPSILON", "LEARNED_RANGE", True, rows=slice(None, None, -1))
    assert np.array_equal(back[::-1], whole)
    for b in clips:
        alone = run(case, "EPSILON", "LEARNED_RANGE", True, rows=slice(b, b + 1))
        assert np.array_equal(alone[0], whole[b]), b
    check_against_oracle(whole, case, "EPSILON", "LEARNED_RANGE", True, what=f"{shape}")


def test_misaligned_tensors_take_scalar_loads_and_give_the_same_bits():
    case = constructed(3, 7, 26)
    got = run(case, "START_X", "FIXED_SMALL", True)

    def off4(a):      # the same values 4 bytes past an aligned address
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        buf[1:] = dev(a).reshape(-1)
        v = buf[1:].view(a.shape)
        assert v.data_ptr() % 8 == 4 and v.is_contiguous()
        return v
    odd = native.vb_terms(off4(case["x0"]), dev(case["xt"]), dev(case["model_out"]), case["coef"], "START_X", "FIXED_SMALL", True,
                          noise=off4(case["noise"])).cpu().numpy()
    assert np.array_equal(odd, got)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prior_kl_against_fp64(shape):
    B, T, P = shape
    x0 = H.make_case(B, T, P, "START_X", "FIXED_SMALL", False, mixed_timesteps(B))["x0"]
    tb = H.tables(BETAS)
    a, lv = np.full(B, np.float32(tb["sqrt_ac"][-1])), np.full(B, np.float32(tb["log_1m_ac"][-1]))
    a[0], lv[0] = np.float32(0.7), np.float32(-0.5)      # a clip of its own scalars
    got = native.prior_kl(dev(x0), a, lv).cpu().numpy()
    want, bound = H.prior_oracle(x0, a, lv)
    ratio = np.abs(got - want) / bound
    print(f"dc_prior_kl {shape}: worst |error| / bound {ratio.max():.4f}")
    assert (ratio <= 1.0).all(), (got, want, bound)
    assert np.array_equal(native.prior_kl(dev(x0), a, lv).cpu().numpy(), got)
    assert np.array_equal(native.prior_kl(dev(x0[:1]), a[:1], lv[:1]).cpu().numpy(), got[:1])


# ---- through the Python surface ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g19():
    return dict(golden("g19_vb_terms.npz"))


def diffusion(mean_type="START_X", var_type="FIXED_SMALL", steps=H.S):
    return GaussianDiffusion(betas=H.linear_betas(steps), model_mean_type=getattr(ModelMeanType, mean_type),
                             model_var_type=getattr(ModelVarType, var_type), loss_type=LossType.MSE)


@pytest.mark.parametrize("clip", (True, False))
@pytest.mark.parametrize("var_type", H.VAR_TYPES)
@pytest.mark.parametrize("mean_type", H.MEAN_TYPES)
def test_vb_terms_bpd_with_the_stub_models_matches_the_reference(g19, mean_type, var_type, clip):
    gd = diffusion(mean_type, var_type)
    for (B, T), ts in H.FIXTURE_CASES.items():
        tag = f"c_B{B}_T{T}_{mean_type}_{var_type}_clip{int(clip)}"
        c = H.make_case(B, T, 26, mean_type, var_type, clip, ts)
        want, bound, z, pred = H.case_oracle(c, mean_type, var_type, clip)
        assert H.band(z)[0] == 0
        fixed = dev(c["model_out"] if c["var_values"] is None else np.concatenate([c["model_out"], c["var_values"]], axis=1))
        out = gd._vb_terms_bpd(lambda *a, **k: fixed, dev(c["x0"]), dev(c["xt"]), torch.tensor(ts), clip_denoised=clip, noise=dev(c["noise"]))
        terms = out["terms"].cpu().numpy()
        assert out["terms"].is_cuda and np.array_equal(out["output"].cpu().numpy(), terms[:, 0])
        assert np.array_equal(out["pred_xstart"].cpu().numpy().reshape(B, -1), pred)      # _xstart_of: the affine stage, bit for bit
        check_against_oracle(terms, c, mean_type, var_type, clip, what=tag)
        f32, f64 = g19[tag + "_f32"].astype(np.float64), g19[tag + "_f64"]
        assert (np.abs(terms[:, :5] - f32) <= bound + np.abs(f32 - f64)).all(), tag


@pytest.mark.parametrize("mean_type,var_type", H.LOOP_TYPES)
def test_calc_bpd_loop_with_the_stub_models_matches_the_reference(g19, monkeypatch, mean_type, var_type):
    gd = diffusion(mean_type, var_type, H.LOOP_S)
    x0, fixed = H.loop_inputs(mean_type, var_type)
    steps = iter(range(H.LOOP_S - 1, -1, -1))
    monkeypatch.setattr(sampler.th, "randn_like", lambda x, **k: dev(H.loop_noise(next(steps))))
    fx = dev(fixed)
    rd = gd.calc_bpd_loop(lambda *a, **k: fx, dev(x0))
    assert next(steps, None) is None
    assert torch.equal(rd["total_bpd"], rd["vb"].sum(dim=1) + rd["prior_bpd"])      # (on the device: the sum's order is torch's there)
    r = {k: v.cpu().numpy() for k, v in rd.items()}
    B, tag = H.LOOP_B, f"loop_{mean_type}_{var_type}"
    want, bound, pw, pb = H.loop_oracle(mean_type, var_type)
    worst = {}
    for key, slot in (("vb", 0), ("xstart_mse", 3), ("mse", 4)):
        ratio = np.abs(r[key] - want[:, :, slot]) / bound[:, :, slot]
        worst[key] = float(ratio.max())
        assert (ratio <= 1.0).all(), (key, ratio.max())
        f32, f64 = g19[f"{tag}_{key}_f32"].astype(np.float64), g19[f"{tag}_{key}_f64"]
        assert (np.abs(r[key] - f32) <= bound[:, :, slot] + np.abs(f32 - f64)).all(), key
    assert (np.abs(r["prior_bpd"] - pw) <= pb).all()
    tot_bound = H.total_bound(want, bound, pw, pb)
    f32, f64 = g19[f"{tag}_total_bpd_f32"].astype(np.float64), g19[f"{tag}_total_bpd_f64"]
    assert (np.abs(r["total_bpd"] - (want[:, :, 0].sum(axis=1) + pw)) <= tot_bound).all()
    assert (np.abs(r["total_bpd"] - f32) <= tot_bound + np.abs(f32 - f64)).all()
    print(f"{tag}: worst |error| / bound {worst}; total_bpd {r['total_bpd'].tolist()} (reference {f32.tolist()})")


@pytest.fixture(scope="module")
def model():
    return make_model("fp16", DEV)


MODEL_B, MODEL_T, MODEL_S, MODEL_SEED = 3, 64, 25, 7


def test_calc_bpd_loop_with_the_denoiser_in_the_loop(model):
    gd = diffusion(steps=MODEL_S)
    betas = H.linear_betas(MODEL_S)
    x0 = synthetic_motion(MODEL_B, MODEL_T, seed=71).reshape(MODEL_B, MODEL_T, 26)
    xf_proj, xf_out = (t.to(DEV) for t in xf_pair(MODEL_B, MODEL_T))
    mk = {"xf_proj": xf_proj, "xf_out": xf_out}
    r = gd.calc_bpd_loop(model, dev(x0), model_kwargs=mk, noise_seed=MODEL_SEED)
    assert all(v.is_cuda for v in r.values())
    again = gd.calc_bpd_loop(model, dev(x0), model_kwargs=mk, noise_seed=MODEL_SEED)
    for key in r:      # (4) the seed reproduces the loop bit for bit
        assert torch.equal(r[key], again[key]), key
    assert tuple(r["vb"].shape) == (MODEL_B, MODEL_S) and bool(torch.isfinite(r["total_bpd"]).all())
    assert torch.equal(r["total_bpd"], r["vb"].sum(dim=1) + r["prior_bpd"])      # (2)
    other = gd.calc_bpd_loop(model, dev(x0), model_kwargs=mk, noise_seed=MODEL_SEED + 1)
    assert not torch.equal(other["mse"], r["mse"])
    worst = np.zeros(5)
    for col, t in enumerate(range(MODEL_S - 1, -1, -1)):
        tt = torch.full((MODEL_B,), t, dtype=torch.long)
        a, s = native.q_sample_coefficients(gd.alphas_cumprod, tt)
        x_t, nz = native.q_sample(dev(x0), a, s, noise_seed=(MODEL_SEED, t, 0), return_noise=True)
        out = gd._vb_terms_bpd(model, dev(x0), x_t, tt, model_kwargs=mk, noise=nz)
        terms = out["terms"].cpu().numpy()
        for key, slot in (("vb", 0), ("xstart_mse", 3), ("mse", 4)):      # the loop is these calls
            assert np.array_equal(r[key][:, col].cpu().numpy(), terms[:, slot]), (key, t)
        # (1) float64 from the RETURNED pred_xstart and the regenerated x_t: the model's own error stays out
        coef = H.coefficients(betas, "FIXED_SMALL", [t] * MODEL_B)
        pred, m1, m2 = H.stages_fp32(x0, x_t.cpu().numpy(), out["pred_xstart"].cpu().numpy(), coef, "START_X", True)
        assert np.array_equal(pred, out["pred_xstart"].cpu().numpy().reshape(MODEL_B, -1))
        want, bound, z = H.oracle(x0, x_t.cpu().numpy(), pred, m1, m2, coef, "FIXED_SMALL", None, nz.cpu().numpy())
        if t == 0:
            n_band, inner, saturated = H.band(z)
            print(f"t = 0: {n_band / z.size:.1%} of the elements between the regimes, {inner:.1%} inner, {saturated:.1%} saturated")
        ratio = np.abs(terms[:, :5] - want) / bound
        worst = np.maximum(worst, ratio.max(axis=0))
        assert (ratio <= 1.0).all(), (t, ratio.max(axis=0))
        # (3) the plain-torch definitions on the same tensors (denoised_fn routes there), inside the same bounds
        plain = gd._vb_terms_bpd(model, dev(x0), x_t, tt, model_kwargs=mk, noise=nz, denoised_fn=lambda x: x)
        assert torch.equal(plain["pred_xstart"], out["pred_xstart"])
        assert (np.abs(plain["terms"].cpu().numpy()[:, :5] - want) <= bound).all(), t
    print(f"denoiser in the loop: worst |error| / bound per slot {np.round(worst, 4).tolist()}; total_bpd {r['total_bpd'].tolist()}")
    sub = gd.calc_bpd_loop(model, dev(x0), model_kwargs=mk, noise_seed=MODEL_SEED, timesteps=[0, 24, 12])
    assert sub["total_bpd"] is None and torch.equal(sub["vb"], r["vb"][:, [0, 12, 24]])


# ---- harness and command line -------------------------------------------------------------------------------------------------------
VAL_T, VAL_CLIPS = 64, 5


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("bpd_clips")
    mel = batch_mel(VAL_CLIPS, 3 * VAL_T, 128, seed=41)
    motion = synthetic_motion(VAL_CLIPS, VAL_T, seed=42)
    for i in range(VAL_CLIPS):
        os.makedirs(root / f"clip{i}")
        np.save(root / f"clip{i}" / "mel.npy", mel[i])
        np.save(root / f"clip{i}" / "motion.npy", motion[i])
    return str(root), mel, motion


@pytest.fixture(scope="module")
def trainer(model):
    from diffusion_conductor_amd import DDPMTrainer
    tr = DDPMTrainer(types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=H.S, is_train=False), model)
    tr.eval_mode()
    return tr


def test_bound_bpd_returns_the_documented_numbers(trainer, dataset):
    _, mel, motion = dataset
    r = trainer.bound_bpd(mel, motion, m_lens=[64, 1, 17, 64, 200], timesteps=[0, 999, 500], seed=3)
    assert r["timesteps"] == [999, 500, 0] and r["total_bpd"] is None and r["mean_total_bpd"] is None
    assert r["vb"].shape == r["xstart_mse"].shape == r["mse"].shape == (VAL_CLIPS, 3) and r["prior_bpd"].shape == (VAL_CLIPS,)
    assert all(np.isfinite(r[k]).all() for k in ("vb", "xstart_mse", "mse", "prior_bpd", "mean_vb", "mean_xstart_mse", "mean_mse"))
    assert np.array_equal(r["mean_vb"], r["vb"].mean(axis=0)) and math.isfinite(r["mean_prior_bpd"])
    again = trainer.bound_bpd(mel, motion, m_lens=[64, 1, 17, 64, 200], timesteps=[0, 999, 500], seed=3)
    assert np.array_equal(again["vb"], r["vb"]) and np.array_equal(again["mse"], r["mse"])
    one = trainer.bound_bpd(mel[2], motion[2], timesteps=[500], seed=3)
    assert one["vb"].shape == (1, 1) and np.isfinite(one["vb"]).all()


def test_evaluate_bpd_prints_one_json_line(trainer, dataset, capsys):
    from diffusion_conductor_amd.evaluate import bound_dataset, bound_grid, main
    root = dataset[0]
    assert bound_grid(1000, 4) == [999, 666, 333, 0] and bound_grid(1000, 2) == [999, 0] and bound_grid(25, 25) == list(range(24, -1, -1))
    assert main(["--data_root", root, "--bpd", "--bpd_timesteps", "4", "--batch_size", "2", "--seed", "11"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    cli = json.loads(lines[0])
    assert cli["clips"] == VAL_CLIPS and cli["timesteps"] == [999, 666, 333, 0] and cli["total_bpd"] is None and cli["evaluations"] == 4
    assert [row["t"] for row in cli["per_timestep"]] == cli["timesteps"] and math.isfinite(cli["prior_bpd"])
    assert all(math.isfinite(row[k]) for row in cli["per_timestep"] for k in ("vb", "xstart_mse", "mse"))
    same = bound_dataset(trainer, root, timesteps=4, batch_size=2, seed=11)
    assert cli["per_timestep"] == json.loads(json.dumps(same["per_timestep"]))
    for extra in (["--val_loss"], ["--steps", "10"], ["--rhythm"], ["--smooth"]):
        with pytest.raises(SystemExit):
            main(["--data_root", root, "--bpd"] + extra)
    with pytest.raises(SystemExit):
        main(["--data_root", root, "--bpd_timesteps", "4"])
