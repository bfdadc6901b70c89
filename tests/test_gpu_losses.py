"""The held-out denoising losses on the MI355X (csrc/dc_loss.hip, sampler.py, harness.py, evaluate.py) against the reference's
numbers of tests/golden/g14_training_losses.npz (tools/make_golden_losses.py) and fp64 numpy.

Reduction tolerance.  dc_motion_loss_terms and dc_latent_l1 run ONE workgroup of THREADS = 256 threads per clip; a thread adds up
its share in a serial fp32 chain, then a fixed tree of DEPTH = 8 levels (6 butterflies in a wave, 2 over the 4 waves) combines the
partials.  Every addend is a float64 difference squared (or its absolute value) rounded once, and the sum is divided once:
    relative error <= (longest chain + DEPTH + 3) * 2^-24          (sums of non-negative terms)
  motion terms: a thread takes float2 pairs, chain = ceil(13 T / 256) + 1 (the pair's own sum)     T = 1800: 104 * 2^-24 = 6.2e-6
  latent L1:    a thread takes float4 quads, chain = ceil(16 T / 256) + 2 (the quad's own tree)     T = 1800: 126 * 2^-24 = 7.5e-6
Both are below the 3e-5 the fixture's shapes may use at most.

Model in the loop: three assertions keep the model's error and the kernels' apart - (1) the returned prediction against the
reference's, the project's standing 1e-3 rel-L2 per clip; (2) the returned terms against an fp64 recomputation from the RETURNED
tensors, the reduction tolerance; (3) the returned terms against the REFERENCE's terms, inside a bound computed from the data: with
d = target - pred_ref and delta = pred - pred_ref, | |d - delta|^2 - |d|^2 | <= 2 |d| |delta| + |delta|^2, the same through the
frame-difference operator D with |D delta| <= 2 |delta|, and for the latent term the triangle inequality over the latent difference
the test measures, mean |f(pred) - f(pred_ref)|, plus what the ST-GCN kernels may differ from the reference's encoder on equal
inputs: their standing bound, 1e-5 rel-L2 per clip (tests/test_gpu_motion_encoder.py), so at most 1e-5 (rms f(pred_ref) + rms f(target))
in the mean.  Measured figures: DESIGN.md section 11.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from helpers import make_model, rel_l2
from helpers_losses import CASES_A, CASES_B, MEAN_TYPES, S, case_inputs, check_digests, g14, latent_l1_fp64, rel, terms_fp64

from diffusion_conductor_amd import metrics, native
from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN
from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule
from diffusion_conductor_amd.synthetic import batch_mel, batch_noise, synthetic_motion, synthetic_motion_encoder_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
THREADS, DEPTH = 256, 8          # DC_LOSS_THREADS and the tree of block_tree (csrc/dc_loss.hip)
PRED_TOL, ENCODER_TOL = 1e-3, 1e-5


def terms_tol(T):
    return (math.ceil(13 * T / THREADS) + 1 + DEPTH + 3) * 2.0 ** -24


def l1_tol(T):
    return (math.ceil(16 * T / THREADS) + 2 + DEPTH + 3) * 2.0 ** -24


def diffusion(mean_type="START_X"):
    return GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=getattr(ModelMeanType, mean_type),
                             model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


@pytest.fixture(scope="module")
def encoder():
    return MotionEncoder_STGCN(DEV).load_state_dict(synthetic_motion_encoder_state_dict(0))


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(precision):
        if precision not in cache:
            cache[precision] = make_model(precision, DEV)
        return cache[precision]
    return get


def test_tolerances_stay_inside_what_the_shapes_may_use():
    assert terms_tol(1800) < 3e-5 and l1_tol(1800) < 3e-5
    assert native.lib() and native.LOSS_TERMS == 8


# ---- dc_q_sample ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", CASES_A)
def test_q_sample_with_explicit_noise_is_the_reference_bit_for_bit(B, T):
    g, tag = g14(), f"a_B{B}_T{T}"
    x0, noise, stub = case_inputs(B, T)
    check_digests(tag, x0, noise, stub)
    x_t = diffusion().q_sample(dev(x0), torch.from_numpy(g[f"{tag}_t"]), noise=dev(noise))
    assert x_t.is_cuda and tuple(x_t.shape) == x0.shape
    assert np.array_equal(x_t.cpu().numpy(), g[f"{tag}_START_X_x_t"])
    flat = diffusion().q_sample(dev(x0.reshape(B, T, 26)), g[f"{tag}_t"], noise=dev(noise.reshape(B, T, 26)))     # [B, T, 26] too
    assert np.array_equal(flat.cpu().numpy().reshape(x0.shape), g[f"{tag}_START_X_x_t"])


@pytest.mark.parametrize("B,T", ((3, 33), (2, 1800)))       # T * 26 no multiple of 4: the scalar form; 46 800: the vector form, 46 blocks
def test_seeded_q_sample_is_the_explicit_one_on_the_step_noise_draws(B, T):
    x0 = dev(synthetic_motion(B, T, seed=31).reshape(B, T, 26))
    a, s = native.q_sample_coefficients(diffusion().alphas_cumprod, [S - 1, 0, 250][:B])
    seed, it = 0x1234567890abcdef, 5
    z = native.step_noise((B, T, 26), seed, it, DEV)
    want = native.q_sample(x0, a, s, noise=z)
    got, drawn = native.q_sample(x0, a, s, noise_seed=(seed, it, 0), return_noise=True)
    assert torch.equal(drawn, z) and torch.equal(got, want)
    assert torch.equal(native.q_sample(x0, a, s, noise_seed=(seed, it, 0)), want)      # the draws land in x_t and are replaced in place
    assert not torch.equal(native.q_sample(x0, a, s, noise_seed=(seed, it + 1, 0)), want)


@pytest.mark.parametrize("B,T,pos", ((3, 33, 2), (3, 5, 1)))        # first_element 1716, and 130 - not a multiple of the draw's quads
def test_a_clips_seeded_noising_does_not_depend_on_the_batch_around_it(B, T, pos):
    gd = diffusion()
    x0 = dev(synthetic_motion(B, T, seed=32))
    t = torch.tensor([17, 999, 400][:B])
    whole = gd.q_sample(x0, t, noise_seed=(7, 3, 0))
    alone = gd.q_sample(x0[pos:pos + 1].contiguous(), t[pos:pos + 1], noise_seed=(7, 3, pos * T * 26))
    assert torch.equal(alone[0], whole[pos])


# ---- the reductions ---------------------------------------------------------------------------------------------------------------
def _check_terms(pred, target, length, T, what):
    got = native.motion_loss_terms(dev(pred), dev(target), length)
    again = native.motion_loss_terms(dev(pred), dev(target), length)
    assert torch.equal(got, again), "a rerun must be bit-identical"
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and not got[:, 6:].any()
    want = terms_fp64(pred, target, length)
    err = np.abs(got[:, :6] - want[:, :6]) / want[:, :6]
    print(f"dc_motion_loss_terms {what}: relative error per slot {err.max(axis=0)} (tolerance {terms_tol(T):.2e})")
    assert err.max() <= terms_tol(T), (what, err)
    return got


@pytest.mark.parametrize("mean_type", MEAN_TYPES)
@pytest.mark.parametrize("B,T", CASES_A)
def test_motion_loss_terms_against_fp64_on_the_fixtures_tensors(B, T, mean_type):
    g, tag = g14(), f"a_B{B}_T{T}"
    x0, noise, stub = case_inputs(B, T)
    pred = (g[f"{tag}_stub_scale"] * stub).astype(np.float32)
    target = (x0 if mean_type == "START_X" else noise).reshape(B, T, 26)
    got = _check_terms(pred, target, g[f"{tag}_length"], T, f"{tag} {mean_type}")
    assert rel(got[:, :6], g[f"{tag}_{mean_type}_terms"][:, :6]) <= 3e-5        # ... and the reference's own fp32 numbers


def test_motion_loss_terms_at_full_length_and_every_ragged_length():
    B, T = 2, 1800
    x0, noise, _ = case_inputs(B, T)
    pred = g14()[f"b_B{B}_T{T}_START_X_pred"]
    _check_terms(pred, x0.reshape(B, T, 26), [1800, 1234], T, "b_B2_T1800")
    T = 33
    x0, noise, stub = case_inputs(3, T)
    for length in ([1, 17, 33], [33, 33, 33], [1, 1, 1], None):
        got = _check_terms(stub, noise.reshape(3, T, 26), [T] * 3 if length is None else length, T, f"T=33 lengths {length}")
        if length is None:
            assert torch.equal(native.motion_loss_terms(dev(stub), dev(noise.reshape(3, T, 26))).cpu(), torch.from_numpy(got))
    with pytest.raises(native.DcError):
        native.motion_loss_terms(dev(stub), dev(noise.reshape(3, T, 26)), [0, 1, 1])
    with pytest.raises(native.DcError):
        native.motion_loss_terms(dev(stub[:, :1]), dev(noise.reshape(3, T, 26)[:, :1]))


@pytest.mark.parametrize("B,T", CASES_A + ((2, 1800),))
def test_latent_l1_against_fp64(encoder, B, T):
    x0, noise, stub = case_inputs(B, T)
    a, b = encoder.latent(dev(x0)), encoder.latent(dev(stub.reshape(B, T, 13, 2)))
    got = native.latent_l1(a, b)
    assert torch.equal(got, native.latent_l1(a, b)), "a rerun must be bit-identical"
    err = rel(got.cpu().numpy(), latent_l1_fp64(a.cpu().numpy(), b.cpu().numpy()))
    print(f"dc_latent_l1 B={B} T={T}: relative error {err:.2e} (tolerance {l1_tol(T):.2e})")
    assert tuple(got.shape) == (B,) and err <= l1_tol(T)
    assert torch.equal(native.latent_l1(a[B - 1:].contiguous(), b[B - 1:].contiguous())[0], got[B - 1])      # batch-invariant


# ---- the model in the loop --------------------------------------------------------------------------------------------------------
def _norm(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).sum(axis=tuple(range(1, np.ndim(a)))))


@pytest.mark.parametrize("precision", ("fp16", "bf16x3"))
@pytest.mark.parametrize("mean_type", MEAN_TYPES)
@pytest.mark.parametrize("B,T", CASES_B)
def test_training_losses_with_the_denoiser(models, encoder, B, T, mean_type, precision):
    g, tag = g14(), f"b_B{B}_T{T}"
    x0, noise, _, mel = case_inputs(B, T, mel=True)
    check_digests(tag, x0, noise, mel)
    length, t = g[f"{tag}_length"], g[f"{tag}_t"]
    ref_pred, ref_terms, ref_l1 = (g[f"{tag}_{mean_type}_{k}"] for k in ("pred", "terms", "latent_l1"))
    if T == 1800:
        assert np.array_equal(ref_pred[:, g["latent_T1800_frames"]], g[f"{tag}_{mean_type}_pred_windows"])
    out = diffusion(mean_type).training_losses(models(precision), dev(x0), torch.from_numpy(t), noise=dev(noise),
                                               model_kwargs={"text": dev(mel), "length": torch.from_numpy(length)})
    pred, target, terms = out["pred"].cpu().numpy(), out["target"].cpu().numpy(), out["terms"].cpu().numpy()
    assert np.array_equal(target, (x0 if mean_type == "START_X" else noise).reshape(B, T, 26))
    assert tuple(out["mse"].shape) == (B,) and out["velocity"].dim() == 0 and torch.equal(out["mse"], out["terms"][:, 0])
    fake, real, fake_ref = (encoder.latent(dev(v.reshape(B, T, 13, 2))) for v in (pred, target, ref_pred))
    l1 = native.latent_l1(fake, real).cpu().numpy()
    # (1) the model: the standing parity bound, per clip
    e_pred = [rel_l2(pred[b], ref_pred[b]) for b in range(B)]
    # (2) the kernels: against fp64 on the tensors they were given
    e_kernel = rel(terms[:, :6], terms_fp64(pred, target, length)[:, :6])
    e_l1 = rel(l1, latent_l1_fp64(fake.cpu().numpy(), real.cpu().numpy()))
    # (3) against the reference's terms, inside the bound the data gives
    p64, r64, t64 = (np.asarray(v, np.float64) for v in (pred, ref_pred, target))
    delta, d = p64 - r64, t64 - r64
    n, mask = T * 26, (np.arange(T)[None, :] < length[:, None])[:, :, None]
    D = lambda v: v[:, 1:] - v[:, :-1]      # noqa: E731
    groups = {2: [10, 11, 12, 13, 22, 23, 24, 25], 3: list(range(14, 22)), 4: list(range(10))}

    def quad(base, dl):       # | |base - dl|^2 - |base|^2 | <= 2 |base| |dl| + |dl|^2
        return 2 * base * dl + dl ** 2
    bound = np.zeros((B, 6))
    bound[:, 0] = quad(_norm(d), _norm(delta)) / n
    bound[:, 1] = quad(_norm(d * mask), _norm(delta * mask)) / 26
    for slot, idx in groups.items():
        bound[:, slot] = quad(_norm(D(r64)[:, :, idx]), 2 * _norm(delta[:, :, idx])) / ((T - 1) * len(idx))
    bound[:, 5] = quad(_norm(D(t64) - D(r64)), 2 * _norm(delta)) / ((T - 1) * 26)
    bound += 2 * terms_tol(T) * np.abs(ref_terms[:, :6])                      # both sides are rounded fp32 reductions
    diff = np.abs(terms[:, :6].astype(np.float64) - ref_terms[:, :6])
    fr = fake_ref.cpu().numpy().astype(np.float64)
    rms = lambda v: np.sqrt((np.asarray(v, np.float64) ** 2).mean(axis=(1, 2)))      # noqa: E731
    l1_bound = np.abs(fake.cpu().numpy() - fr).mean(axis=(1, 2)) + ENCODER_TOL * (rms(fr) + rms(real.cpu().numpy())) * (1 + ENCODER_TOL) \
        + 2 * l1_tol(T) * np.abs(ref_l1)
    l1_diff = np.abs(l1.astype(np.float64) - ref_l1)
    print(f"{tag} {mean_type} {precision}: pred rel-L2 {max(e_pred):.2e}; terms vs fp64 {e_kernel:.2e}, latent L1 vs fp64 {e_l1:.2e}; "
          f"terms vs reference, relative, per slot {(diff / np.abs(ref_terms[:, :6])).max(axis=0)} (share of the bound "
          f"{(diff / bound).max(axis=0)}); latent L1 vs reference {(l1_diff / ref_l1).max():.2e} (share {(l1_diff / l1_bound).max():.2f})")
    assert max(e_pred) <= PRED_TOL, e_pred
    assert e_kernel <= terms_tol(T) and e_l1 <= l1_tol(T), (e_kernel, e_l1)
    assert (diff <= bound).all(), (diff, bound)
    assert (l1_diff <= l1_bound).all(), (l1_diff, l1_bound)


# ---- the surfaces -----------------------------------------------------------------------------------------------------------------
VAL_T, VAL_CLIPS = 64, 5
ROW_KEYS = {"t", "loss", "loss_mot_rec", "loss_mot_feat", "loss_velocity", "loss_velocity_elbow", "loss_velocity_head", "loss_velocity_body",
            "velocity_elbow", "mse", "feat_included"}


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("val_clips")
    mel = batch_mel(VAL_CLIPS, 3 * VAL_T, 128, seed=41)
    motion = synthetic_motion(VAL_CLIPS, VAL_T, seed=42)
    for i in range(VAL_CLIPS):
        os.makedirs(root / f"clip{i}")
        np.save(root / f"clip{i}" / "mel.npy", mel[i])
        np.save(root / f"clip{i}" / "motion.npy", motion[i])
    return str(root), mel, motion


@pytest.fixture(scope="module")
def trainer(models):
    import types

    from diffusion_conductor_amd import DDPMTrainer
    tr = DDPMTrainer(types.SimpleNamespace(device=torch.device(DEV), diffusion_steps=S, is_train=False), models("fp16"))
    tr.eval_mode()
    return tr


def test_validation_losses_returns_the_documented_numbers(trainer, encoder, dataset):
    _, mel, motion = dataset
    r = trainer.validation_losses(mel, motion, m_lens=[64, 1, 17, 64, 200], t=[0, 999, 500, 250, 750], seed=3, motion_encoder=encoder)
    assert r["t"] == [0, 999, 500, 250, 750] and len(r["mse_per_clip"]) == VAL_CLIPS and r["terms"].shape == (VAL_CLIPS, 8)
    assert r["feat_included"] is True and r["latent_l1"].shape == (VAL_CLIPS,) and math.isfinite(r["loss"])
    want = metrics.denoising_loss_scalars(r["terms"], [64, 1, 17, 64, 64], r["latent_l1"])
    assert all(r[k] == want[k] for k in want)
    again = trainer.validation_losses(mel, motion, m_lens=[64, 1, 17, 64, 200], t=[0, 999, 500, 250, 750], seed=3, motion_encoder=encoder)
    assert np.array_equal(again["terms"], r["terms"]) and again["loss"] == r["loss"]
    plain = trainer.validation_losses(mel, motion, m_lens=[64, 1, 17, 64, 200], t=[0, 999, 500, 250, 750], seed=3)
    assert plain["loss_mot_feat"] is None and plain["feat_included"] is False and np.array_equal(plain["terms"], r["terms"])
    assert plain["loss"] == pytest.approx(r["loss"] - 1e-6 * r["loss_mot_feat"], rel=1e-12)
    # t=None: one uniform timestep per clip from the seed, on the host; one clip as [Tm, 128] / [T, 13, 2]
    d1, d2 = (trainer.validation_losses(mel, motion, seed=s) for s in (5, 5))
    assert d1["t"] == d2["t"] and all(0 <= v < S for v in d1["t"]) and d1["loss"] == d2["loss"]
    one = trainer.validation_losses(mel[2], motion[2], t=500, seed=3)
    assert one["t"] == [500] and one["terms"].shape == (1, 8) and math.isfinite(one["loss"])
    # explicit noise: the reference's protocol; a clip's numbers do not depend on the batch around it
    nz = batch_noise(VAL_CLIPS, VAL_T, 26, seed=43)
    whole = trainer.validation_losses(mel, motion, t=[0, 999, 500, 250, 750], noise=nz)
    part = trainer.validation_losses(mel[3:], motion[3:], t=[250, 750], noise=nz[3:])
    assert np.array_equal(part["terms"], whole["terms"][3:])


def test_validation_dataset_does_not_depend_on_the_batch_size(trainer, encoder, dataset, capsys):
    from diffusion_conductor_amd.evaluate import main, validation_dataset, validation_grid
    root = dataset[0]
    assert validation_grid(S, 3) == [0, 500, 999] and validation_grid(S, 1) == [0] and validation_grid(50, 50) == list(range(50))
    r5 = validation_dataset(trainer, root, timesteps=3, batch_size=5, seed=11, motion_encoder=encoder)
    r2 = validation_dataset(trainer, root, timesteps=3, batch_size=2, seed=11, motion_encoder=encoder)
    r5 = json.loads(json.dumps(r5))                      # what the command line prints
    assert r5["clips"] == VAL_CLIPS and r5["timesteps"] == [0, 500, 999] and r5["evaluations"] == 3
    assert [row["t"] for row in r5["per_timestep"]] == [0, 500, 999] and all(set(row) == ROW_KEYS for row in r5["per_timestep"])
    assert all(math.isfinite(row["loss"]) and row["feat_included"] and row["loss_mot_feat"] > 0 for row in r5["per_timestep"])
    assert math.isfinite(r5["average"]["loss"])
    assert r5["average"]["loss"] == pytest.approx(np.mean([row["loss"] for row in r5["per_timestep"]]), rel=1e-12)
    assert r2["per_timestep"] == r5["per_timestep"] and r2["average"] == r5["average"]
    listed = validation_dataset(trainer, root, timesteps=[500], batch_size=5, seed=11, limit=3)
    assert listed["clips"] == 3 and listed["per_timestep"][0]["loss_mot_feat"] is None and not listed["average"]["feat_included"]
    assert "loss_mot_feat" in listed["average"] and listed["average"]["loss_mot_feat"] is None
    drawn = [validation_dataset(trainer, root, batch_size=b, seed=11) for b in (2, 5)]      # the one-draw-per-clip protocol
    assert drawn[0]["timesteps"] is None and drawn[0]["per_timestep"] == drawn[1]["per_timestep"] and drawn[0]["evaluations"] == 1
    # the command line: one JSON line, no sampling loop (its own model on the same seeded weights)
    capsys.readouterr()
    assert main(["--data_root", root, "--val_loss", "--val_timesteps", "3", "--batch_size", "2", "--seed", "11"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    cli = json.loads(lines[0])
    no_feat = validation_dataset(trainer, root, timesteps=3, batch_size=5, seed=11)
    assert cli["per_timestep"] == json.loads(json.dumps(no_feat["per_timestep"])) and cli["timesteps"] == [0, 500, 999]
