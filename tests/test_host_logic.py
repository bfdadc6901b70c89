"""Host-side logic and the C ABI surface, on a CPU-only box (no compute calls into the GPU path)."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import ROOT, golden, state_dict_np

from diffusion_conductor_amd import native
from diffusion_conductor_amd.param_spec import DenoiserConfig, param_shapes


def test_library_loads_and_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "dc_ddim.h")).read()
    declared = set(re.findall(r"\b(dc_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"dc_sampler", "dc_config", "dc_status", "dc_precision"}
    assert declared == set(native.EXPORTS), declared ^ set(native.EXPORTS)
    L = native.lib()
    for name in declared:
        assert hasattr(L, name), name
    assert b"gfx950" in L.dc_version()


def test_dynamic_symbol_table_is_exactly_the_header():
    """The library is built with -fvisibility=hidden and the header marks its entry points DC_EXPORT: the functions the library
    defines in its dynamic symbol table (`nm -D --defined-only`, type T) are the header's and nothing else - no helper with C
    linkage, no C++-mangled launcher (round 3 exported `widen_coef` and 29 `_Z...` functions).  What remains beside them are
    weak libstdc++ template instantiations (W) and the HIP kernel handles (V), neither of which is an entry point."""
    import subprocess
    path = os.environ.get("DC_DDIM_LIB", native.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    defined = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] == "T"}
    defined -= {"_init", "_fini"}
    assert defined == set(native.EXPORTS), defined ^ set(native.EXPORTS)


def test_schedule_and_coefficients_match_reference_tables():
    """The C-ABI schedule helper reproduces the reference's fp64 tables BIT FOR BIT (numpy's linspace / cumprod order of
    operations).  The four fp32 step scalars: sqrt_recip / sqrt_recipm1 are casts of those tables (bit-equal); the two
    square roots are IEEE sqrtf, while the fixture holds torch's CPU `th.sqrt` (MKL VML), which is not correctly rounded on
    a handful of near-tie entries of the 1000-step table - those may differ by one ulp, nothing else may differ at all."""
    g = golden("g1_schedule.npz")
    for S in (50, 1000):
        tab = native.linear_beta_schedule(S)
        for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                  "sqrt_recipm1_alphas_cumprod"):
            assert np.array_equal(tab[k], g[f"S{S}_{k}"]), (S, k)
        co = native.ddim_coefficients(g[f"S{S}_alphas_cumprod"])
        ref = g[f"S{S}_step_coeff"][:, :4].astype(np.float32)
        assert np.array_equal(co[:, :2], ref[:, :2])
        ulp = np.abs(co[:, 2:].view(np.int32).astype(np.int64) - ref[:, 2:].view(np.int32).astype(np.int64))
        assert ulp.max() <= 1 and (ulp != 0).sum() <= S // 50, (S, ulp.max(), int((ulp != 0).sum()))
        # ... and every entry that differs is the correctly rounded one on the ABI's side
        ap = np.append(1.0, g[f"S{S}_alphas_cumprod"][:-1]).astype(np.float32)
        exact = np.stack([np.sqrt(ap.astype(np.float64)), np.sqrt((np.float32(1.0) - ap).astype(np.float64))], axis=1)
        bad = ulp != 0
        assert (np.abs(co[:, 2:].astype(np.float64) - exact)[bad] <= np.abs(ref[:, 2:].astype(np.float64) - exact)[bad]).all()
        assert co[0, 2] == 1.0 and co[0, 3] == 0.0


def test_coefficients_ex_match_the_oracles_fp32_scalars():
    """dc_ddim_coefficients_ex (eta > 0): sigma and sqrt(1 - abar_prev - sigma^2) in the reference's fp32 op order
    (gaussian_diffusion.py:814-826) - within 2 ulp of the oracle's torch evaluation; eta = 0 reproduces the 4-float table."""
    from helpers import O
    for S in (50, 1000):
        tab = O.ddim_tables(O.linear_beta_schedule(S))
        for eta in (0.0, 0.3, 1.0):
            ref = O.ddim_step_coefficients(tab, eta)
            co = native.ddim_coefficients(tab["alphas_cumprod"], eta)
            assert co.shape == (S, 8) and not co[:, 5:].any()
            assert np.allclose(co[:, :5], ref, rtol=3e-7, atol=1e-9), (S, eta, np.abs(co[:, :5] - ref).max())
            assert co[0, 4] == 0.0                                   # t = 0: no noise (the reference's nonzero_mask)
        assert np.array_equal(native.ddim_coefficients(tab["alphas_cumprod"], 0.0)[:, :4], native.ddim_coefficients(tab["alphas_cumprod"]))


def test_sampler_routes_every_model_branch_to_the_native_loop():
    """Which calls take the captured loop: START_X and EPSILON, any clip_denoised / eta; host callbacks do not."""
    from diffusion_conductor_amd import MotionTransformer
    from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType,
                                                 get_named_beta_schedule)
    m = MotionTransformer(input_feats=26, num_frames=64, num_layers=1, latent_dim=128, device="cpu", precision="auto")
    assert m.active_precision == "fp16" and m.check_numerics
    with pytest.raises(ValueError):
        MotionTransformer(input_feats=26, latent_dim=128, precision="fp8")
    for mt, ok in ((ModelMeanType.START_X, True), (ModelMeanType.EPSILON, True), (ModelMeanType.PREVIOUS_X, False)):
        gd = GaussianDiffusion(betas=get_named_beta_schedule("linear", 50), model_mean_type=mt,
                               model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)
        assert gd._fast_path_ok(m, None, None) is ok
        assert not gd._fast_path_ok(m, lambda x: x, None) and not gd._fast_path_ok(lambda *a, **k: None, None, None)
    assert gd.native_coefficients(0.5).shape == (50, 8) and gd.native_coefficients().shape == (50, 4)
    # numerics_fallback: only "auto" switches, once, and never for a FiLM tile outside the fp16 storage range
    assert not m.numerics_fallback(native.STATUS_F16_SATURATED) and m.active_precision == "fp16"
    assert m.numerics_fallback(native.STATUS_NONFINITE) and m.active_precision == "mixed"
    assert not m.numerics_fallback(native.STATUS_NONFINITE)
    m2 = MotionTransformer(input_feats=26, num_frames=64, num_layers=1, latent_dim=128, device="cpu", precision="fp16")
    assert not m2.numerics_fallback(native.STATUS_NONFINITE)
    assert "precision='mixed'" in native.describe_status(native.STATUS_NONFINITE, "fp16")


def test_gaussian_diffusion_tables_and_enums():
    from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType,
                                                 get_named_beta_schedule)
    g = golden("g1_schedule.npz")
    gd = GaussianDiffusion(betas=get_named_beta_schedule("linear", 50), model_mean_type=ModelMeanType.START_X,
                           model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)
    assert gd.num_timesteps == 50
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
              "sqrt_recipm1_alphas_cumprod"):
        assert np.array_equal(getattr(gd, k), g[f"S50_{k}"])
    assert gd.sample.__func__ is gd.ddim_sample_loop.__func__
    with pytest.raises(NotImplementedError):
        get_named_beta_schedule("quadratic", 10)
    with pytest.raises(AssertionError):
        GaussianDiffusion(betas=np.array([0.0, 0.5]), model_mean_type=ModelMeanType.START_X,
                          model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)


def _bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def _tile_row(r, hh):
    return (r & 3) + 8 * (r >> 2) + 4 * hh


def _mfma_32x32x16(a_frag, b_frag):
    """Reference semantics of v_mfma_f32_32x32x16_bf16 on lane-major fragments [64][8]:
    A[row = l&31][k = 8*(l>>5)+j], B[k = 8*(l>>5)+j][col = l&31]; returns D[32][32]."""
    A = np.zeros((32, 16), np.float64)
    Bm = np.zeros((16, 32), np.float64)
    for l in range(64):
        for j in range(8):
            A[l & 31, 8 * (l >> 5) + j] = a_frag[l, j]
            Bm[8 * (l >> 5) + j, l & 31] = b_frag[l, j]
    return A @ Bm


def _acc_to_frag(tile, s):
    """An accumulator tile D[32 rows][32 cols] as the next MFMA's operand fragment for k-step s:
    lane (c, hh) element j = register 8s+j = D[tile_row(8s+j, hh)][c]."""
    f = np.zeros((64, 8), np.float64)
    for l in range(64):
        for j in range(8):
            f[l, j] = tile[_tile_row(8 * s + j, l >> 5), l & 31]
    return f


@pytest.mark.parametrize("n_out,k_in", [(128, 128), (64, 128), (128, 64), (26, 128), (128, 26)])
def test_chained_weight_image_reproduces_matmul(n_out, k_in):
    """The packed weight image, consumed as the A operand against an activation that arrives as an
    accumulator tile (the in-register chaining the kernels rely on), reproduces W @ X exactly
    (integer-valued data, so bf16 and fp32 accumulation are exact)."""
    rng = np.random.default_rng(0)
    W = rng.integers(-8, 9, (n_out, k_in)).astype(np.float32)
    X = rng.integers(-8, 9, (k_in, 32)).astype(np.float32)          # [features][32 tokens]
    hi, lo = native.pack_weight(W, chained=True)
    OT, KT = (n_out + 31) // 32, (k_in + 31) // 32
    hi = _bf16_to_f32(hi).reshape(KT, OT, 2, 64, 8).transpose(1, 0, 2, 3, 4)     # image is kt-major
    assert not _bf16_to_f32(lo).any()                                  # small integers are exact in bf16
    Xp = np.zeros((KT * 32, 32), np.float32)
    Xp[:k_in] = X
    Y = np.zeros((OT * 32, 32))
    for ot in range(OT):
        for kt in range(KT):
            for s in range(2):
                Y[32 * ot:32 * ot + 32] += _mfma_32x32x16(hi[ot, kt, s], _acc_to_frag(Xp[32 * kt:32 * kt + 32], s))
    np.testing.assert_array_equal(Y[:n_out], W.astype(np.float64) @ X)
    # ... and as the B operand it yields X^T W^T (tokens on rows), the orientation K and V use
    Yt = np.zeros((32, OT * 32))
    for oc in range(OT):
        for kt in range(KT):
            for s in range(2):
                Yt[:, 32 * oc:32 * oc + 32] += _mfma_32x32x16(_acc_to_frag(Xp[32 * kt:32 * kt + 32], s), hi[oc, kt, s])
    np.testing.assert_array_equal(Yt[:, :n_out], (W.astype(np.float64) @ X).T)


def test_natural_weight_image_and_split_precision():
    rng = np.random.default_rng(1)
    W = rng.standard_normal((64, 512)).astype(np.float32)
    hi, lo = native.pack_weight(W, chained=False)
    hi = _bf16_to_f32(hi).reshape(2, 16, 2, 64, 8)          # natural-k images are [ot][ks]
    lo = _bf16_to_f32(lo).reshape(2, 16, 2, 64, 8)
    for (ot, kt, s, l, j) in [(0, 0, 0, 0, 0), (1, 7, 1, 45, 3), (1, 15, 1, 63, 7), (0, 9, 0, 32, 5)]:
        w = W[32 * ot + (l & 31), 32 * kt + 16 * s + 8 * (l >> 5) + j]
        assert abs(hi[ot, kt, s, l, j] - w) <= abs(w) * 2.0 ** -8
        assert abs(hi[ot, kt, s, l, j] + lo[ot, kt, s, l, j] - w) <= abs(w) * 2.0 ** -16


def test_param_spec_matches_reference_state_dict_layout():
    shapes = param_shapes(DenoiserConfig())
    sd = state_dict_np()
    assert len(shapes) == 396 and list(shapes) == list(sd)
    assert sum(int(np.prod(s)) for n, s in shapes.items() if not n.endswith("num_batches_tracked")
               and "running_" not in n) == 5952666          # parameter count of the reference model
    from diffusion_conductor_amd import MotionTransformer
    m = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device="cpu", no_clip=True)
    assert list(m.state_dict()) == list(shapes)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    assert torch.equal(m.generate_src_mask(5, torch.tensor([5, 2])), torch.tensor([[1., 1, 1, 1, 1], [1, 1, 0, 0, 0]]))


def test_no_gpu_fails_loudly_not_silently():
    """On a box without an MI355X the product refuses to run; it never falls back to CPU."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(native.DcError, match="no HIP device|no CPU fallback"):
        native.NativeSampler(DenoiserConfig())
    from diffusion_conductor_amd import MotionTransformer
    m = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 64, 26), torch.zeros(1, dtype=torch.long), length=[64],
          xf_proj=torch.zeros(1, 64, 64), xf_out=torch.zeros(1, 64, 64))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "diffusion-conductor_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "/root/reference" not in src, f


def test_shard_bounds_partition():
    from diffusion_conductor_amd.sharding import shard_bounds
    for n in (1, 7, 32, 256, 294):
        for w in (1, 2, 3, 8):
            b = [shard_bounds(n, r, w) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n and all(b[i][1] == b[i + 1][0] for i in range(w - 1))
            sizes = [hi - lo for lo, hi in b]
            assert max(sizes) - min(sizes) <= 1


def test_savgol_coefficients_match_scipy():
    """dc_savgol_coefficients (host) vs scipy.signal: row window/2 of the hat matrix is savgol_coeffs, and the edge rows
    reproduce savgol_filter(mode="interp") on unit impulses (tools/visualization.py:20-26 uses kernel 19 / 11, order 5)."""
    from scipy.signal import savgol_coeffs, savgol_filter
    from diffusion_conductor_amd import native
    for w, o in ((19, 5), (11, 5), (5, 2)):
        H = native.savgol_coefficients(w, o).astype(np.float64)
        assert np.allclose(H[w // 2], savgol_coeffs(w, o, use="dot"), atol=2e-6)
        eye = np.eye(w)
        ref = savgol_filter(eye, w, o, axis=0, mode="interp")       # column k = response to an impulse at k
        assert np.allclose(H, ref, atol=2e-6), (w, o)
    with pytest.raises(native.DcError):
        native.savgol_coefficients(18, 5)


def test_evaluate_dataset_host_logic(tmp_path):
    """Directory walk, batching, noise independence of batch size and the reference's MSE bookkeeping
    (eval_new.py:104-134) with a stand-in sampler (no GPU)."""
    import torch
    from diffusion_conductor_amd import evaluate as ev
    rng = np.random.default_rng(0)
    for i in (3, 1, 2, 10):
        d = tmp_path / f"clip{i:02d}"
        d.mkdir()
        np.save(d / "mel.npy", rng.random((270, 128), dtype=np.float32))
        np.save(d / "motion.npy", rng.standard_normal((90, 13, 2)).astype(np.float32))
    (tmp_path / "stray").mkdir()                     # no npy files: skipped
    assert ev.list_clips(str(tmp_path)) == ["clip01", "clip02", "clip03", "clip10"]

    class FakeTrainer:
        calls = []

        def generate_music_motion(self, mel, dim_pose, noise=None, **kw):
            self.calls.append(mel.shape[0])
            return noise * 0.5 + mel[:, ::3, :dim_pose]      # any deterministic per-clip function of (mel, noise)

    a = ev.evaluate_dataset(FakeTrainer(), str(tmp_path), 26, batch_size=3, seed=7, verbose=False)
    b = ev.evaluate_dataset(FakeTrainer(), str(tmp_path), 26, batch_size=1, seed=7, verbose=False)
    assert a["clips"] == 4 and FakeTrainer.calls[:2] == [3, 1]
    assert a["per_clip"] == b["per_clip"] and abs(a["final_mse"] - b["final_mse"]) < 1e-6
    # the reference's arithmetic for one clip
    mel = np.load(tmp_path / "clip02" / "mel.npy")
    pred = (ev.clip_noise(7, 1, 90, 26) * 0.5 + torch.from_numpy(mel)[::3, :26]).numpy().reshape(90, 13, 2)
    assert a["per_clip"]["clip02"] == float(ev.mse_loss(np.load(tmp_path / "clip02" / "motion.npy"), pred))
    # like the reference, the running total stays in the precision of the per-clip values (float32 numpy scalars)
    assert abs(a["total_loss"] - sum(a["per_clip"][k] for k in sorted(a["per_clip"]))) < 1e-5


def test_evaluate_dataset_resamples_a_non_finite_early_batch(tmp_path):
    """A batch whose poses come back non-finite from the unchecked pipelined pass is sampled again through the checked path (where
    precision="auto" falls back) when the results are collected - also when it is an EARLY batch, whose error the sampling loop meets
    while it frees that batch's pinned slot two batches later (that wait must not raise)."""
    import torch
    from diffusion_conductor_amd import evaluate as ev
    rng = np.random.default_rng(1)
    for i in range(9):
        d = tmp_path / f"clip{i:02d}"
        d.mkdir()
        np.save(d / "mel.npy", rng.random((270, 128), dtype=np.float32))
        np.save(d / "motion.npy", rng.standard_normal((90, 13, 2)).astype(np.float32))

    class Enc:
        check_numerics = True

    class FakeTrainer:
        def __init__(self, poison):
            self.encoder, self.poison, self.calls, self.checked_calls = Enc(), poison, 0, 0

        def generate_music_motion(self, mel, dim_pose, noise=None, **kw):
            k = self.calls
            self.calls += 1
            out = noise * 0.5 + mel[:, ::3, :dim_pose]
            if self.encoder.check_numerics:
                self.checked_calls += 1                          # the checked path: finite (the fallback precision)
                return out
            if k == self.poison:
                out = out.clone()
                out[0, 5, 3] = float("inf")
            return out

    clean = ev.evaluate_dataset(FakeTrainer(-1), str(tmp_path), 26, batch_size=2, seed=3, verbose=False)      # 5 batches
    for poison in (0, 1, 4):
        tr = FakeTrainer(poison)
        got = ev.evaluate_dataset(tr, str(tmp_path), 26, batch_size=2, seed=3, verbose=False)
        assert tr.checked_calls == 1 and tr.calls == 6, (poison, tr.calls, tr.checked_calls)
        assert got["per_clip"] == clean["per_clip"]
        assert tr.encoder.check_numerics is True                  # restored

    class Unchecked(FakeTrainer):                                 # no check to fall back to: the error surfaces
        def __init__(self, poison):
            super().__init__(poison)
            self.encoder.check_numerics = False
    with pytest.raises(FloatingPointError):
        ev.evaluate_dataset(Unchecked(0), str(tmp_path), 26, batch_size=2, seed=3, verbose=False)


class _SeenBatches:
    """Base of the stand-ins below: counts, per method, which batch's ground truth (or mel) it was handed.  `firsts`: batch -> the
    flattened first clip of that batch's input; anything else (sampled poses, latents) is not counted."""

    def __init__(self, firsts):
        self.firsts, self.seen = firsts, {}

    def note(self, method, x):
        row = torch.as_tensor(x)[0].reshape(-1)
        for k, first in enumerate(self.firsts):
            if row.shape == first.shape and torch.equal(row, first):
                self.seen[(method, k)] = self.seen.get((method, k), 0) + 1


class _AllFamilies:
    """Pure-torch stand-ins for every score family of evaluate_dataset, each a deterministic function of one clip's input (no reduction
    across the batch), so a clip's row cannot depend on the pass that produced it."""
    idx, w = torch.arange(64) % 26, torch.linspace(-1.0, 1.5, 64)

    class Encoder(_SeenBatches):
        def latent(self, x):
            self.note("latent", x)
            B, T = x.shape[0], x.shape[1]
            return (x.reshape(B, T, 26)[:, :, _AllFamilies.idx] * _AllFamilies.w).transpose(1, 2).contiguous()

    class M2SNet(_SeenBatches):
        def __init__(self, firsts, mel_firsts):
            super().__init__(firsts)
            self.mels = _SeenBatches(mel_firsts)

        def music_latent(self, mel):
            self.mels.note("music_latent", mel)
            mel = torch.as_tensor(mel)
            T = (mel.shape[1] - 1) // 3 + 1
            return mel[:, :3 * T:3, :64].contiguous()

        def motion_latent(self, x):
            self.note("motion_latent", x)
            B, T = x.shape[0], x.shape[1]
            return (0.1 * x.reshape(B, T, 26)[:, :, _AllFamilies.idx] * _AllFamilies.w).transpose(1, 2).contiguous()

        def fuse(self, mus, mot):
            return torch.sigmoid(4.0 * (mus * mot.transpose(1, 2)).sum(2))

        def fuse_pairs(self, mus, mot):
            p = torch.stack([torch.stack([self.fuse(mus[i:i + 1], mot[j:j + 1])[0] for j in range(mot.shape[0])]) for i in range(mus.shape[0])])
            return {"mean": p.mean(2), "above": (p > 0.5).sum(2).int(), "below": (p < 0.5).sum(2).int(),
                    "count": torch.full(p.shape[:2], p.shape[2], dtype=torch.int32)}

    class Rhythm(_SeenBatches):
        def psd(self, x):
            self.note("psd", x)
            return (x.reshape(x.shape[0], -1, 26)[:, :32] ** 2).mean(2)

        def contour_and_std(self, x):
            self.note("contour_and_std", x)
            B, T = x.shape[0], x.shape[1]
            W = (T - 60) // 30 + 1
            x = x.reshape(B, T, 26)
            return x[:, :30 * W].reshape(B, W, 30 * 26).abs().mean(2), x.reshape(B, -1).std(1)

        def motion_beats(self, x):
            self.note("motion_beats", x)
            x = x.reshape(x.shape[0], -1, 26)
            return (x[:, :, 0] > x[:, :, 1] + 1.0).to(torch.uint8)

        def beat_scores(self, motion_beats, music_beats, music_stride=1, counts=False):
            mo, mu = motion_beats.float(), torch.as_tensor(music_beats).float()
            at = (mu * torch.arange(mu.shape[1])).sum(1) * music_stride          # (zeros behind a clip's last beat change nothing)
            scores = torch.stack([mo.mean(1) + 1e-4 * at, mo[:, ::2].mean(1) - 1e-4 * at], dim=1)
            n = torch.stack([mu.sum(1), mo.sum(1)], dim=1).to(torch.int32)
            return (scores, n) if counts else scores

    class Critic(_SeenBatches):
        def forward(self, x):
            self.note("forward", x)
            return (x.reshape(x.shape[0], -1) * 0.01).sum(1)


def test_evaluate_dataset_resamples_a_batch_with_every_score_family_on(tmp_path, monkeypatch):
    """The re-sample path with the latent, sync (+ retrieval), movement and beat scores all switched on: whichever batch is poisoned,
    every key but the timings is exactly the clean run's, the checked path ran once, every stand-in saw the poisoned batch's ground
    truth twice and every other batch's once, and each batch's ground truth is stacked once per pass, not once per family."""
    from diffusion_conductor_amd import evaluate as ev
    rng = np.random.default_rng(2)
    n, T, bs = 5, 256, 2                                            # (T = 256: the smallest the rhythm scores accept)
    mels, gts = rng.random((n, 3 * T - 2, 128), dtype=np.float32), rng.standard_normal((n, T, 13, 2)).astype(np.float32)
    beats = {}
    for i in range(n):
        d = tmp_path / f"clip{i:02d}"
        d.mkdir()
        np.save(d / "mel.npy", mels[i])
        np.save(d / "motion.npy", gts[i])
        beats[f"clip{i:02d}"] = (np.arange(3 * T - 2 - 7 * i) % (40 + i) == 3).astype(np.uint8)       # lengths differ: padded per batch
    firsts = [torch.from_numpy(gts[k]).reshape(-1) for k in range(0, n, bs)]
    mel_firsts = [torch.from_numpy(mels[k]).reshape(-1) for k in range(0, n, bs)]

    class Enc:
        check_numerics = True

    class FakeTrainer:
        def __init__(self, poison):
            self.encoder, self.poison, self.calls, self.checked_calls = Enc(), poison, 0, 0

        def generate_music_motion(self, mel, dim_pose, noise=None, **kw):
            k = self.calls
            self.calls += 1
            out = noise * 0.5 + torch.as_tensor(mel)[:, ::3, :dim_pose]
            if self.encoder.check_numerics:
                self.checked_calls += 1
                return out
            if k == self.poison:
                out = out.clone()
                out[0, 5, 3] = float("inf")
            return out

    stacks = []                                                     # clips per np.stack of ground truths (arrays of T * 26 values)
    stack = np.stack

    def recording_stack(arrays, *a, **kw):
        if np.size(arrays[0]) == T * 26:
            stacks.append(len(arrays))
        return stack(arrays, *a, **kw)
    monkeypatch.setattr(ev.np, "stack", recording_stack)

    def run(poison):
        tr = FakeTrainer(poison)
        parts = {"motion_encoder": _AllFamilies.Encoder(firsts), "m2snet": _AllFamilies.M2SNet(firsts, mel_firsts),
                 "rhythm": _AllFamilies.Rhythm(firsts), "discriminator": _AllFamilies.Critic(firsts)}
        del stacks[:]
        r = ev.evaluate_dataset(tr, str(tmp_path), 26, batch_size=bs, seed=3, verbose=False, music_beats=beats, beat_stride=3,
                                retrieval=True, diversity_seed=1, **parts)
        return tr, parts, r, list(stacks)

    timing = {"seconds", "frames_per_s", "steady_frames_per_s", "main_thread_s", "metrics_s", "m2s_retrieval_s"}
    _, _, clean, _ = run(-1)
    assert {"fgd", "m2s_sync_gen", "m2s_mean_rank_gen", "rde", "w_distance", "bc_gen", "beat_align_real"} <= set(clean)
    assert all(v == v for k, v in clean.items() if isinstance(v, float))          # (a NaN would equal nothing below)
    for poison in (0, 1, 2):                                         # first, middle, last (a batch of one clip)
        tr, parts, got, stacked = run(poison)
        assert list(got) == list(clean)
        for key in clean:
            if key not in timing:
                assert got[key] == clean[key], (poison, key)
        assert tr.checked_calls == 1 and tr.calls == 4, (poison, tr.calls, tr.checked_calls)
        assert tr.encoder.check_numerics is True                     # restored
        seen = dict(parts["m2snet"].mels.seen)
        for p in parts.values():
            seen.update(p.seen)
        assert sorted({m for m, _ in seen}) == ["contour_and_std", "forward", "latent", "motion_beats", "motion_latent", "music_latent", "psd"]
        for (method, k), count in seen.items():
            assert count == (2 if k == poison else 1), (poison, method, k, count)
        # one stack of the ground truth per batch pass, shared by the four families: three batches and the re-sampled one
        assert stacked == [2, 2, 1] + [1 if poison == 2 else 2], (poison, stacked)


def _isa_of(src, tmp_path):
    """Device ISA + resource remarks of one HIP source (hipcc cross-compiles without a GPU)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out_s = str(tmp_path / (os.path.basename(src) + ".s"))
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value",
                          src, "-o", out_s, "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return open(out_s).read(), out.stderr


def _compiler_m0_uses(isa):
    """Lines outside inline-asm blocks that name M0: the LDS-DMA statements of dc_dev.h overwrite M0 without restoring it, which is
    sound only while the compiler itself never keeps a value there (it treats M0 as reserved and refuses a clobber)."""
    import re
    hits, inasm = [], False
    for ln in isa.split("\n"):
        if "#ASMSTART" in ln:
            inasm = True
        elif "#ASMEND" in ln:
            inasm = False
        elif not inasm and re.search(r"\bm0\b", ln) and not ln.strip().startswith(";"):
            hits.append(ln.strip())
    return hits


def test_production_layer_kernel_has_no_register_spills(tmp_path):
    """Performance guard: the production k_layer instantiations sit at 249 - 254 of 256 VGPRs without a spill; a change that
    tips them over costs scratch traffic in the kernel that is 55 % of the loop.  (Until round 4 this was a correctness guard:
    the FiLM-tile prefetch used loads the compiler could not see.  It is compiler-tracked now, dc_dev.h epre_load.)
    Correctness guard of round 5's LDS-DMA statements: no compiler-generated use of M0 anywhere in the kernels' ISA."""
    import re
    csrc = os.path.join(ROOT, "diffusion-conductor_amd", "csrc")
    isa, remarks = _isa_of(os.path.join(csrc, "dc_kernels.hip"), tmp_path)
    assert _compiler_m0_uses(isa) == []
    spills = {}
    name = None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and name:
            spills[name] = int(m.group(1))
    # non-split, no hooks, WGR, per-layer launches: 8-wave form with / without stamps, the narrow (4-wave) form, and the two production
    # forms once more for G' scale tiles (loops with a precise tail) - times two operand types
    prod = [k for k in spills if re.match(r"_Z7k_layerIDF16[_b]Lb0ELb0ELb[01]ELb1ELb[01]ELb[01]EE", k)]
    assert len(prod) == 10, prod
    assert all(spills[k] == 0 for k in prod), {k: spills[k] for k in prod}
    # the 16-token kernel of the small-batch path (one wave per SIMD, bounds of 2: no AGPR half, no spills)
    isa16, remarks16 = _isa_of(os.path.join(csrc, "dc_layer16.hip"), tmp_path)
    assert _compiler_m0_uses(isa16) == []
    l16 = re.findall(r"Function Name: (_Z9k_layer16\S+).*?AGPRs: (\d+).*?VGPRs Spill: (\d+)", remarks16, flags=re.S)
    assert len(l16) == 4 and all(int(a) == 0 and int(sp) == 0 for _, a, sp in l16), l16          # (two operand types x G' - 1 / G' tiles)


# ---- tools/visualization.py-shaped entry point: reading a training run's opt.txt ------------------------------------------
def test_get_opt_reads_a_training_runs_opt_txt(tmp_path):
    from diffusion_conductor_amd.visualize import get_opt, make_parser
    p = tmp_path / "opt.txt"
    p.write_text("------------ Options -------------\n"
                 "batch_size: 32\ncheckpoints_dir: ./checkpoints\ndataset_name: ConductorMotion100\ndiffusion_steps: 50\n"
                 "gpu_id: [0]\nis_train: True\nlatent_dim: 128\nlr: 0.0002\nname: train\nno_clip: True\nnum_epochs: 500\n"
                 "unit_length: 4\nweird: 1e-4\nneg: -3\nnegf: -0.5\nplus: +7\nnote: a value: with a colon\n"
                 "-------------- End ----------------\n")
    opt = get_opt(str(p), "cuda:0")
    assert opt.batch_size == 32 and isinstance(opt.batch_size, int)
    assert opt.lr == 0.0002 and isinstance(opt.lr, float)
    assert opt.no_clip is True and opt.no_eff is False          # no_eff absent -> the default an old opt.txt implies
    assert opt.gpu_id == "[0]" and opt.weird == "1e-4"          # neither an integer nor digits.digits: stays text
    assert opt.neg == -3 and opt.negf == -0.5 and opt.plus == 7 and opt.note == "a value: with a colon"
    assert opt.num_layers == 8 and opt.latent_dim == 128 and opt.diffusion_steps == 50
    assert opt.which_epoch == "latest" and opt.is_train is False and opt.is_continue is False
    assert opt.max_motion_length == 1800 and opt.joints_num == 13 and opt.dim_pose == 26
    assert opt.model_dir == os.path.join("./checkpoints", "ConductorMotion100", "train", "model") and opt.device == "cuda:0"
    (tmp_path / "bad.txt").write_text("dataset_name: t2m\ncheckpoints_dir: x\nname: y\nunit_length: 4\n")
    with pytest.raises(KeyError, match="Dataset not recognized"):
        get_opt(str(tmp_path / "bad.txt"), "cpu")
    (tmp_path / "short.txt").write_text("dataset_name: ConductorMotion100\nname: y\n")
    with pytest.raises(KeyError, match="checkpoints_dir"):
        get_opt(str(tmp_path / "short.txt"), "cpu")
    a = make_parser().parse_args(["--opt_path", "o", "--music_path", "m.npy"])
    assert a.npy_path == "" and a.motion_length == 60 and a.result_path == "test_sample.gif"      # the reference's defaults


def test_visualize_load_mels(tmp_path):
    from diffusion_conductor_amd.visualize import load_mels
    np.save(tmp_path / "a.npy", np.zeros((90, 128), np.float32))
    np.save(tmp_path / "b.npy", np.ones((90, 128), np.float64))
    m, names = load_mels(str(tmp_path))
    assert m.shape == (2, 90, 128) and m.dtype == np.float32 and names == ["a.npy", "b.npy"]
    m, _ = load_mels(str(tmp_path / "b.npy"))
    assert m.shape == (90, 128)
    with pytest.raises(ValueError, match="audio decoding"):
        load_mels(str(tmp_path / "song.mp3"))


def test_bench_parent_spawns_one_process_per_gpu():
    """`python bench.py --gpus 2` without WORLD_SIZE is the parent: it starts 2 ranks itself and returns their worst exit
    code.  In this CPU container every rank stops at the `needs MI355X` assert - after having received its RANK."""
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("CPU-container test (on a GPU box both ranks would share cuda:0 / need cuda:1)")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DC_BENCH_WORKER")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert r.stderr.count("AssertionError: bench.py needs MI355X GPUs") == 2, r.stderr[-2000:]
    assert "WORLD_SIZE=" not in r.stderr                      # the ranks saw WORLD_SIZE == --gpus


def test_bench_parent_launches_eight_ranks(tmp_path):
    """The launcher at N = 8 (the driver's scaling run), with a stub in place of the rank program: eight processes, ranks 0..7,
    one rendezvous (127.0.0.1, one port, HSA_ENABLE_IPC_MODE_LEGACY=0), the arguments forwarded, rank 0's JSON line on the
    parent's stdout and the worst child code as the parent's own."""
    import json
    import subprocess
    import sys
    stub = tmp_path / "rank_stub.py"
    stub.write_text(
        "import json, os, sys\n"
        "r = int(os.environ['RANK'])\n"
        "rec = {k: os.environ.get(k) for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'LOCAL_WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT',"
        " 'HSA_ENABLE_IPC_MODE_LEGACY')}\n"
        "rec['argv'] = sys.argv[1:]\n"
        "open(os.path.join(os.environ['STUB_OUT'], f'rank{r}.json'), 'w').write(json.dumps(rec))\n"
        "if r == 0: print(json.dumps({'metric': 'stub', 'n_gpus': int(os.environ['WORLD_SIZE'])}), flush=True)\n"
        "sys.exit(int(os.environ.get('STUB_FAIL_RANK', '-1')) == r and 7 or 0)\n")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(DC_BENCH_WORKER=str(stub), STUB_OUT=str(tmp_path))
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "3", "--warmup", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"metric": "stub", "n_gpus": 8}
    recs = [json.loads((tmp_path / f"rank{i}.json").read_text()) for i in range(8)]
    assert [int(x["RANK"]) for x in recs] == list(range(8)) == [int(x["LOCAL_RANK"]) for x in recs]
    assert {x["WORLD_SIZE"] for x in recs} == {"8"} == {x["LOCAL_WORLD_SIZE"] for x in recs}
    assert {x["MASTER_ADDR"] for x in recs} == {"127.0.0.1"} and len({x["MASTER_PORT"] for x in recs}) == 1
    assert {x["HSA_ENABLE_IPC_MODE_LEGACY"] for x in recs} == {"0"}
    assert all(x["argv"] == ["--gpus", "8", "--steps", "3", "--warmup", "1"] for x in recs)
    r = subprocess.run(cmd, env=dict(env, STUB_FAIL_RANK="5"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 7                                   # a failing rank is the parent's exit code


def test_prefetcher_hands_loader_errors_to_the_consumer(tmp_path):
    """A failing loader thread must raise in take(), not leave the previous batch behind."""
    from diffusion_conductor_amd.evaluate import _Prefetcher
    for i in range(3):
        d = tmp_path / f"{i:03d}"
        d.mkdir()
        np.save(d / "mel.npy", np.zeros((9, 128), np.float32) if i < 2 else np.zeros((7, 128), np.float32))
        np.save(d / "motion.npy", np.zeros((3, 13, 2), np.float32))
    pf = _Prefetcher(str(tmp_path), ["000", "001", "002"], 2, (9, 128))
    pf.start(0)
    ids, mel, gts = pf.take()
    assert ids == ["000", "001"] and len(gts) == 2
    pf.start(1)                                               # clip 002 has the wrong mel shape
    with pytest.raises(ValueError, match="002/mel.npy"):
        pf.take()


def test_pinned_host_encode_chunk_boundaries():
    """denoiser._h2d_bounds: a first chunk, then the rest; explicit schedules; every clip exactly once, in order."""
    from diffusion_conductor_amd.denoiser import MotionTransformer
    f = MotionTransformer._h2d_bounds
    assert f(32, [8, 24]) == [(0, 8), (8, 32)] and f(16, [8, 8]) == [(0, 8), (8, 16)] and f(5, [8, 1]) == [(0, 5)]
    assert f(9, [8, 1]) == [(0, 8), (8, 9)] and f(19, [4, 12, 16]) == [(0, 4), (4, 16), (16, 19)]
    assert f(40, [8, 8, 8]) == [(0, 8), (8, 16), (16, 40)] and f(1, [8, 1]) == [(0, 1)]
    sched = lambda B: f(B, [max(1, B // d) for d in MotionTransformer.h2d_schedule] + [B])      # the default: growing chunks
    assert sched(32) == [(0, 4), (4, 8), (8, 16), (16, 32)] and sched(17) == [(0, 2), (2, 4), (4, 8), (8, 17)]
    for B in range(1, 70):
        for r in (f(B, [8, max(1, B - 8)]), sched(B)):
            assert r[0][0] == 0 and r[-1][1] == B and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(lo < hi for lo, hi in r)


def test_push_set_carries_nothing_the_gpu_pool_refuses():
    """The shared MI355X machines refuse any run that would execute a file carrying a GPU-sanitizer or XNACK request (round 5's
    GPU suite was refused for exactly that).  Walk what the repository carries - the files git tracks, or the whole tree where there
    is no git work tree - and fail on XNACK requests anywhere, and on any sanitizer option that is not limited to host code: each one
    has `-Xarch_host` right before it, or its line carries `-fno-gpu-sanitize` and no other `-Xarch_` option.  Records that quote the
    refusal (VERDICT, GPUTEST, ...) are never executed; they are skipped."""
    import fnmatch
    import subprocess
    san = "-fsanitize" + "="
    triggers = ("HSA_" + "XNACK", "xnack" + "+")
    records = ("VERDICT.md", "ADVICE.md", "GPUTEST_r*.json", "BENCH_r*.json", "SCALE_r*.json", "MULTICHIP_r*.json", "PROGRESS.jsonl",
               "COPYCHECK.json", "PAPERS.md", "SNIPPETS.md")
    r = subprocess.run(["git", "ls-files", "--cached", "--others", "--exclude-standard", "-z"], cwd=ROOT, capture_output=True, text=True)
    if r.returncode == 0 and os.path.isdir(os.path.join(ROOT, ".git")):
        files = [f for f in r.stdout.split("\0") if f]
    else:
        files = []
        for d, dirs, fs in os.walk(ROOT):
            dirs[:] = [x for x in dirs if not x.startswith(".") and x not in ("__pycache__", "build")]
            files += [os.path.relpath(os.path.join(d, f), ROOT) for f in fs]
    host_only = re.compile(r"-Xarch_host\W{0,6}" + re.escape(san))
    bad, san_lines = [], {}
    for rel in files:
        p = os.path.join(ROOT, rel)
        if ("/" not in rel and any(fnmatch.fnmatch(rel, g) for g in records)) or not os.path.isfile(p):
            continue
        if os.path.getsize(p) > 8 << 20 or rel.endswith((".so", ".o", ".alt", ".npz", ".npy", ".pyc")):
            continue
        try:
            text = open(p, encoding="utf-8").read()
        except (UnicodeDecodeError, OSError):
            continue
        bad += [(rel, t) for t in triggers if t in text]
        for line in text.splitlines():
            if san in line:
                san_lines[rel] = san_lines.get(rel, 0) + 1
                if line.count(san) != len(host_only.findall(line)) and not ("-fno-gpu-sanitize" in line and "-Xarch_" not in line):
                    bad.append((rel, line.strip()[:160]))
    assert not bad, f"files carry what the GPU machines refuse: {bad}"
    assert san_lines.get(os.path.join("tests", "test_host_sanitize.py"), 0) >= 2       # the host sanitizer build is seen, and passes


_G11_CASES = [("prevx_small_clip", "PREVIOUS_X", "FIXED_SMALL", False, True, 0.0),
              ("prevx_large_eta", "PREVIOUS_X", "FIXED_LARGE", False, True, 0.4),
              ("startx_learned_clip", "START_X", "LEARNED", False, True, 0.0),
              ("eps_range_eta", "EPSILON", "LEARNED_RANGE", False, False, 0.3),
              ("startx_cond", "START_X", "FIXED_SMALL", True, False, 0.0),
              ("eps_cond_clip_eta", "EPSILON", "FIXED_SMALL", True, True, 0.2),
              ("prevx_range_cond", "PREVIOUS_X", "LEARNED_RANGE", True, True, 0.1)]


@pytest.mark.parametrize("tag,mean,var,cond,clip,eta", _G11_CASES)
def test_sampler_off_path_branches_g11(tag, mean, var, cond, clip, eta):
    """ModelMeanType.PREVIOUS_X (gaussian_diffusion.py:510-514, 545), the learned-variance output split (:472-486) and cond_fn /
    condition_score (:581-603, 806-808) of the step-through path against the imported reference's outputs on weight-free callables
    (fixture G11, oracle/toy_models.py): samples and pred_xstart of three iterations, the final sample, p_mean_variance's whole dict."""
    import torch
    from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule
    from oracle import toy_models as TM
    g = np.load(os.path.join(ROOT, "tests", "golden", "g11_offpath_branches.npz"))
    S = 50
    gd = GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=getattr(ModelMeanType, mean),
                           model_var_type=getattr(ModelVarType, var), loss_type=LossType.MSE)
    mdl = TM.toy_model_learned if var.startswith("LEARNED") else TM.toy_model
    x_T, z = torch.from_numpy(g["toy_x_T"]), torch.from_numpy(g["toy_z"])
    kw = dict(noise=x_T, clip_denoised=clip, cond_fn=TM.toy_cond_fn if cond else None, eta=eta, device="cpu", model_kwargs={"scale": 0.8},
              step_noise=z)
    outs = list(gd.ddim_sample_loop_progressive(mdl, TM.SHAPE, **kw))

    def close(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return np.linalg.norm(a - b) <= 2e-6 * max(np.linalg.norm(b), 1e-30)
    assert len(outs) == S
    for it in (0, 24, 49):
        assert close(outs[it]["sample"], g[f"toy_{tag}_sample{it}"]), (tag, it)
        assert close(outs[it]["pred_xstart"], g[f"toy_{tag}_pred{it}"]), (tag, it)
    res = gd.ddim_sample_loop(mdl, TM.SHAPE, idxs=[24], **kw)          # the dict form: {iteration: sample} + {S: final}
    assert set(res) == {24, S} and close(res[S], g[f"toy_{tag}_final"]) and close(res[24], g[f"toy_{tag}_sample24"])
    pmv = gd.p_mean_variance(mdl, x_T, torch.tensor([49, 7, 0]), clip_denoised=clip, model_kwargs={"scale": 0.8})
    for k in ("mean", "variance", "log_variance", "pred_xstart"):
        assert close(pmv[k].expand(TM.SHAPE), g[f"toy_{tag}_pmv_{k}"]), (tag, k)
