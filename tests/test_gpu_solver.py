"""Sampling on a sub-sequence of a 1000-step checkpoint's timesteps, first order (DDIM) or second order (DPM-Solver++ 2M), inside the
captured loop (include/dc_ddim.h, dc_solver_table / dc_sampler_solver_loop).  Needs an MI355X.

One caller shape per update site (the names of tests/test_gpu_guided.py) against helpers_solver.solver_loop, the oracle's loop
restated on the sub-schedule plus the history term; the seeded model of helpers.make_model, make_diffusion(1000), n = 25 timesteps
unless said.

Bounds, per clip of >= 100 frames (rel-L2).  Order 1 is a DDIM loop on another schedule: the project's gate, 1e-3, or
1e-3 (|w| + |w - 1|) when guided (tests/test_gpu_guided.py).  Order 2: 1e-3 for `mixed`; fp16 / bf16 1e-3 A with A = 2, the factor by
which the second-order update carries more of an evaluation's error to the final sample than DDIM does on the same list - measured in
the fp64 oracle alone (tools/solver_amplification.py: every evaluation's output perturbed by seeded relative noise of 1e-4; the
largest ratio of the final deviations over these shapes and both spacings is 1.82 - "uniform" spacing, 1.01 with "logsnr" - floored
at 1 and rounded up to one digit; profiles/solver_gpu_tests.txt).  The two ragged 2 x 96 batches take their bound over the valid
frames of the whole batch."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import batch_mel, batch_noise, make_diffusion, make_model, oracle_params, rel_l2, xf_pair
from helpers_known import prefix_mask, unknown_rel_l2
from helpers_solver import solver_loop

from diffusion_conductor_amd import native
from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule,
                                             spaced_timesteps)
from diffusion_conductor_amd.synthetic import batch_step_noise

pytestmark = pytest.mark.gpu
S, N, P, W, A = 1000, 25, 26, 2.0, 2.0
ORDER = {"ddim": 1, "dpmpp2m": 2}

# name -> (model key, the caller's B, T, lengths or None, guidance scale or None)
SHAPES = {"layer16": ("fp16", 1, 256, None, None),
          "narrow": ("fp16", 36, 256, None, None),
          "wide_aligned": ("fp16", 80, 256, None, None),
          "wide_flat": ("fp16", 55, 300, None, None),
          "group_96": ("fp16", 2, 96, [96, 70], None),
          "no_eff": ("no_eff", 2, 96, [96, 70], None),
          "bf16": ("bf16", 1, 256, None, None),
          "mixed": ("mixed", 1, 256, None, None),
          "guided": ("fp16", 1, 256, None, W)}


def tol(key, solver, w=None):
    t = 1e-3 * (abs(w) + abs(w - 1)) if (w is not None and key != "mixed") else 1e-3
    return t * (A if (solver == "dpmpp2m" and key != "mixed") else 1.0)


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    made = {}

    def get(key):
        if key not in made:
            made[key] = make_model("fp16", no_eff=True) if key == "no_eff" else make_model(key)
        return made[key]
    return get


_inputs, _refs, _gd = {}, {}, {}


def _diffusion(steps=S, eps=False):
    if (steps, eps) not in _gd:
        _gd[steps, eps] = make_diffusion(steps) if not eps else GaussianDiffusion(
            betas=get_named_beta_schedule("linear", steps), model_mean_type=ModelMeanType.EPSILON, model_var_type=ModelVarType.FIXED_SMALL,
            loss_type=LossType.MSE)
    return _gd[steps, eps]


def _list(spacing, n=N):
    return spaced_timesteps(_diffusion().alphas_cumprod, n, spacing)


def _setup(name):
    if name not in _inputs:
        _, B, T, length, _ = SHAPES[name]
        xfp, xfo = xf_pair(B, T, first=60)
        _inputs[name] = dict(B=B, T=T, length=length or [T] * B, xfp=xfp, xfo=xfo, x=torch.from_numpy(batch_noise(B, T, first=60)),
                             known=0.5 * torch.from_numpy(batch_noise(B, T, first=260)), eps=torch.from_numpy(batch_noise(B, T, first=460)))
    return _inputs[name]


def _clips(B):
    return [2, 3, B - 1 if (B - 1) % 4 != 1 else B - 3] if B > 3 else list(range(B))


def _gpu(model, d, ts=None, solver="ddim", w=None, gd=None, idxs=(), mask=None, **kw):
    """ddim_sample_loop on the list `ts` (None: no solver keyword at all - today's call)."""
    gd = gd or _diffusion()
    if mask is not None:
        kw.update(known=d["known"].cuda(), known_mask=mask.cuda(), known_noise=d["eps"].cuda())
    if ts is not None:
        kw.update(timesteps=ts, solver=solver)
    kw.setdefault("clip_denoised", False)
    out = gd.ddim_sample_loop(model, (d["B"], d["T"], P), noise=d["x"].cuda(), progress=False, idxs=list(idxs), guidance_scale=w,
                              model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda(), "length": torch.LongTensor(d["length"])}, **kw)
    torch.cuda.synchronize()
    return out


def _oracle(name, clips, ts, solver, w=None, mask=None, tag="", steps=S, **kw):
    """The checker's run of `clips` of a shape alone, computed once per (shape, clips, list, solver, branch)."""
    key = (name, tuple(clips), tuple(ts), solver, w, tag, steps)
    if key not in _refs:
        d = _setup(name)
        c = torch.tensor(clips)
        if "step_noise" in kw:
            kw["step_noise"] = kw["step_noise"][:, c]
        kn = dict(known=d["known"][c], mask=mask[c], eps=d["eps"][c]) if mask is not None else {}
        _refs[key] = solver_loop(oracle_params(), d["x"][c], d["xfp"][c], d["xfo"][c], [d["length"][i] for i in clips], steps, ts,
                                 ORDER[solver], w=w, no_eff=SHAPES[name][0] == "no_eff", **kn, **kw)
    return _refs[key]


def _errors(name, out, ref, clips):
    d = _setup(name)
    if d["T"] >= 100:
        return {c: rel_l2(out[c], ref[j]) for j, c in enumerate(clips)}
    valid = prefix_mask(d["B"], d["T"], P, d["length"]) != 0      # clips shorter than 100 frames: the batch's valid frames as one figure
    return {"batch": rel_l2(out[valid], ref[valid])}


@pytest.mark.parametrize("spacing", ["uniform", "logsnr"])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_against_the_checker(models, name, solver, spacing):
    """1: the figures go to DESIGN.md section 4.8 and profiles/solver_gpu_tests.txt."""
    key, B, T, _, w = SHAPES[name]
    d, ts = _setup(name), _list(spacing)
    out = _gpu(models(key), d, ts, solver, w=w).cpu()
    assert torch.isfinite(out).all()
    clips = _clips(B)
    errs = _errors(name, out, _oracle(name, clips, ts, solver, w=w), clips)
    worst = max(errs.values())
    print(f"solver parity {name} {solver} {spacing} n={len(ts)}: worst {worst:.3e} (bound {tol(key, solver, w):.1e})  " +
          " ".join(f"[{c}] {e:.2e}" for c, e in errs.items()))
    assert worst <= tol(key, solver, w), errs


@pytest.mark.parametrize("variant", ["plain", "eta", "known", "guided"])
@pytest.mark.parametrize("name", ["layer16", "wide_aligned", "no_eff"])
def test_full_sequence_is_todays_loop(models, name, variant):
    """2: timesteps = 24 .. 0 of a 25-step schedule at order 1 against ddim_sample_loop without the keywords: the same bits."""
    key, B, T, _, _ = SHAPES[name]
    d, m, gd = _setup(name), models(key), _diffusion(25)
    kw, mask, w = {}, None, None
    if variant == "eta":
        kw = dict(eta=0.5, step_noise=torch.from_numpy(batch_step_noise(25, B, T, first=60)).cuda())
    elif variant == "known":
        mask = prefix_mask(B, T, P, [40] * B)
        mask[:, :, 5] = 1
    elif variant == "guided":
        w = W
    want = _gpu(m, d, None, gd=gd, w=w, mask=mask, idxs=(3,), **kw)
    got = _gpu(m, d, list(range(24, -1, -1)), "ddim", gd=gd, w=w, mask=mask, idxs=(3,), **kw)
    for it in (3, 25):
        assert torch.isfinite(got[it]).all() and torch.equal(got[it], want[it]), (name, variant, it, rel_l2(got[it], want[it]))


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("name", ["layer16", "narrow", "wide_aligned"])
def test_eager_equals_captured(models, name, solver, monkeypatch):
    """3: a strided loop under DC_DISABLE_GRAPH=1 (read per call) - every step launches k_begin_step, which looks the step's row up -
    gives the bits of the captured loop.  Timesteps up to 999 on tables of 25 rows: the rows are indexed by iteration."""
    key, B, T, _, _ = SHAPES[name]
    d, m, ts = _setup(name), models(key), _list("logsnr")
    captured = _gpu(m, d, ts, solver, idxs=(3,))
    monkeypatch.setenv("DC_DISABLE_GRAPH", "1")
    eager = _gpu(m, d, ts, solver, idxs=(3,))
    monkeypatch.delenv("DC_DISABLE_GRAPH")
    for it in (3, len(ts)):
        assert torch.isfinite(eager[it]).all() and torch.equal(eager[it], captured[it]), (name, solver, it, rel_l2(eager[it], captured[it]))


@pytest.mark.parametrize("solver", ["ddim", "dpmpp2m"])
def test_profile_loop_runs_strided(models, solver):
    """3: dc_sampler_solver_profile_loop - the eager pass with per-kernel events - on the list, inside the bound."""
    name = "layer16"
    key, B, T, _, _ = SHAPES[name]
    d, m, ts = _setup(name), models(key), _list("logsnr")
    nat = m.set_conditioning(d["xfp"].cuda(), d["xfo"].cuda(), d["length"])
    nat.set_known(None, None, None)
    nat.set_smoothing(0, 0)
    rows = native.solver_table(_diffusion().alphas_cumprod, ts, 0.0, ORDER[solver])[0]
    prof, out = nat.solver_profile_loop(d["x"].cuda(), ts, rows)
    assert nat.status() == 0 and prof["k_begin_step"][1] == len(ts) and prof["k_film_gemm"][1] == len(ts)
    e = rel_l2(out[0], _oracle(name, [0], ts, solver)[0])
    print(f"solver profile loop {name} {solver}: {e:.3e} (bound {tol(key, solver):.1e})")
    assert e <= tol(key, solver)


def test_history_crosses_graph_replays(models):
    """4: n = 96 is two replays of 48 captured steps, the precise tail in the second graph; order 2 against the checker."""
    name = "layer16"
    key, B, T, _, _ = SHAPES[name]
    d, ts = _setup(name), _list("uniform", 96)
    assert len(ts) == 96
    out = _gpu(models(key), d, ts, "dpmpp2m", idxs=(47, 48))
    ref = _oracle(name, [0], ts, "dpmpp2m", idxs=(47, 48))
    errs = {it: rel_l2(out[it][0], ref[it][0]) for it in (47, 48, 96)}
    print("solver n=96 dpmpp2m layer16: " + " ".join(f"[{it}] {e:.2e}" for it, e in errs.items()) + f" (bound {tol(key, 'dpmpp2m'):.1e})")
    assert max(errs.values()) <= tol(key, "dpmpp2m")


def test_another_list_reuses_the_graph(models):
    """5: another list of the same length on a used sampler gives the bits of a fresh sampler; snapshots match the checker."""
    name = "layer16"
    key, B, T, _, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    ts_a, ts_b = _list("logsnr"), _list("uniform")
    assert len(ts_a) == len(ts_b) == N and ts_a != ts_b
    snaps = (0, 3, N - 1)
    a = _gpu(m, d, ts_a, "dpmpp2m", idxs=snaps)
    b = _gpu(m, d, ts_b, "dpmpp2m", idxs=snaps)
    a2 = _gpu(m, d, ts_a, "dpmpp2m", idxs=snaps)
    want = _gpu(make_model(key), d, ts_b, "dpmpp2m", idxs=snaps)
    ref = _oracle(name, [0], ts_b, "dpmpp2m", idxs=snaps, tag="snaps")
    assert sorted(b) == sorted(snaps + (N,))
    for it in snaps + (N,):
        assert torch.equal(a[it], a2[it]) and torch.equal(b[it], want[it]) and not torch.equal(a[it], b[it])
        e = rel_l2(b[it][0], ref[it][0])
        print(f"solver snapshot {it}: {e:.3e}")
        assert e <= tol(key, "dpmpp2m")
    assert torch.equal(b[N - 1], b[N])           # the snapshot behind the last iteration is the final sample


def test_off_means_off(models):
    """6: after an order-2 loop, a plain ddim_sample_loop and an order-1 loop on the same sampler give the bits of a fresh sampler."""
    name = "layer16"
    key, B, T, _, _ = SHAPES[name]
    d, m, fresh, ts = _setup(name), models(key), make_model(key), _list("logsnr")
    gd25 = _diffusion(25)
    want_plain, want_o1 = _gpu(fresh, d, None, gd=gd25, idxs=(3,)), _gpu(fresh, d, ts, "ddim", idxs=(3,))
    second = _gpu(m, d, ts, "dpmpp2m", idxs=(3,))
    plain = _gpu(m, d, None, gd=gd25, idxs=(3,))
    _gpu(m, d, ts, "dpmpp2m")
    o1 = _gpu(m, d, ts, "ddim", idxs=(3,))
    for it, n in ((3, 3), (25, N)):
        assert torch.equal(plain[it], want_plain[it]) and torch.equal(o1[n], want_o1[n]) and not torch.equal(second[n], want_o1[n])


@pytest.mark.parametrize("branch", ["clip", "eps", "known", "smooth"])
def test_sampler_branches(models, branch):
    """7: 1 x 256 at order 2 against the checker.  With clipping the history holds the clipped prediction.  (The EPSILON case clips, as
    tests/test_gpu_known.py's does and for its reason: DESIGN.md section 4.6.)"""
    name, solver = "layer16", "dpmpp2m"
    key, B, T, _, _ = SHAPES[name]
    d, m, ts = _setup(name), models(key), _list("logsnr")
    mask, gkw, okw = None, {}, {}
    if branch in ("clip", "eps"):
        gkw, okw = dict(clip_denoised=True), dict(clip_denoised=True, eps_model=branch == "eps")
    elif branch == "known":
        mask = prefix_mask(B, T, P, [100])
        mask[:, :, 5] = 1
    elif branch == "smooth":
        gkw = dict(smooth=(19, 5))
    out = _gpu(m, d, ts, solver, gd=_diffusion(S, eps=True) if branch == "eps" else None, mask=mask, **gkw).cpu()
    ref = _oracle(name, [0], ts, solver, mask=mask, tag=branch, **okw)
    assert torch.isfinite(out).all()
    if branch == "known":
        k = mask != 0
        assert torch.equal(out[k], d["known"][k])                                 # bit for bit
        e = unknown_rel_l2(out[0], ref[0], mask[0])
    elif branch == "smooth":
        unsmoothed = _gpu(m, d, ts, solver)
        assert torch.equal(out, native.savgol_filter(unsmoothed, 19, 5).cpu()) and not torch.equal(out, unsmoothed.cpu())
        e = rel_l2(unsmoothed[0], ref[0])
    else:
        if branch == "clip":
            assert float(ref.abs().max()) == 1.0                                  # (the clamp does act on this model)
        e = rel_l2(out[0], ref[0])
    print(f"solver branch {branch} {solver}: {e:.3e} (bound {tol(key, solver):.1e})")
    assert e <= tol(key, solver)


def test_long_piece_has_exact_seams(models):
    """7: generate_long_music_motion on two windows of 256 frames with steps=25, solver="dpmpp2m": the frames the windows share are
    the same bits in both, and the piece is the hand-written chain of loops around known values."""
    from diffusion_conductor_amd import DDPMTrainer
    from diffusion_conductor_amd.harness import plan_windows
    T, ov, Tm = 256, 64, 1344
    L = (Tm - 1) // 3 + 1
    assert plan_windows(L, T, ov) == [(0, 0), (192, 64)]
    m = models("fp16")
    tr = DDPMTrainer(Namespace(device="cuda", diffusion_steps=S, is_train=False), m)
    mel = torch.from_numpy(batch_mel(1, Tm, first=5)).cuda()
    noise = torch.from_numpy(np.concatenate([batch_noise(1, T, first=900 + 10 * w) for w in range(2)], axis=1)[:, :L]).cuda()
    skw = dict(steps=N, spacing="logsnr", solver="dpmpp2m")
    out = tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T, **skw)
    assert tuple(out.shape) == (1, L, P) and torch.isfinite(out).all()
    xfp, xfo = m.encode_music(torch.stack([mel[0, 3 * s:3 * s + 3 * T] for s in (0, 192)]), "cuda")
    wins = []
    for w, s in enumerate((0, 192)):
        kw = {}
        if w:
            km = torch.zeros(1, T, device="cuda")
            km[:, :ov] = 1
            kw = dict(known=torch.cat([wins[0][:, T - ov:], torch.zeros(1, T - ov, P, device="cuda")], 1), known_mask=km,
                      known_noise=noise[:, s:s + T].contiguous())
        wins.append(tr.diffusion.ddim_sample_loop(m, (1, T, P), noise=noise[:, s:s + T].contiguous(), clip_denoised=False, progress=False,
                                                  model_kwargs={"xf_proj": xfp[w:w + 1].contiguous(), "xf_out": xfo[w:w + 1].contiguous(),
                                                                "length": torch.LongTensor([T])}, **skw, **kw))
    assert torch.equal(wins[1][:, :ov], wins[0][:, T - ov:])
    assert torch.equal(out[:, :192], wins[0][:, :192]) and torch.equal(out[:, 192:], wins[1])
    plain = tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T, steps=N, spacing="logsnr")
    assert not torch.equal(plain, out)


def test_errors(models):
    """8."""
    name = "layer16"
    d, m = _setup(name), models("fp16")
    B, T = d["B"], d["T"]
    gd, ts = _diffusion(), _list("logsnr")
    kw = dict(noise=d["x"].cuda(), clip_denoised=False, progress=False,
              model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda(), "length": torch.LongTensor(d["length"])})
    with pytest.raises(ValueError, match="eta must be 0"):
        gd.ddim_sample_loop(m, (B, T, P), steps=N, solver="dpmpp2m", eta=0.5, **kw)
    with pytest.raises(ValueError, match="denoised_fn"):
        gd.ddim_sample_loop(m, (B, T, P), steps=N, denoised_fn=lambda x: x, **kw)
    with pytest.raises(ValueError, match="strictly decreasing"):
        gd.ddim_sample_loop(m, (B, T, P), timesteps=[5, 7, 0], **kw)
    # the C ABI: max_timesteps is 1000 (helpers.make_model)
    nat = m.set_conditioning(kw["model_kwargs"]["xf_proj"], kw["model_kwargs"]["xf_out"], d["length"])
    nat.set_known(None, None, None)
    nat.set_smoothing(0, 0)
    x = d["x"].cuda()
    ac = np.cumprod(1.0 - get_named_beta_schedule("linear", 2000))
    long_ts = list(range(1000, -1, -1))                                          # 1001 entries, and t = 1000
    with pytest.raises(native.DcError, match="max_timesteps"):
        nat.solver_loop(x, long_ts, native.solver_table(ac, long_ts, 0.0, 1)[0])
    high = [1000, 500, 0]
    with pytest.raises(native.DcError, match="strictly decreasing inside"):
        nat.solver_loop(x, high, native.solver_table(ac, high, 0.0, 1)[0])
    rows = native.solver_table(gd.alphas_cumprod, ts, 0.0, 2)[0]
    rows[:, 4] = 0.1                                                             # sigma beside a history coefficient
    with pytest.raises(native.DcError, match="deterministic"):
        nat.solver_loop(x, ts, rows, step_noise=torch.zeros(len(ts), B, T, P, device="cuda"))
    out = _gpu(m, d, ts, "ddim")                                                 # the sampler is as it was
    assert torch.equal(out, _gpu(make_model("fp16"), d, ts, "ddim"))
