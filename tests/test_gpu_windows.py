"""Sampling a long piece's windows in one loop, blending the overlaps at every step (include/dc_ddim.h,
dc_sampler_set_conditioning_windows).  Needs an MI355X.

One shape per update site of the INTERNAL batch (W B windows x T; the forms are pinned on the CPU by tests/test_host_windows.py, FORMS)
against helpers_windows.ddim_windows_loop: the oracle's loop on one tensor in piece space, one forward call per window and step,
blended in fp32.  S = 25 steps, clip_denoised=False unless said.

Bounds, per piece (rel-L2): the project's gate 1e-3 with no extra factor - the blend is a convex combination of the windows'
outputs, so it cannot amplify a window's error; the guided row takes the guided tests' bound 1e-3 (|w| + |w - 1|)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import batch_mel, batch_noise, make_diffusion, make_model, oracle_params, rel_l2, xf_pair
from helpers_windows import SHAPES, ddim_windows_loop

from diffusion_conductor_amd import native
from diffusion_conductor_amd.harness import plan_windows, window_weights
from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule,
                                             spaced_timesteps)
from diffusion_conductor_amd.synthetic import batch_step_noise

pytestmark = pytest.mark.gpu
S = 25
P = 26


def tol(key, w=None):
    return 1e-3 if (key == "mixed" or w is None) else 1e-3 * (abs(w) + abs(w - 1))


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    made = {}

    def get(key):
        if key not in made:
            made[key] = make_model("fp16", no_eff=True) if key == "no_eff" else make_model(key)
        return made[key]
    return get


_inputs, _refs = {}, {}


def _make(B, T, L, starts, blend="tent"):
    W = len(starts)
    xfp, xfo = xf_pair(W * B, T, first=60)
    return dict(B=B, T=T, L=L, W=W, starts=list(starts), weights=window_weights(L, T, starts, blend), xfp=xfp, xfo=xfo,
                x=torch.from_numpy(batch_noise(B, L, first=60)), known=0.5 * torch.from_numpy(batch_noise(B, L, first=260)),
                eps=torch.from_numpy(batch_noise(B, L, first=460)))


def _setup(name):
    """Seeded inputs of a shape (host tensors), made once: features of the W B windows (window-major), piece-space noise."""
    if name not in _inputs:
        _, B, T, overlap, L, W, _ = SHAPES[name]
        starts = [s for s, _ in plan_windows(L, T, overlap)]
        assert len(starts) == W
        _inputs[name] = _make(B, T, L, starts)
    return _inputs[name]


def _clips(B):
    """The pieces a case compares with the checker's run of them alone (at most three, as tests/test_gpu_known.py picks them)."""
    return [2, 3, B - 1 if (B - 1) % 4 != 1 else B - 3] if B > 3 else list(range(B))


def _rows(d, pieces):
    """Rows of the window-major features that belong to `pieces`, window-major again."""
    return torch.tensor([k * d["B"] + b for k in range(d["W"]) for b in pieces])


def _gpu(model, d, w=None, gd=None, idxs=(), mask=None, **kw):
    gd = gd or make_diffusion(S)
    if mask is not None:
        kw.update(known=d["known"].cuda(), known_mask=mask.cuda(), known_noise=d["eps"].cuda())
    kw.setdefault("clip_denoised", False)
    out = gd.ddim_sample_loop(model, (d["B"], d["L"], P), noise=d["x"].cuda(), progress=False, idxs=list(idxs), guidance_scale=w,
                              model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda()}, window_starts=d["starts"],
                              window_weights=d["weights"], **kw)
    torch.cuda.synchronize()
    return out


def _plain(model, d, rows=None, idxs=(), **kw):
    """The plain loop on the windows as clips [W B, T, P], window k of piece b starting from its rows of the piece's noise."""
    B, T = d["B"], d["T"]
    x = torch.stack([d["x"][b, s:s + T] for s in d["starts"] for b in range(B)])
    xfp, xfo = d["xfp"], d["xfo"]
    if rows is not None:
        x, xfp, xfo = x[rows], xfp[rows], xfo[rows]
    out = make_diffusion(S).ddim_sample_loop(model, tuple(x.shape), noise=x.cuda(), progress=False, clip_denoised=False, idxs=list(idxs),
                                             model_kwargs={"xf_proj": xfp.cuda(), "xf_out": xfo.cuda(), "length": torch.LongTensor([T] * x.shape[0])},
                                             **kw)
    torch.cuda.synchronize()
    return out


def _sequential(model, d):
    """generate_long_music_motion's sequential path on the same features: window k sampled around the frames window k - 1 produced."""
    B, T, L = d["B"], d["T"], d["L"]
    gd, noise = make_diffusion(S), d["x"].cuda()
    out = torch.zeros(B, L, P, device="cuda")
    for k, s in enumerate(d["starts"]):
        kn = 0 if k == 0 else d["starts"][k - 1] + T - s
        x_T = noise[:, s:s + T].contiguous()
        mask = torch.zeros(B, T, device="cuda")
        mask[:, :kn] = 1
        out[:, s:s + T] = gd.ddim_sample_loop(model, (B, T, P), noise=x_T, clip_denoised=False, progress=False,
                                              model_kwargs={"xf_proj": d["xfp"][k * B:(k + 1) * B].cuda(), "xf_out": d["xfo"][k * B:(k + 1) * B].cuda(),
                                                            "length": torch.LongTensor([T] * B)},
                                              known=out[:, s:s + T].contiguous(), known_mask=mask, known_noise=x_T)
    return out.cpu()


def _overlap_frames(d):
    cover = np.zeros(d["L"], np.int64)
    for s in d["starts"]:
        cover[s:s + d["T"]] += 1
    return torch.from_numpy(cover > 1)


def _oracle(name, pieces, d=None, mask=None, tag="", **kw):
    """The checker's run of `pieces` of a shape alone, computed once per (shape, pieces, branch)."""
    key = (name, tuple(pieces), tag)
    if key not in _refs:
        d = d or _setup(name)
        c = torch.tensor(pieces)
        r = _rows(d, pieces)
        if "step_noise" in kw:
            kw["step_noise"] = kw["step_noise"][:, c]
        kn = dict(known=d["known"][c], mask=mask[c], eps=d["eps"][c]) if mask is not None else {}
        _refs[key] = ddim_windows_loop(oracle_params(), d["x"][c], d["xfp"][r], d["xfo"][r], d["starts"], d["weights"], S,
                                       no_eff=SHAPES.get(name, ("",))[0] == "no_eff", **kn, **kw)
    return _refs[key]


@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_against_the_checker(models, name):
    """1: per piece; the figures go to DESIGN.md section 4.10 and profiles/windows_gpu_tests.txt."""
    key, B, T, _, L, W, w = SHAPES[name]
    d, m = _setup(name), models(key)
    out = _gpu(m, d, w=w).cpu()
    assert tuple(out.shape) == (B, L, P) and torch.isfinite(out).all()
    pieces = _clips(B)
    ref = _oracle(name, pieces, w=w)
    errs = {c: rel_l2(out[c], ref[j]) for j, c in enumerate(pieces)}
    ov = _overlap_frames(d)
    seq = _sequential(m, d)
    moved = min(rel_l2(out[c][ov], seq[c][ov]) for c in pieces)
    worst = max(errs.values())
    print(f"windows parity {name}: worst {worst:.3e} (bound {tol(key, w):.1e})  " + " ".join(f"[{c}] {e:.2e}" for c, e in errs.items()) +
          f"  moved from the sequential windows by >= {moved:.2f} on the overlap frames")
    assert moved >= 0.1                                          # the blend did act on every compared piece
    assert worst <= tol(key, w), errs


@pytest.mark.parametrize("name", ["layer16", "wide_aligned"])
def test_disjoint_windows_are_independent_loops(models, name, monkeypatch):
    """2: overlap 0, L = W T: every weight is exactly 1 and the joint result, reshaped, is the plain loop on those clips - bit for bit
    in the same launch form (DC_NO_EMBED_NEXT=1 on the plain loop where it would embed the next step in its last layer), within the
    5e-4 tests/test_gpu_known.py allows between embed_next and a step's own front work otherwise."""
    key, B, T, _, _, W, _ = SHAPES[name]
    m = models(key)
    d = _make(B, T, W * T, [k * T for k in range(W)])
    assert (d["weights"] == 1).all()
    got = _gpu(m, d, idxs=(3,))
    as_clips = lambda t: t.view(B, W, T, P).transpose(0, 1).reshape(W * B, T, P)
    free = _plain(m, d, idxs=(3,))
    if name == "wide_aligned":
        monkeypatch.setenv("DC_NO_EMBED_NEXT", "1")
    same = _plain(m, d, idxs=(3,))
    monkeypatch.delenv("DC_NO_EMBED_NEXT", raising=False)
    for it in (3, S):
        assert torch.isfinite(got[it]).all() and torch.equal(as_clips(got[it]), same[it]), (name, it, rel_l2(as_clips(got[it]), same[it]))
        e = max(rel_l2(as_clips(got[it])[c], free[it][c]) for c in range(W * B))
        print(f"windows disjoint {name} iteration {it}: against the plain loop as it runs by default {e:.2e}")
        assert e <= 5e-4


@pytest.mark.parametrize("name", ["layer16", "wide_aligned"])
def test_one_window_is_the_plain_loop(models, name, monkeypatch):
    """3: W = 1, L = T, the same bit-for-bit conditions (wide_aligned: 160 pieces, the internal batch of the shape)."""
    key, B, T, _, _, W, _ = SHAPES[name]
    m = models(key)
    d = _make(B * W, T, T, [0])
    got = _gpu(m, d, idxs=(3,))
    free = _plain(m, d, idxs=(3,))
    if name == "wide_aligned":
        monkeypatch.setenv("DC_NO_EMBED_NEXT", "1")
    same = _plain(m, d, idxs=(3,))
    monkeypatch.delenv("DC_NO_EMBED_NEXT", raising=False)
    for it in (3, S):
        assert torch.equal(got[it], same[it]), (name, it, rel_l2(got[it], same[it]))
        assert max(rel_l2(got[it][c], free[it][c]) for c in range(B * W)) <= 5e-4


def test_a_piece_does_not_depend_on_its_batch(models):
    """4: piece 2 of the wide_aligned batch against the same piece sampled alone.  Alone its 4 windows run the small-batch form
    (16-token waves), in the batch the wide form: the plain loop is not bit-identical between the two forms either, so this asserts
    the 1e-3 gate; bit for bit it equals piece 2 of a batch of other pieces in the same form (clip-aligned units)."""
    name = "wide_aligned"
    key, B, T, _, L, W, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    full = _gpu(m, d)
    alone = dict(d, B=1, x=d["x"][2:3], xfp=d["xfp"][_rows(d, [2])], xfo=d["xfo"][_rows(d, [2])])
    e = rel_l2(_gpu(m, alone)[0], full[2])
    print(f"windows batch invariance: piece 2 alone (small-batch form) against the batch of {B}: {e:.2e}")
    assert e <= 1e-3
    other = dict(d, x=d["x"].clone(), xfp=d["xfp"].clone(), xfo=d["xfo"].clone())
    keep = _rows(d, [2])
    rest = torch.tensor([i for i in range(W * B) if i not in set(keep.tolist())])
    other["xfp"][rest] = d["xfp"][rest].flip(0)
    other["xfo"][rest] = d["xfo"][rest].flip(0)
    other["x"][torch.arange(B) != 2] = d["x"][torch.arange(B) != 2].flip(0)
    moved = _gpu(m, other)
    assert torch.equal(moved[2], full[2]) and not torch.equal(moved[3], full[3])


def _eps_diffusion():
    return GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=ModelMeanType.EPSILON,
                             model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)


@pytest.mark.parametrize("branch", ["eta", "clip", "eps", "dpmpp2m", "smooth", "snapshots", "known"])
def test_sampler_branches(models, branch):
    """5: the existing update behind the blend, 1 x (2 x 256), against the checker at the gate.  (The EPSILON case clips, as
    tests/test_gpu_known.py's does and for its reason: DESIGN.md section 4.6.)"""
    name = "layer16"
    key, B, T, _, L, W, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    mask, idxs, gd = None, (), None
    if branch == "eta":
        z = torch.from_numpy(batch_step_noise(S, B, L, first=60))
        assert tuple(z.shape) == (S, B, L, P)
        gkw, okw = dict(eta=0.5, step_noise=z.cuda()), dict(eta=0.5, step_noise=z)
    elif branch in ("clip", "eps"):
        gkw, okw = dict(clip_denoised=True), dict(clip_denoised=True, eps_model=branch == "eps")
        gd = _eps_diffusion() if branch == "eps" else None
    elif branch == "dpmpp2m":
        ts = spaced_timesteps(make_diffusion(S).alphas_cumprod, 10, "uniform")
        gkw, okw = dict(steps=10, solver="dpmpp2m"), dict(timesteps=ts, order=2)
    elif branch == "smooth":
        gkw, okw = dict(smooth=(11, 5)), {}
    elif branch == "snapshots":
        gkw, okw, idxs = {}, dict(idxs=(0, 3)), (0, 3)
    else:
        mask = torch.zeros(B, L, P)
        mask[:, 150:300] = 1                                     # the middle of the piece, across the seam at frames 192 .. 255
        mask[:, :, 5] = 1
        gkw, okw = {}, {}
    out = _gpu(m, d, gd=gd, mask=mask, idxs=idxs, **gkw)
    ref = _oracle(name, [0], mask=mask, tag=branch, **okw)
    if branch == "snapshots":
        errs = []
        for it in (0, 3, S):
            assert tuple(out[it].shape) == (B, L, P) and torch.isfinite(out[it]).all()
            errs.append(rel_l2(out[it][0], ref[it][0]))
        e = max(errs)
    elif branch == "known":
        out = out.cpu()
        k = mask != 0
        assert torch.equal(out[k], d["known"][k])                                 # bit for bit
        u = (mask[0] == 0)
        e = rel_l2(out[0][u], ref[0][u])
    elif branch == "smooth":
        unsmoothed = _gpu(m, d)
        assert torch.equal(out, native.savgol_filter(unsmoothed, 11, 5)) and not torch.equal(out, unsmoothed)
        e = rel_l2(unsmoothed[0], ref[0])
    else:
        assert torch.isfinite(out).all()
        e = rel_l2(out[0], ref[0])
    print(f"windows branch {branch}: {e:.3e} (bound {tol(key):.1e})")
    assert e <= tol(key)


def test_another_plan_reuses_the_graph(models):
    """6: starts and weights travel through device tables: another plan of the same (B, W, T, L) - one interior start shifted by 8 frames,
    uniform weights - matches the checker, a re-run of the first plan gives its bits again, and the second plan on a used sampler gives
    the bits of a fresh one (the sampler exposes no capture count to assert on)."""
    key, B, T, _, L, W, _ = SHAPES["narrow"]
    m = models(key)
    d = _setup("narrow")
    starts2 = list(d["starts"])
    starts2[1] += 8
    d2 = dict(d, starts=starts2, weights=window_weights(L, T, starts2, "uniform"))
    a = _gpu(m, d)
    b = _gpu(m, d2)
    a2 = _gpu(m, d)
    fresh = _gpu(make_model(key), d2)
    assert torch.equal(a, a2) and torch.equal(b, fresh) and not torch.equal(a, b)
    pieces = _clips(B)[:1]
    ref = _oracle("narrow/shifted", pieces, d=d2)
    e = rel_l2(b[pieces[0]], ref[0])
    print(f"windows second plan (start + 8, uniform): {e:.3e} (bound 1.0e-03)")
    assert e <= 1e-3


@pytest.mark.parametrize("name", ["layer16", "guided"])
def test_profile_loop_runs_windows(models, name):
    """dc_sampler_profile_loop on a windows conditioning: the eager, unfolded pass - one k_windows_update per step and no
    k_guided_update, guided or not - within the parity bound of the checker."""
    key, B, T, _, L, W, w = SHAPES[name]
    d, m = _setup(name), models(key)
    nat = m.set_conditioning(d["xfp"].cuda(), d["xfo"].cuda(), guided=w is not None, windows=(d["starts"], d["weights"], L))
    nat.set_known(None, None, None)
    nat.set_smoothing(0, 0)
    if w is not None:
        nat.set_guidance_scale(w)
    prof, out = nat.profile_loop(d["x"].cuda(), make_diffusion(S).native_coefficients())
    assert nat.status() == 0 and prof["k_windows_update"][1] == S and prof["k_guided_update"][1] == 0 and prof["k_film_gemm"][1] == S
    e = rel_l2(out[0], _oracle(name, [0], w=w)[0])
    print(f"windows profile loop {name}: {e:.3e} (bound {tol(key, w):.1e})")
    assert e <= tol(key, w)


def test_errors(models):
    """7: each refusal leaves the sampler usable."""
    d, m = _setup("layer16"), models("fp16")
    B, T, L = d["B"], d["T"], d["L"]
    gd = make_diffusion(S)
    kw = dict(noise=d["x"].cuda(), clip_denoised=False, progress=False, model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda()},
              window_starts=d["starts"], window_weights=d["weights"])
    want = _gpu(m, d)
    with pytest.raises(ValueError, match="takes"):
        gd.ddim_sample_loop(m, (B, L, P), takes=2, **dict(kw, noise=None))
    with pytest.raises(ValueError, match="progressive"):
        next(gd.ddim_sample_loop_progressive(m, (B, L, P), **kw))
    with pytest.raises(ValueError, match="denoised_fn|this call"):
        gd.ddim_sample_loop(m, (B, L, P), denoised_fn=lambda x: x, **kw)
    with pytest.raises(ValueError, match="come together"):
        gd.ddim_sample_loop(m, (B, L, P), **dict(kw, window_weights=None))
    with pytest.raises(ValueError, match="not 0|L - T"):
        gd.ddim_sample_loop(m, (B, L + 8, P), **dict(kw, noise=None))
    with pytest.raises(ValueError, match="full"):
        gd.ddim_sample_loop(m, (B, L, P), **dict(kw, model_kwargs=dict(kw["model_kwargs"], length=torch.LongTensor([T - 1] * 2 * B))))
    # a single evaluation, and the debug entry points, under a windows conditioning
    nat = m._ensure_native("cuda")
    assert nat.windows == (2, T)
    with pytest.raises(ValueError, match="windows"):
        nat.denoise(torch.zeros(2 * B, T, P, device="cuda"), [3] * (2 * B))
    import ctypes as C
    x = torch.zeros(2 * B, T, P, device="cuda")
    ts = np.full(2 * B, 3, np.int32)
    assert native.lib().dc_sampler_denoise(nat._h, x.data_ptr(), ts.ctypes.data_as(C.POINTER(C.c_int32)), x.data_ptr(), None) == -1
    assert "windows" in native.lib().dc_last_error().decode()
    with pytest.raises(native.DcError, match="windows"):
        nat.debug_layer(np.zeros((B, L, 128), np.float32), [3] * B, 0, 1, 1)
    # the harness: overlap beyond half a window, and sharded use
    from diffusion_conductor_amd import DDPMTrainer
    import diffusion_conductor_amd.harness as harness
    tr = DDPMTrainer(Namespace(device="cuda", diffusion_steps=S, is_train=False), m)
    mel = torch.from_numpy(batch_mel(1, 3 * 448, first=5))
    with pytest.raises(ValueError, match="overlap"):
        tr.generate_long_music_motion(mel, P, overlap=130, window=256, joint=True)
    with pytest.raises(ValueError, match="joint=True"):
        tr.generate_long_music_motion(mel, P, overlap=64, window=256, known=torch.zeros(1, 448, P), known_mask=torch.zeros(1, 448))
    dist_info = harness.dist_info
    harness.dist_info = lambda: (0, 2)
    try:
        with pytest.raises(NotImplementedError, match="shard"):
            tr.generate_long_music_motion(mel, P, overlap=64, window=256, joint=True)
    finally:
        harness.dist_info = dist_info
    assert torch.equal(_gpu(m, d), want)                         # the sampler is as it was


def test_generate_long_music_motion_joint():
    """8: one piece of 640 frames under three windows of 256, end to end on synthetic mel (fp16): shape, finite, the bits of the
    sampler-level call on the same features; joint=False on the same inputs returns the same bits twice and the concatenation
    property of the sequential path (a window's known frames are its predecessor's, bit for bit: tests/test_gpu_known.py)."""
    from diffusion_conductor_amd import DDPMTrainer
    m = make_model("fp16")
    tr = DDPMTrainer(Namespace(device="cuda", diffusion_steps=S, is_train=False), m)
    T, L, ov = 256, 640, 64
    mel = torch.from_numpy(batch_mel(1, 3 * L, first=5))
    noise = torch.from_numpy(batch_noise(1, L, first=900))
    out = tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T, joint=True)
    assert tuple(out.shape) == (1, L, P) and torch.isfinite(out).all()
    starts = [s for s, _ in plan_windows(L, T, ov)]
    assert starts == [0, 192, 384]
    melc = mel.cuda()
    mel_w = torch.stack([melc[:, 3 * s:3 * s + 3 * T] for s in starts]).reshape(3, 3 * T, 128)
    xfp, xfo = m.encode_music(mel_w, "cuda")
    direct = make_diffusion(S).ddim_sample_loop(m, (1, L, P), noise=noise.cuda(), clip_denoised=False, progress=False,
                                                model_kwargs={"xf_proj": xfp, "xf_out": xfo}, window_starts=starts,
                                                window_weights=window_weights(L, T, starts, "tent"))
    assert torch.equal(out, direct)
    uniform = tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T, joint=True, blend="uniform")
    assert torch.isfinite(uniform).all() and not torch.equal(uniform, out)
    # the default path is untouched: deterministic, and window k's run alone around window k - 1's frames reproduces its rows
    seq = tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T)
    assert torch.equal(seq, tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T, joint=False))
    s = starts[1]
    x_T = noise.cuda()[:, s:s + T].contiguous()
    mask = torch.zeros(1, T, device="cuda")
    mask[:, :ov] = 1
    again = make_diffusion(S).ddim_sample_loop(m, (1, T, P), noise=x_T, clip_denoised=False, progress=False,
                                               model_kwargs={"xf_proj": xfp[1:2], "xf_out": xfo[1:2], "length": torch.LongTensor([T])},
                                               known=seq[:, s:s + T].contiguous(), known_mask=mask, known_noise=x_T)
    assert torch.equal(again, seq[:, s:s + T]) and not torch.equal(seq, out)
    ovf = torch.zeros(L, dtype=torch.bool)
    ovf[192:256] = ovf[384:448] = True
    print(f"generate_long_music_motion joint against sequential on the overlap frames: {rel_l2(out[0][ovf].cpu(), seq[0][ovf].cpu()):.2f}")
