"""Classifier-free guidance inside the captured DDIM loop (include/dc_ddim.h, dc_sampler_set_conditioning_guided).
Needs an MI355X.

One caller shape per update site of the INTERNAL batch (2 B clips; the forms are pinned on the CPU by tests/test_host_guided.py, FORMS)
against helpers_guided.ddim_guided_loop: the oracle's loop with two forward calls per step combined as c + (w - 1)(c - u).  S = 25
steps (the linear schedule needs S > 20), w = 2 unless said.

Bounds, per clip of >= 100 frames (rel-L2): `mixed` the project's gate 1e-3; fp16 / bf16 1e-3 (|w| + |w - 1|) - the per-loop bound times
the first-order amplification of the combination when each branch's error is at the bound - 3e-3 at w = 2.  The two ragged fp16 batches
whose clips are all shorter (2 x 96: 166 valid frames) take the same bound over the whole batch; 3 x 20 (34 valid frames) is printed
only."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import O, batch_mel, batch_noise, make_diffusion, make_model, oracle_params, rel_l2, xf_pair
from helpers_guided import ddim_guided_loop, null_pair
from helpers_known import prefix_mask, unknown_rel_l2

from diffusion_conductor_amd import native
from diffusion_conductor_amd.synthetic import batch_step_noise

pytestmark = pytest.mark.gpu
S = 25
P = 26
W = 2.0

# name -> (model key, the caller's B, T, lengths or None); the internal form each runs: tests/test_host_guided.py
SHAPES = {"layer16": ("fp16", 1, 256, None),
          "narrow": ("fp16", 36, 256, None),
          "wide_aligned": ("fp16", 80, 256, None),
          "wide_flat": ("fp16", 55, 300, None),
          "group_96": ("fp16", 2, 96, [96, 70]),
          "group_20": ("fp16", 3, 20, [20, 1, 13]),
          "no_eff": ("no_eff", 2, 96, [96, 70]),
          "bf16": ("bf16", 1, 256, None),
          "mixed": ("mixed", 1, 256, None),
          "padded_300": ("fp16", 1, 300, None),          # clip stride padded to 320: the padding lanes of the shadow groups read the null column
          "odd_255": ("fp16", 1, 255, None)}             # 6630 elements, no multiple of 4: k_guided_update's scalar path and its short tail
# 55 x 300 = 16500 and 1 x 255 tokens per half: no whole number of groups, the full GEMM
SHARED = [n for n in SHAPES if n not in ("wide_flat", "odd_255")]


def tol(key, w=W):
    return 1e-3 if key == "mixed" else 1e-3 * (abs(w) + abs(w - 1))


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


def _setup(name):
    """Seeded inputs of a shape (host tensors), made once."""
    if name not in _inputs:
        _, B, T, length = SHAPES[name]
        xfp, xfo = xf_pair(B, T, first=60)
        _inputs[name] = dict(B=B, T=T, length=length or [T] * B, xfp=xfp, xfo=xfo, x=torch.from_numpy(batch_noise(B, T, first=60)),
                             known=0.5 * torch.from_numpy(batch_noise(B, T, first=260)), eps=torch.from_numpy(batch_noise(B, T, first=460)))
    return _inputs[name]


def _clips(B):
    """The clips a case compares with the checker's run of them alone (at most three, as tests/test_gpu_known.py picks them)."""
    return [2, 3, B - 1 if (B - 1) % 4 != 1 else B - 3] if B > 3 else list(range(B))


def _gpu(model, d, w=W, gd=None, idxs=(), mask=None, **kw):
    gd = gd or make_diffusion(S)
    if mask is not None:
        kw.update(known=d["known"].cuda(), known_mask=mask.cuda(), known_noise=d["eps"].cuda())
    kw.setdefault("clip_denoised", False)
    out = gd.ddim_sample_loop(model, (d["B"], d["T"], P), noise=d["x"].cuda(), progress=False, idxs=list(idxs), guidance_scale=w,
                              model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda(), "length": torch.LongTensor(d["length"])}, **kw)
    torch.cuda.synchronize()
    return out


def _oracle(name, clips, w=W, mask=None, tag="", **kw):
    """The checker's run of `clips` of a shape alone, computed once per (shape, clips, w, branch)."""
    key = (name, tuple(clips), w, tag)
    if key not in _refs:
        d = _setup(name)
        c = torch.tensor(clips)
        if "step_noise" in kw:
            kw["step_noise"] = kw["step_noise"][:, c]
        kn = dict(known=d["known"][c], mask=mask[c], eps=d["eps"][c]) if mask is not None else {}
        _refs[key] = ddim_guided_loop(oracle_params(), d["x"][c], d["xfp"][c], d["xfo"][c], [d["length"][i] for i in clips], S, w,
                                      no_eff=SHAPES[name][0] == "no_eff", **kn, **kw)
    return _refs[key]


def _raw_loop(model, d, w, null, flags=0):
    """A guided loop through the sampler object itself, with the null pair given (the Python surface always passes null_conditioning())."""
    nat = model._ensure_native("cuda")
    model._cond_key = None                    # (the module's cache of its last conditioning no longer describes the sampler)
    nat.set_conditioning(d["xfp"].cuda().contiguous(), d["xfo"].cuda().contiguous(), d["length"], null=null)
    nat.set_smoothing(0, 0)
    nat.set_known(None, None, None)
    nat.set_guidance_scale(w)
    out, snaps = nat.ddim_loop(d["x"].cuda(), make_diffusion(S).native_coefficients(), [3])
    assert nat.status() == 0
    return out, snaps


@pytest.mark.parametrize("name", list(SHAPES))
def test_parity_against_the_checker(models, name):
    """1: per clip, clips of >= 100 frames; the figures go to DESIGN.md section 4.7 and profiles/guided_gpu_tests.txt."""
    key, B, T, _ = SHAPES[name]
    d = _setup(name)
    out = _gpu(models(key), d).cpu()
    assert torch.isfinite(out).all()
    clips = _clips(B)
    ref = _oracle(name, clips)
    plain = make_diffusion(S).ddim_sample_loop(models(key), (B, T, P), noise=d["x"].cuda(), progress=False, clip_denoised=False,
                                               model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda(),
                                                             "length": torch.LongTensor(d["length"])}).cpu()
    if T >= 100:
        errs = {c: rel_l2(out[c], ref[j]) for j, c in enumerate(clips)}
        moved = min(rel_l2(out[c], plain[c]) for c in clips)
    else:       # clips shorter than 100 frames (clips == all of them): the valid frames of the whole batch as one figure
        valid = prefix_mask(B, T, P, d["length"]) != 0
        errs = {"batch": rel_l2(out[valid], ref[valid])}
        moved = rel_l2(out[valid], plain[valid])
    worst = max(errs.values())
    print(f"guided parity {name} w={W}: worst {worst:.3e} (bound {tol(key):.1e})  " + " ".join(f"[{c}] {e:.2e}" for c, e in errs.items()) +
          f"  moved from the unguided loop by >= {moved:.2f}")
    assert moved >= 0.1                                        # guidance did act on every compared clip
    if name != "group_20":                                     # (34 valid frames: printed only)
        assert worst <= tol(key), errs


@pytest.mark.parametrize("name", SHARED)
def test_shared_column_is_the_full_gemm_bit_for_bit(models, name, monkeypatch):
    """2: the unconditional half reading ONE FiLM column against DC_GUIDE_FULL_FILM=1, the GEMM over all 2 B clips' groups."""
    key, B, T, _ = SHAPES[name]
    d = _setup(name)
    iters = (0, S // 2)
    shared = _gpu(models(key), d, idxs=iters)
    monkeypatch.setenv("DC_GUIDE_FULL_FILM", "1")
    full = _gpu(models(key), d, idxs=iters)
    monkeypatch.delenv("DC_GUIDE_FULL_FILM")
    for it in iters + (S,):
        assert torch.isfinite(shared[it]).all() and torch.equal(shared[it], full[it]), (name, it, rel_l2(shared[it], full[it]))


@pytest.mark.parametrize("name", ["layer16", "wide_aligned"])
def test_scale_one_ignores_the_unconditional_branch(models, name):
    """3: out = c + (w - 1)(c - u) returns c bit for bit at w = 1 whenever u is finite: two null pairs, the same bits."""
    key, B, T, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    a, sa = _raw_loop(m, d, 1.0, m.null_conditioning())
    rnd = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 64)).astype(np.float32))
    b, sb = _raw_loop(m, d, 1.0, (rnd[0], rnd[1]))
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(sa, sb)
    c, _ = _raw_loop(m, d, W, (rnd[0], rnd[1]))               # (the other null pair does reach the kernels)
    e, _ = _raw_loop(m, d, W, m.null_conditioning())
    assert not torch.equal(c, e) and not torch.equal(e, a)
    m._cond_key = None


def test_another_scale_reuses_the_graph(models):
    """4: scales travel through a device slot; a re-run gives the same bits, and a scale first seen on a used sampler gives the bits of a
    fresh one (the sampler exposes no capture count to assert on)."""
    d, m = _setup("layer16"), models("fp16")
    a = _gpu(m, d, w=2.0, idxs=(3,))
    b = _gpu(m, d, w=3.0, idxs=(3,))
    a2 = _gpu(m, d, w=2.0, idxs=(3,))
    want = _gpu(make_model("fp16"), d, w=3.0, idxs=(3,))
    for it in (3, S):
        assert torch.equal(a[it], a2[it]) and torch.equal(b[it], want[it]) and not torch.equal(a[it], b[it])
    ref = _oracle("layer16", [0], w=3.0)
    e = rel_l2(b[S][0], ref[0])
    print(f"guided parity layer16 w=3: {e:.3e} (bound {tol('fp16', 3.0):.1e})")
    assert e <= tol("fp16", 3.0)


def _eps_diffusion():
    from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule)
    return GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=ModelMeanType.EPSILON,
                             model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)


@pytest.mark.parametrize("branch", ["eta", "clip", "eps", "known", "smooth"])
def test_sampler_branches(models, branch):
    """5: the existing update behind the combination, 1 x 256 against the checker with the same gates.  (The EPSILON case clips, as
    tests/test_gpu_known.py's does and for its reason: DESIGN.md section 4.6.)"""
    name = "layer16"
    key, B, T, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    mask = None
    if branch == "eta":
        z = torch.from_numpy(batch_step_noise(S, B, T, first=60))
        gkw, okw = dict(eta=0.5, step_noise=z.cuda()), dict(eta=0.5, step_noise=z)
    elif branch in ("clip", "eps"):
        gkw, okw = dict(clip_denoised=True), dict(clip_denoised=True, eps_model=branch == "eps")
    elif branch == "known":
        mask = prefix_mask(B, T, P, [100])
        mask[:, :, 5] = 1
        gkw, okw = {}, {}
    else:
        gkw, okw = dict(smooth=(19, 5)), {}
    out = _gpu(m, d, gd=_eps_diffusion() if branch == "eps" else None, mask=mask, **gkw).cpu()
    ref = _oracle(name, [0], mask=mask, tag=branch, **okw)
    assert torch.isfinite(out).all()
    if branch == "known":
        k = mask != 0
        assert torch.equal(out[k], d["known"][k])                                 # bit for bit
        e = unknown_rel_l2(out[0], ref[0], mask[0])
    elif branch == "smooth":
        unsmoothed = _gpu(m, d)
        assert torch.equal(out, native.savgol_filter(unsmoothed, 19, 5).cpu()) and not torch.equal(out, unsmoothed.cpu())
        e = rel_l2(unsmoothed[0], ref[0])
    else:
        e = rel_l2(out[0], ref[0])
    print(f"guided branch {branch} w={W}: {e:.3e} (bound {tol(key):.1e})")
    assert e <= tol(key)


@pytest.mark.parametrize("name", ["layer16", "wide_aligned", "group_96", "no_eff"])
def test_guidance_off_means_off(models, name):
    """6: after a guided loop, a plain conditioning and loop gives the bits of a fresh sampler's loop; guidance_scale=None never
    touches the guided entry points."""
    key, B, T, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    fresh = make_model("fp16", no_eff=True) if key == "no_eff" else make_model(key)
    want = _gpu(fresh, d, w=None, idxs=(3,))
    guided = _gpu(m, d, idxs=(3,))
    after = _gpu(m, d, w=None, idxs=(3,))
    for it in (3, S):
        assert torch.equal(after[it], want[it]) and not torch.equal(guided[it], want[it])
    assert m._native.guided is False and fresh._native.guided is False


def test_errors(models):
    """7."""
    d, m = _setup("layer16"), models("fp16")
    B, T = d["B"], d["T"]
    xfp, xfo = d["xfp"].cuda(), d["xfo"].cuda()
    nat = m._ensure_native("cuda")
    m._cond_key = None
    npj, nout = m.null_conditioning()
    with pytest.raises(native.DcError, match="null pair"):
        nat.set_conditioning(xfp, xfo, d["length"], null=(None, nout))
    with pytest.raises(native.DcError, match="null pair"):
        nat.set_conditioning(xfp, xfo, d["length"], null=(npj, None))
    nat.set_conditioning(xfp, xfo, d["length"])
    with pytest.raises(native.DcError, match="guided"):
        nat.set_guidance_scale(2.0)                                               # no guided conditioning to scale
    nat.set_conditioning(xfp, xfo, d["length"], null=(npj, nout))
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(native.DcError, match="finite"):
            nat.set_guidance_scale(bad)
    with pytest.raises(native.DcError, match="guided"):
        nat.denoise(d["x"].cuda(), [3] * B)
    with pytest.raises(native.DcError, match="guided"):
        nat.debug_denoise(d["x"].cuda(), [3] * B, 8, 0)
    with pytest.raises(native.DcError, match="guided"):
        nat.debug_layer(np.zeros((B, T, 128), np.float32), [3] * B, 0, 1, 1)
    m._cond_key = None
    kw = dict(noise=d["x"].cuda(), clip_denoised=False, progress=False,
              model_kwargs={"xf_proj": xfp, "xf_out": xfo, "length": torch.LongTensor(d["length"])})
    from diffusion_conductor_amd.sampler import GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule
    gd = make_diffusion(S)
    with pytest.raises(ValueError, match="denoised_fn"):
        gd.ddim_sample_loop(m, (B, T, P), guidance_scale=2.0, denoised_fn=lambda x: x, **kw)
    with pytest.raises(ValueError, match="cond_fn"):
        gd.ddim_sample_loop(m, (B, T, P), guidance_scale=2.0, cond_fn=lambda x, t, **k: x, **kw)
    with pytest.raises(ValueError, match="finite"):
        gd.ddim_sample_loop(m, (B, T, P), guidance_scale=float("nan"), **kw)
    with pytest.raises(ValueError, match="progressive"):
        next(gd.ddim_sample_loop_progressive(m, (B, T, P), guidance_scale=2.0, **kw))
    for mean, var, what in ((ModelMeanType.PREVIOUS_X, ModelVarType.FIXED_SMALL, "PREVIOUS_X"),
                            (ModelMeanType.START_X, ModelVarType.LEARNED_RANGE, "learned-variance")):
        g2 = GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=mean, model_var_type=var, loss_type=LossType.MSE)
        with pytest.raises(ValueError, match=what):
            g2.ddim_sample_loop(m, (B, T, P), guidance_scale=2.0, **kw)
    out = gd.ddim_sample_loop(m, (B, T, P), **kw)                                 # the sampler is as it was
    assert torch.equal(out, _gpu(make_model("fp16"), d, w=None))


def test_generate_music_motion_guided():
    """8: DDPMTrainer.generate_music_motion(mel, guidance_scale=2) for 2 clips of 256 frames against the checker fed by the oracle's
    encode_music: `mixed`, 1e-3."""
    from diffusion_conductor_amd import DDPMTrainer
    m = make_model("mixed")
    tr = DDPMTrainer(Namespace(device="cuda", diffusion_steps=S, is_train=False), m)
    mel = torch.from_numpy(batch_mel(2, 768, first=5))
    noise = torch.from_numpy(batch_noise(2, 256, first=900))
    out = tr.generate_music_motion(mel, P, noise=noise, guidance_scale=W).cpu()
    plain = tr.generate_music_motion(mel, P, noise=noise).cpu()
    p = oracle_params()
    with torch.no_grad():
        xfp, xfo = O.encode_music(p, mel)
    assert tuple(xfo.shape) == (2, 256, 64)
    ref = ddim_guided_loop(p, noise, xfp, xfo, [256, 256], S, W, null=null_pair(p))
    errs = [rel_l2(out[b], ref[b]) for b in range(2)]
    print(f"generate_music_motion guided w={W} (mixed): {errs[0]:.3e} {errs[1]:.3e}; moved by {rel_l2(out, plain):.2f}")
    assert max(errs) <= 1e-3 and rel_l2(out, plain) >= 0.1


def test_known_values_belong_to_the_callers_geometry():
    """Known tensors are [B, T, P] of the CALLER's clips while a guided sampler's internal batch is 2 B: guided(1) with known values
    set, then a plain conditioning of 2 clips (as many as the guided internal batch) must drop them - they hold one clip -, and
    plain(2) with known values, then guided(1), likewise.  All-ones masks: a loop that kept them would return `known`."""
    T = 256
    xfp, xfo = (t.cuda() for t in xf_pair(2, T, first=60))
    x = torch.from_numpy(batch_noise(2, T, first=60)).cuda()
    known = 0.5 * torch.from_numpy(batch_noise(2, T, first=260)).cuda()
    ones = torch.ones(2, T, P, device="cuda")
    coef = make_diffusion(S).native_coefficients_known(0.0)

    def guided1(nat, with_known):
        nat.set_conditioning(xfp[:1].contiguous(), xfo[:1].contiguous(), [T], null=null)
        nat.set_guidance_scale(W)
        if with_known:
            nat.set_known(known[:1].contiguous(), ones[:1].contiguous(), x[:1].contiguous())
        out, _ = nat.ddim_loop(x[:1].contiguous(), coef)
        assert nat.status() == 0
        return out

    def plain2(nat, with_known):
        nat.set_conditioning(xfp, xfo, [T, T])
        if with_known:
            nat.set_known(known, ones, x)
        out, _ = nat.ddim_loop(x, coef)
        assert nat.status() == 0
        return out

    fresh, used = make_model("fp16"), make_model("fp16")
    null = fresh.null_conditioning()
    want_p, want_g = plain2(fresh._ensure_native("cuda"), False), guided1(fresh._ensure_native("cuda"), False)
    nat = used._ensure_native("cuda")
    kept = guided1(nat, True)
    assert torch.equal(kept, known[:1])                                          # (set on this conditioning, they do act)
    assert torch.equal(plain2(nat, False), want_p)                               # guided(1) -> plain(2): dropped
    assert torch.equal(plain2(nat, True), known)
    assert torch.equal(guided1(nat, False), want_g)                              # plain(2) -> guided(1): dropped
    nat.set_conditioning(xfp[:1].contiguous(), xfo[:1].contiguous(), [T])        # guided(1) -> plain(1): the same caller geometry,
    nat.set_known(known[:1].contiguous(), ones[:1].contiguous(), x[:1].contiguous())      # another conditioning
    assert torch.equal(guided1(nat, False), want_g)


def test_seeded_step_noise_is_sized_for_the_callers_clips(models):
    """eta > 0 with the library's own draws (one [B, T, P] buffer refilled per step, the CALLER's B): the bits of the same loop fed
    the draws as an explicit [S, B, T, P] tensor."""
    name = "narrow"
    key, B, T, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    seeded = _gpu(m, d, eta=0.5, step_noise_seed=7, idxs=(3,))
    z = torch.stack([native.step_noise((B, T, P), 7, it, "cuda") for it in range(S)])
    explicit = _gpu(m, d, eta=0.5, step_noise=z, idxs=(3,))
    for it in (3, S):
        assert torch.isfinite(seeded[it]).all() and torch.equal(seeded[it], explicit[it])
    assert not torch.equal(seeded[S], _gpu(m, d))


def test_profile_loop_runs_guided(models):
    """dc_sampler_profile_loop on a guided conditioning: the eager, unfolded pass - one k_guided_update and one FiLM launch per step,
    the embedding in its own launch - within the parity bound of the checker."""
    name = "layer16"
    key, B, T, _ = SHAPES[name]
    d, m = _setup(name), models(key)
    nat = m.set_conditioning(d["xfp"].cuda(), d["xfo"].cuda(), d["length"], guided=True)
    nat.set_known(None, None, None)
    nat.set_smoothing(0, 0)
    nat.set_guidance_scale(W)
    prof, out = nat.profile_loop(d["x"].cuda(), make_diffusion(S).native_coefficients())
    assert nat.status() == 0 and prof["k_guided_update"][1] == S and prof["k_film_gemm"][1] == S and prof["k_embed_front"][1] == S
    e = rel_l2(out[0], _oracle(name, [0])[0])
    print(f"guided profile loop {name} w={W}: {e:.3e} (bound {tol(key):.1e})")
    assert e <= tol(key)
