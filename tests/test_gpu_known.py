"""Sampling around known values on the GPU (include/dc_ddim.h, dc_sampler_set_known).  Needs an MI355X.

One shape per site of the DDIM update (the forms are pinned on the CPU by tests/test_host_known.py, FORMS), three masks per shape,
against helpers_known.ddim_known_loop: the oracle's loop plus the replacement rule in fp32.  S = 25 steps: the linear schedule needs
S > 20 (beta_end = 20 / S), 25 is what the other loop tests of short clips run.

Bounds: the project's per-clip gate 1e-3 (rel-L2, here over a clip's UNKNOWN elements); known elements of the final sample bitwise;
known elements of a snapshot within 2^-22 (|c2 known| + |c5 eps|) of the fp32 value (a fused against an unfused multiply-add)."""
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import O, batch_mel, batch_noise, make_diffusion, make_model, oracle_params, rel_l2, xf_pair
from helpers_known import ddim_known_loop, prefix_mask, unknown_rel_l2
from helpers_solver import solver_loop

from diffusion_conductor_amd import native
from diffusion_conductor_amd.synthetic import batch_step_noise

pytestmark = pytest.mark.gpu
TOL = 1e-3
S = 25
P = 26

# name -> (model key, B, T, lengths or None); the form each runs: tests/test_host_known.py
SHAPES = {"layer16": ("fp16", 2, 256, None),
          "narrow": ("fp16", 72, 256, None),
          "wide_embed_next": ("fp16", 160, 256, None),
          "wide_flat": ("fp16", 110, 300, None),
          "group_96": ("fp16", 2, 96, [96, 70]),
          "group_20": ("fp16", 3, 20, [20, 1, 13]),
          "no_eff": ("no_eff", 2, 96, [96, 70]),
          "bf16": ("bf16", 2, 256, None)}
PARITY = ("layer16", "narrow", "wide_embed_next", "wide_flat", "bf16")        # clips with >= 100 unknown frames; the others: properties only
MASKS = ("prefix", "edges", "channels")


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    made = {}

    def get(key):
        if key not in made:
            made[key] = make_model("fp16", no_eff=True) if key == "no_eff" else make_model(key)
        return made[key]
    return get


def _mask(kind, B, T):
    if kind == "prefix":          # another length per clip: 0 for one, T for one
        lens = [(0, T, min(T - 1, 37 + (b % 50)), T // 2 + 22)[b % 4] for b in range(B)]
        return prefix_mask(B, T, P, lens)
    m = torch.zeros(B, T, P)
    if kind == "edges":           # in-betweening: first and last frames known
        e = min(16, T // 3)
        m[:, :e] = 1
        m[:, T - e:] = 1
    else:                         # joint constraints: two pose channels on all frames
        m[:, :, 3] = 1
        m[:, :, 17] = 1
    return m


_inputs = {}


def _setup(name):
    """Seeded inputs of a shape (host tensors), made once: x_T, features, lengths, known values and their fixed draw."""
    if name not in _inputs:
        _, B, T, length = SHAPES[name]
        xfp, xfo = xf_pair(B, T, first=60)
        _inputs[name] = dict(B=B, T=T, length=length or [T] * B, xfp=xfp, xfo=xfo, x=torch.from_numpy(batch_noise(B, T, first=60)),
                             known=0.5 * torch.from_numpy(batch_noise(B, T, first=260)), eps=torch.from_numpy(batch_noise(B, T, first=460)))
    return _inputs[name]


def _clips(B):
    """The clips a case compares with the checker's run of them alone (at most three; of _mask's "prefix" lengths: a short prefix,
    a long one, and the last clip of the batch unless that one is all known)."""
    return [2, 3, B - 1 if (B - 1) % 4 != 1 else B - 3] if B > 3 else list(range(B))


def _gpu(model, d, gd=None, idxs=(), mask=None, known=None, eps=None, **kw):
    gd = gd or make_diffusion(S)
    if mask is not None:
        kw.update(known=(d["known"] if known is None else known).cuda(), known_mask=mask.cuda(), known_noise=(d["eps"] if eps is None else eps).cuda())
    kw.setdefault("clip_denoised", False)
    out = gd.ddim_sample_loop(model, (d["B"], d["T"], P), noise=d["x"].cuda(), progress=False, idxs=list(idxs),
                              model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda(), "length": torch.LongTensor(d["length"])}, **kw)
    torch.cuda.synchronize()
    return out


def _oracle(d, clips, mask, no_eff=False, **kw):
    c = torch.tensor(clips)
    sub = lambda t: t[c]
    if "step_noise" in kw:
        kw["step_noise"] = kw["step_noise"][:, c]
    return ddim_known_loop(oracle_params(), sub(d["x"]), sub(d["xfp"]), sub(d["xfo"]), [d["length"][i] for i in clips], S,
                           known=sub(d["known"]), mask=sub(mask), eps=sub(d["eps"]), no_eff=no_eff, **kw)


def _check_snapshots(res, d, mask, iters, eta=0.0):
    """Known elements of the snapshot of iteration `it` (timestep S - 1 - it): c2 known + c5 eps in fp32, to a fused multiply-add."""
    ck, _ = native.ddim_coefficients_known(make_diffusion(S).alphas_cumprod, eta)
    k = (mask != 0).numpy()
    for it in iters:
        c2, c5 = ck[S - 1 - it, 2], ck[S - 1 - it, 5]
        a, b = c2 * d["known"].numpy(), c5 * d["eps"].numpy()              # fp32
        got = res[it].cpu().numpy().astype(np.float64)
        bound = 2.0 ** -22 * (np.abs(a).astype(np.float64) + np.abs(b))
        assert np.all(np.abs(got - (a + b).astype(np.float64))[k] <= bound[k]), (it, float(np.abs(got - (a + b))[k].max()))


def _check_parity(tag, out, ref, clips, mask, need_frames=100):
    errs = {}
    for j, c in enumerate(clips):
        if int((mask[c] == 0).any(dim=1).sum()) >= need_frames:
            errs[c] = unknown_rel_l2(out[c], ref[j], mask[c])
    assert errs, "no compared clip keeps 100 unknown frames"
    print(f"known parity {tag}: worst clip {max(errs.values()):.3e}  " + " ".join(f"[{c}] {e:.2e}" for c, e in errs.items()))
    assert max(errs.values()) <= TOL, errs


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_known_values_per_update_site(models, name, kind):
    """Checks 1, 3, 4: the final sample equals `known` bitwise on the known elements; snapshots of the first, a middle and the last
    iteration hold the replaced values; the unknown elements of the compared clips meet the per-clip gate against the checker's run
    of those clips (the replaced inputs differ from unreplaced ones by O(1): a site that skipped the replacement fails here).  Every
    fp16 / bf16 loop's last evaluation is a split one (the precise tail)."""
    key, B, T, _ = SHAPES[name]
    d = _setup(name)
    mask = _mask(kind, B, T)
    iters = (0, S // 2, S - 1)
    res = _gpu(models(key), d, idxs=iters, mask=mask)
    out = res[S].cpu()
    k = mask != 0
    assert torch.isfinite(out).all()
    assert torch.equal(out[k], d["known"][k])                                   # 1: exact
    assert torch.equal(res[S - 1].cpu(), out)                                   # (the last iteration's snapshot is the final sample)
    _check_snapshots(res, d, mask, iters)                                       # 3
    if name in PARITY:                                                          # 4
        clips = _clips(B)
        _check_parity(f"{name}/{kind}", out, _oracle(d, clips, mask), clips, mask)


@pytest.mark.parametrize("name", list(SHAPES))
def test_off_means_off(models, name):
    """Check 2: an all-zero mask gives the bits of the loop without known values; after a loop with known values, a loop without them
    (the setting cleared) gives the bits a fresh sampler gives."""
    key, B, T, _ = SHAPES[name]
    d = _setup(name)
    m = models(key)
    fresh = make_model("fp16", no_eff=True) if key == "no_eff" else make_model(key)
    want = _gpu(fresh, d, idxs=(3,))
    zero = _gpu(m, d, idxs=(3,), mask=torch.zeros(B, T, P))
    with_known = _gpu(m, d, idxs=(3,), mask=_mask("edges", B, T))
    cleared = _gpu(m, d, idxs=(3,))
    for it in (3, S):
        assert torch.equal(zero[it], want[it]) and torch.equal(cleared[it], want[it])
        assert not torch.equal(with_known[it], want[it])
    assert m._native._known is None


def test_embed_next_ordering(models, monkeypatch):
    """Check 5: in the wide form the last layer embeds x_{t-1} from registers for the next step (DC_UPD_EMBED_NEXT): the replacement
    has to be in those registers, not only in the stored tensor.  With the front work in every step's own launch (DC_NO_EMBED_NEXT=1)
    and without: known elements of every snapshot bitwise equal, results within what the two forms differ by today (5e-4,
    test_last_layer_does_the_next_steps_front_work)."""
    d = _setup("wide_embed_next")
    mask = _mask("prefix", d["B"], d["T"])
    k = mask != 0
    iters = (0, 7, S // 2, S - 1)
    m = models("fp16")
    fused = _gpu(m, d, idxs=iters, mask=mask)
    monkeypatch.setenv("DC_NO_EMBED_NEXT", "1")
    own = _gpu(m, d, idxs=iters, mask=mask)
    monkeypatch.delenv("DC_NO_EMBED_NEXT")
    for it in iters + (S,):
        assert torch.equal(fused[it].cpu()[k], own[it].cpu()[k]), it
        e = rel_l2(fused[it], own[it])
        print(f"known, embed_next vs own front work, iteration {it}: {e:.2e}")
        assert e <= 5e-4, (it, e)
    assert not torch.equal(fused[S], own[S])                                    # (the switch does switch)


def _eps_diffusion():
    from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule)
    return GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=ModelMeanType.EPSILON,
                             model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)


def _check_branch(models, name, branch):
    """A sampler branch around known values on one shape: the known elements stay exact, the middle snapshot holds the replaced
    values, and - shapes of PARITY - the unknown elements meet the gate against the checker (dpmpp2m: helpers_solver's, on the list of
    every timestep)."""
    key, B, T, _ = SHAPES[name]
    d = _setup(name)
    mask = prefix_mask(B, T, P, [min(T, (100, 37, 0, 150)[b % 4]) for b in range(B)])
    mask[:, :, 5] = 1
    z = torch.from_numpy(batch_step_noise(S, B, T, first=60)) if branch == "eta" else None
    # (the EPSILON case clips, as test_gpu_robust's does: read as an epsilon model the seeded checkpoint grows x_t to 1.2e5 over 25
    # unclipped steps - the checker's own fp32 run - which no 16-bit operand holds)
    gkw = dict(eta=0.5, step_noise=z.cuda()) if branch == "eta" else dict(solver="dpmpp2m") if branch == "dpmpp2m" else dict(clip_denoised=True)
    okw = dict(eta=0.5, step_noise=z) if branch == "eta" else {} if branch == "dpmpp2m" else dict(clip_denoised=True, eps_model=branch == "eps")
    res = _gpu(models(key), d, gd=_eps_diffusion() if branch == "eps" else None, idxs=(S // 2,), mask=mask, **gkw)
    out = res[S].cpu()
    k = mask != 0
    assert torch.isfinite(out).all() and torch.equal(out[k], d["known"][k])
    _check_snapshots(res, d, mask, (S // 2,), eta=0.5 if branch == "eta" else 0.0)
    if name not in PARITY:
        return
    clips = _clips(B)
    if branch == "dpmpp2m":
        c = torch.tensor(clips)
        ref = solver_loop(oracle_params(), d["x"][c], d["xfp"][c], d["xfo"][c], [d["length"][i] for i in clips], S, list(range(S - 1, -1, -1)),
                          order=2, known=d["known"][c], mask=mask[c], eps=d["eps"][c])
    else:
        ref = _oracle(d, clips, mask, **okw)
    _check_parity(f"{name}/{branch}", out, ref, clips, mask)


@pytest.mark.parametrize("name,branch", [("layer16", "eta"), ("layer16", "clip"), ("layer16", "eps"), ("wide_embed_next", "eta")])
def test_sampler_branches_act_on_unknown_elements_only(models, name, branch):
    """Check 6: eta > 0 with explicit step noise, clip_denoised, an EPSILON model - the known elements stay exact, the unknown ones
    meet the gate."""
    _check_branch(models, name, branch)


# (an EPSILON model on full attention at eta = 0 is refused by the library: no such case)
@pytest.mark.parametrize("name,branch", [(n, b) for n in PARITY + ("no_eff",) for b in ("eta", "clip", "eps", "dpmpp2m") if (n, b) != ("no_eff", "eps")])
def test_sampler_branches_at_every_update_site(models, name, branch):
    """Check 6 at every site of the step update, and the second-order multistep update (solver="dpmpp2m") beside its branches: one
    site that drops a branch of the update fails here.  no_eff: the properties without the parity (its clips are too short)."""
    _check_branch(models, name, branch)


def test_other_known_tensors_reuse_the_graph(models):
    """Check 7: two loops with other `known` tensors (addresses and values) on one sampler: the second matches a fresh sampler bitwise
    (the kernels read the addresses from device slots; the sampler exposes no capture count to assert on)."""
    d = _setup("layer16")
    B, T = d["B"], d["T"]
    mask = _mask("edges", B, T)
    m = models("fp16")
    first = _gpu(m, d, mask=mask)
    keep = [torch.empty(3 * B * T * P, device="cuda")]                       # (moves the allocator on: the next tensors get other addresses)
    known2, eps2 = -0.25 * d["known"] + 0.1, torch.from_numpy(batch_noise(B, T, first=700))
    mask2 = _mask("channels", B, T)
    second = _gpu(m, d, mask=mask2, known=known2, eps=eps2)
    want = _gpu(make_model("fp16"), d, mask=mask2, known=known2, eps=eps2)
    assert torch.equal(second, want) and not torch.equal(second, first)
    assert torch.equal(second.cpu()[mask2 != 0], known2[mask2 != 0])
    del keep


def _trainer(model):
    from diffusion_conductor_amd import DDPMTrainer
    return DDPMTrainer(Namespace(device="cuda", diffusion_steps=S, is_train=False), model)


def test_long_piece(models):
    """Check 8: generate_long_music_motion on a synthetic mel of 2.5 windows, a window being 256 frames (`window=`: make_model's
    num_frames is 1800) with 64 frames of overlap: three windows at frames 0, 192, 384."""
    from diffusion_conductor_amd.harness import plan_windows
    T, ov, Tm = 256, 64, 1920
    L = (Tm - 1) // 3 + 1
    assert L == 640 and plan_windows(L, T, ov) == [(0, 0), (192, 64), (384, 64)]
    m = models("fp16")
    tr = _trainer(m)
    mel = torch.from_numpy(batch_mel(2, Tm, first=5)).cuda()
    noise = torch.from_numpy(np.concatenate([batch_noise(2, T, first=900 + 10 * w) for w in range(3)], axis=1)[:, :L]).cuda()
    out = tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T)
    assert tuple(out.shape) == (2, L, P) and torch.isfinite(out).all()
    # a hand-written chain of ddim_sample_loop(known=...) calls on piece 0
    gd = make_diffusion(S)
    xfp, xfo = m.encode_music(torch.stack([mel[0, 3 * s:3 * s + 3 * T] for s in (0, 192, 384)]), "cuda")
    chain, wins = torch.zeros(1, L, P, device="cuda"), []
    for w, s in enumerate((0, 192, 384)):
        kw = {}
        if w:
            km = torch.zeros(1, T, device="cuda")
            km[:, :ov] = 1
            kw = dict(known=chain[:, s:s + T].clone(), known_mask=km, known_noise=noise[:1, s:s + T].contiguous())
        r = gd.ddim_sample_loop(m, (1, T, P), noise=noise[:1, s:s + T].contiguous(), clip_denoised=False, progress=False,
                                model_kwargs={"xf_proj": xfp[w:w + 1].contiguous(), "xf_out": xfo[w:w + 1].contiguous(),
                                              "length": torch.LongTensor([T])}, **kw)
        wins.append(r)
        chain[:, s:s + T] = r
    for w in (1, 2):          # the frames two windows share are the same bits in both
        assert torch.equal(wins[w][:, :ov], wins[w - 1][:, T - ov:])
    alone = [tr.generate_long_music_motion(mel[i], P, overlap=ov, noise=noise[i:i + 1], window=T) for i in range(2)]
    assert torch.equal(alone[0], chain)
    for i in range(2):        # a batch of pieces gives each piece what it gets alone
        assert torch.equal(out[i:i + 1], alone[i])
    smooth = tr.generate_long_music_motion(mel, P, overlap=ov, noise=noise, window=T, smooth=19)
    assert torch.equal(smooth, native.savgol_filter(out, 19, 5)) and not torch.equal(smooth, out)
    seeded = [tr.generate_long_music_motion(mel[:1], P, overlap=ov, seed=11, window=T) for _ in range(2)]
    assert torch.equal(seeded[0], seeded[1]) and not torch.equal(seeded[0], alone[0])


def test_errors(models):
    """Check 9."""
    d = _setup("layer16")
    B, T = d["B"], d["T"]
    m = models("fp16")
    mask = _mask("edges", B, T)
    kw = dict(noise=d["x"].cuda(), clip_denoised=False, progress=False,
              model_kwargs={"xf_proj": d["xfp"].cuda(), "xf_out": d["xfo"].cuda(), "length": torch.LongTensor(d["length"])})
    gd = make_diffusion(S)
    with pytest.raises(ValueError, match="known_mask= without known="):
        gd.ddim_sample_loop(m, (B, T, P), known_mask=mask.cuda(), **kw)
    with pytest.raises(ValueError, match="must be"):
        gd.ddim_sample_loop(m, (B, T, P), known=d["known"][:, :T - 1].cuda(), known_mask=mask.cuda(), **kw)
    with pytest.raises(ValueError, match="known_mask must be"):
        gd.ddim_sample_loop(m, (B, T, P), known=d["known"].cuda(), known_mask=mask[:, :, :2].cuda(), **kw)
    with pytest.raises(NotImplementedError, match="native loop"):
        gd.ddim_sample_loop(m, (B, T, P), known=d["known"].cuda(), known_mask=mask.cuda(), denoised_fn=lambda x: x, **kw)
    # the C ABI refuses likewise: a mask without values, a mask without noise, a table without the known levels
    nat = m.set_conditioning(kw["model_kwargs"]["xf_proj"], kw["model_kwargs"]["xf_out"], d["length"])
    x = mask.cuda()
    with pytest.raises(native.DcError, match="mask without values"):
        nat.set_known(None, x, x)
    with pytest.raises(native.DcError, match="mask without noise"):
        nat.set_known(x, x, None)
    nat.set_known(x, x, x)
    with pytest.raises(native.DcError, match="dc_ddim_coefficients_known"):
        nat.ddim_loop(d["x"].cuda(), gd.native_coefficients(0.0), [], 0)
    nat.set_known(None, None, None)
    with pytest.raises(ValueError, match="shorter than one window"):
        _trainer(m).generate_long_music_motion(torch.zeros(5399, 128), P)
    out = gd.ddim_sample_loop(m, (B, T, P), **kw)                             # the sampler is as it was
    assert torch.equal(out, _gpu(m, d))
