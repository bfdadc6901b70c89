"""Several takes per music on one shared FiLM GEMM (include/dc_ddim.h, dc_sampler_set_conditioning_takes).
Needs an MI355X.

One shape (musics x takes x frames) per launch form of the internal batch - the forms are pinned on the CPU by tests/test_host_takes.py,
FORMS.  The main check needs no tolerance: the takes loop against the existing plain loop fed the same features tiled `takes` times and
the same noise, bit for bit - a FiLM tile does not depend on its token's position.  Parity against the oracle on the tiled features with
the project's bounds: 1e-3 per clip of >= 100 frames (the valid frames of the whole batch where every clip is shorter), and for the
guided case section 4.7's 1e-3 (|w| + |w - 1|).  S = 25 steps (the linear schedule needs S > 20)."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

from helpers import O, batch_mel, batch_noise, make_diffusion, make_model, oracle_params, rel_l2, xf_pair
from helpers_guided import ddim_guided_loop
from helpers_known import prefix_mask

from diffusion_conductor_amd import native
from diffusion_conductor_amd.synthetic import batch_step_noise

pytestmark = pytest.mark.gpu
S = 25
P = 26
W = 2.0

# name -> (model key, musics, takes, T, lengths of the musics or None, guidance scale or None)
SHAPES = {"layer16": ("fp16", 1, 2, 256, None, None),
          "narrow": ("fp16", 18, 4, 256, None, None),
          "wide_aligned": ("fp16", 40, 4, 256, None, None),
          "wide_flat": ("fp16", 56, 2, 300, None, None),          # flat 256-token units: token 16800, where take 1 begins, lies inside unit 65
          "group_96": ("fp16", 2, 2, 96, [96, 70], None),
          "group_20": ("fp16", 3, 2, 20, [20, 1, 13], None),
          "padded_300": ("fp16", 1, 3, 300, None, None),          # clip stride 320: a period of 10 groups
          "odd_255": ("fp16", 1, 2, 255, None, None),             # 255 tokens per take: no whole groups, the GEMM covers all of them
          "no_eff": ("no_eff", 2, 2, 96, [96, 70], None),
          "bf16": ("bf16", 1, 2, 256, None, None),
          "mixed": ("mixed", 1, 2, 256, None, None),
          "guided": ("fp16", 2, 2, 256, None, W)}
SHARING = [n for n in SHAPES if n != "odd_255"]


def _model(key):
    return make_model("fp16", no_eff=True) if key == "no_eff" else make_model(key)


@pytest.fixture(scope="module")
def models():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    made = {}

    def get(key):
        if key not in made:
            made[key] = _model(key)
        return made[key]
    return get


_inputs, _refs = {}, {}


def _setup(name):
    """Seeded inputs of a shape (host tensors), made once: B different musics, takes * B different noise clips."""
    if name not in _inputs:
        _, B, takes, T, length, w = SHAPES[name]
        xfp, xfo = xf_pair(B, T, first=60)
        n = takes * B
        _inputs[name] = dict(B=B, takes=takes, n=n, T=T, w=w, length=length or [T] * B, xfp=xfp, xfo=xfo,
                             x=torch.from_numpy(batch_noise(n, T, first=60)), known=0.5 * torch.from_numpy(batch_noise(n, T, first=260)),
                             eps=torch.from_numpy(batch_noise(n, T, first=460)))
    return _inputs[name]


def _loop(model, d, tiled, gd=None, idxs=(), mask=None, **kw):
    """The takes loop (`tiled` False: B musics, takes=) or the existing path on the features tiled `takes` times (no takes= at all)."""
    gd = gd or make_diffusion(S)
    if mask is not None:
        kw.update(known=d["known"].cuda(), known_mask=mask.cuda(), known_noise=d["eps"].cuda())
    kw.setdefault("clip_denoised", False)
    if d["w"] is not None:
        kw.setdefault("guidance_scale", d["w"])
    r = d["takes"] if tiled else 1
    mk = {"xf_proj": d["xfp"].repeat(r, 1, 1).cuda(), "xf_out": d["xfo"].repeat(r, 1, 1).cuda(), "length": torch.LongTensor(d["length"] * r)}
    if not tiled:
        kw["takes"] = d["takes"]
    out = gd.ddim_sample_loop(model, (d["n"], d["T"], P), noise=d["x"].cuda(), progress=False, idxs=list(idxs), model_kwargs=mk, **kw)
    torch.cuda.synchronize()
    return out


def _same(a, b, its):
    for it in its:
        assert torch.isfinite(a[it]).all() and torch.equal(a[it], b[it]), (it, rel_l2(a[it], b[it]))


@pytest.mark.parametrize("name", list(SHAPES))
def test_takes_are_the_tiled_loop_bit_for_bit(models, name, monkeypatch):
    """1: the takes loop FIRST, on a fresh sampler (no tile of an earlier loop lies in the workspace), with musics that differ; then
    the plain path on the tiled features; the final sample and two snapshots.  On the sharing shapes once more with
    DC_TAKES_FULL_FILM=1, the GEMM over every group."""
    key = SHAPES[name][0]
    d = _setup(name)
    its = (0, S // 2)
    got = _loop(_model(key), d, tiled=False, idxs=its)
    want = _loop(models(key), d, tiled=True, idxs=its)
    _same(got, want, its + (S,))
    B = d["B"]
    assert not torch.equal(got[S][0], got[S][B])               # two takes of music 0
    if B > 1:
        assert not torch.equal(got[S][0], got[S][1])
    if name in SHARING:
        monkeypatch.setenv("DC_TAKES_FULL_FILM", "1")
        full = _loop(_model(key), d, tiled=False, idxs=its)
        monkeypatch.delenv("DC_TAKES_FULL_FILM")
        _same(full, want, its + (S,))


def _oracle(name, clips):
    """The oracle's loop over caller clips `clips` of a shape alone (clip j * B + b: music b, the clip's own noise), once per shape."""
    if name not in _refs:
        d = _setup(name)
        B = d["B"]
        c = torch.tensor(clips)
        mus = torch.tensor([i % B for i in clips])
        ln = [d["length"][i % B] for i in clips]
        no_eff = SHAPES[name][0] == "no_eff"
        with torch.no_grad():
            if d["w"] is None:
                _refs[name] = O.ddim_sample_loop(oracle_params(), d["x"][c], d["xfp"][mus], d["xfo"][mus], ln, S, no_eff=no_eff)
            else:
                _refs[name] = ddim_guided_loop(oracle_params(), d["x"][c], d["xfp"][mus], d["xfo"][mus], ln, S, d["w"], no_eff=no_eff)
    return _refs[name]


@pytest.mark.parametrize("name", ["layer16", "wide_aligned", "wide_flat", "no_eff", "padded_300", "guided"])
def test_parity_against_the_oracle(models, name):
    """2: takes 0 and 1 of one music and take 1 of another (where there is one) against the oracle's loop over those clips."""
    key = SHAPES[name][0]
    d = _setup(name)
    B, T, w = d["B"], d["T"], d["w"]
    out = _loop(models(key), d, tiled=False).cpu()
    assert torch.isfinite(out).all()
    b0 = B - 1
    clips = [b0, B + b0] + ([B + (b0 - 1)] if B > 1 else [])      # music b0: take 0, take 1; music b0 - 1: take 1
    ref = _oracle(name, clips)
    bound = 1e-3 if w is None else 1e-3 * (abs(w) + abs(w - 1))
    if T >= 100:
        errs = {c: rel_l2(out[c], ref[j]) for j, c in enumerate(clips)}
    else:       # every clip shorter than 100 frames: the valid frames of the compared clips as one figure
        valid = prefix_mask(len(clips), T, P, [d["length"][c % B] for c in clips]) != 0
        errs = {"batch": rel_l2(out[torch.tensor(clips)][valid], ref[valid])}
    apart = rel_l2(out[clips[0]], out[clips[1]])
    print(f"takes parity {name}: worst {max(errs.values()):.3e} (bound {bound:.1e})  " + " ".join(f"[{c}] {e:.2e}" for c, e in errs.items()) +
          f"  takes of one music apart by {apart:.2f}")
    assert not torch.equal(out[clips[0]], out[clips[1]]) and apart > bound      # two takes of one music differ ...
    if B > 1:
        assert not torch.equal(out[clips[1]], out[clips[2]])                    # ... and so do two musics
    assert max(errs.values()) <= bound, errs


def _raw_takes(nat, xfp, xfo, length, takes, null=(None, None)):
    """dc_sampler_set_conditioning_takes itself (the Python surface sends takes = 1 to the entry points that existed before)."""
    la = np.ascontiguousarray(length, np.int32)
    nv = [None if v is None else np.ascontiguousarray(v.detach().cpu().numpy(), np.float32) for v in null]
    fp = C.POINTER(C.c_float)
    rc = native.lib().dc_sampler_set_conditioning_takes(nat._h, xfp.data_ptr(), xfo.data_ptr(), la.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        xfp.shape[0], xfp.shape[1], takes,
                                                        *[None if v is None else v.ctypes.data_as(fp) for v in nv], nat._stream())
    if rc:
        raise native.DcError(native.lib().dc_last_error().decode())
    nat.takes, nat.B, nat.T, nat.guided = takes, xfp.shape[0] * takes, xfp.shape[1], nv[0] is not None


def _raw_loop(nat, x, idx=3):
    nat.set_smoothing(0, 0)
    out, snaps = nat.ddim_loop(x, make_diffusion(S).native_coefficients(), [idx])
    assert nat.status() == 0
    return out, snaps


def test_takes_and_plain_conditionings_of_one_geometry_do_not_share_a_graph():
    """3a: takes(2) x 2 musics, then a plain conditioning of 4 (other) musics on the same sampler, and the reverse order: each the
    bits of a fresh sampler.  A replay of the other's graph would read the tiles of musics 0, 1 for clips 2, 3 - or all four columns
    where two were computed."""
    T = 256
    xfp, xfo = (t.cuda().contiguous() for t in xf_pair(4, T, first=60))
    x = torch.from_numpy(batch_noise(4, T, first=60)).cuda()

    def takes2(nat):
        nat.set_conditioning(xfp[:2].contiguous(), xfo[:2].contiguous(), [T, T], takes=2)
        return _raw_loop(nat, x)

    def plain4(nat):
        nat.set_conditioning(xfp, xfo, [T] * 4)
        return _raw_loop(nat, x)

    want_t, want_p = takes2(make_model("fp16")._ensure_native("cuda")), plain4(make_model("fp16")._ensure_native("cuda"))
    assert not torch.equal(want_t[0], want_p[0])
    for first, second, w1, w2 in ((takes2, plain4, want_t, want_p), (plain4, takes2, want_p, want_t)):
        nat = make_model("fp16")._ensure_native("cuda")
        a, b, a2 = first(nat), second(nat), first(nat)
        for got, want in ((a, w1), (b, w2), (a2, w1)):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("guided", [False, True])
def test_one_take_is_the_existing_conditioning(guided):
    """3b: dc_sampler_set_conditioning_takes(takes = 1) against dc_sampler_set_conditioning / _guided, bit for bit."""
    T = 256
    xfp, xfo = (t.cuda().contiguous() for t in xf_pair(2, T, first=60))
    x = torch.from_numpy(batch_noise(2, T, first=60)).cuda()
    m1, m2 = make_model("fp16"), make_model("fp16")
    null = m1.null_conditioning() if guided else None
    n1, n2 = m1._ensure_native("cuda"), m2._ensure_native("cuda")
    n1.set_conditioning(xfp, xfo, [T, 200], null=null)
    _raw_takes(n2, xfp, xfo, [T, 200], 1, null or (None, None))
    if guided:
        n1.set_guidance_scale(W), n2.set_guidance_scale(W)
    a, b = _raw_loop(n1, x), _raw_loop(n2, x)
    assert torch.isfinite(a[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if not guided:      # one take: single evaluations run as on any plain conditioning
        assert torch.equal(n1.denoise(x, [3, 3]), n2.denoise(x, [3, 3]))


def test_known_values_belong_to_their_takes_count():
    """3c: known tensors set under 2 takes of 1 music must not be read by a plain conditioning of 2 clips - the same caller geometry
    in another order -, nor the reverse.  All-ones masks: a loop that kept them would return `known`."""
    T = 256
    xfp, xfo = (t.cuda().contiguous() for t in xf_pair(2, T, first=60))
    x = torch.from_numpy(batch_noise(2, T, first=60)).cuda()
    known = 0.5 * torch.from_numpy(batch_noise(2, T, first=260)).cuda()
    ones = torch.ones(2, T, P, device="cuda")
    coef = make_diffusion(S).native_coefficients_known(0.0)

    def run(nat, takes, with_known):
        if takes == 2:
            nat.set_conditioning(xfp[:1].contiguous(), xfo[:1].contiguous(), [T], takes=2)
        else:
            nat.set_conditioning(xfp, xfo, [T, T])
        if with_known:
            nat.set_known(known, ones, x)
        out, _ = nat.ddim_loop(x, coef)
        assert nat.status() == 0
        return out

    fresh = make_model("fp16")._ensure_native("cuda")
    want_t, want_p = run(fresh, 2, False), run(fresh, 1, False)
    nat = make_model("fp16")._ensure_native("cuda")
    assert torch.equal(run(nat, 2, True), known)               # (set on this conditioning, they do act)
    assert torch.equal(run(nat, 1, False), want_p)             # takes(2) x 1 -> plain(2): dropped
    assert torch.equal(run(nat, 1, True), known)
    assert torch.equal(run(nat, 2, False), want_t)             # plain(2) -> takes(2) x 1: dropped


def test_seeded_step_noise_is_sized_for_all_takes(models):
    """3d: eta > 0 with the library's own draws - one [takes * B, T, P] buffer refilled per step - gives the bits of the same loop
    fed the draws as an explicit [S, takes * B, T, P] tensor."""
    d, m = _setup("narrow"), models("fp16")
    seeded = _loop(m, d, tiled=False, eta=0.5, step_noise_seed=7, idxs=(3,))
    z = torch.stack([native.step_noise((d["n"], d["T"], P), 7, it, "cuda") for it in range(S)])
    explicit = _loop(m, d, tiled=False, eta=0.5, step_noise=z, idxs=(3,))
    _same(seeded, explicit, (3, S))
    assert not torch.equal(seeded[S], _loop(m, d, tiled=False))
    assert not torch.equal(seeded[S][0], seeded[S][d["B"]])


def _eps_diffusion():
    from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType, get_named_beta_schedule)
    return GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=ModelMeanType.EPSILON,
                             model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)


@pytest.mark.parametrize("branch", ["eta", "clip", "eps", "known", "smooth", "dpmpp2m"])
def test_sampler_branches(models, branch):
    """4: the other branches of the update at 1 x 2 x 256: each the tiled plain path with the same options, bit for bit."""
    d, m = _setup("layer16"), models("fp16")
    kw, gd, mask, last = {}, None, None, S
    if branch == "eta":
        kw = dict(eta=0.5, step_noise=torch.from_numpy(batch_step_noise(S, d["n"], d["T"], first=60)).cuda())
    elif branch == "clip":
        kw = dict(clip_denoised=True)
    elif branch == "eps":           # (clipped, as the EPSILON cases of tests/test_gpu_known.py and test_gpu_guided.py are)
        kw, gd = dict(clip_denoised=True), _eps_diffusion()
    elif branch == "known":
        mask = prefix_mask(d["n"], d["T"], P, [100, 60])
        mask[:, :, 5] = 1
    elif branch == "smooth":
        kw = dict(smooth=(19, 5))
    else:
        kw, last = dict(steps=10, spacing="logsnr", solver="dpmpp2m"), 10
    got = _loop(m, d, tiled=False, gd=gd, mask=mask, idxs=(3,), **kw)
    want = _loop(m, d, tiled=True, gd=gd, mask=mask, idxs=(3,), **kw)
    _same(got, want, (3, last))
    base = _loop(m, d, tiled=False)
    assert not torch.equal(got[last], base)                    # the branch did act
    if branch == "known":
        k = mask != 0
        assert torch.equal(got[last].cpu()[k], d["known"][k])


def test_errors(models):
    """5."""
    d, m = _setup("layer16"), models("fp16")
    T = d["T"]
    xfp, xfo = d["xfp"].cuda().contiguous(), d["xfo"].cuda().contiguous()
    nat = m._ensure_native("cuda")
    m._cond_key = None
    npj, nout = m.null_conditioning()
    for bad in (0, -1):
        with pytest.raises(native.DcError, match="takes"):
            _raw_takes(nat, xfp, xfo, d["length"], bad)
    with pytest.raises(native.DcError, match="null pair"):
        nat.set_conditioning(xfp, xfo, d["length"], null=(None, nout), takes=2)
    with pytest.raises(native.DcError, match="null pair"):
        nat.set_conditioning(xfp, xfo, d["length"], null=(npj, None), takes=2)
    with pytest.raises(native.DcError, match="null pair"):
        _raw_takes(nat, xfp, xfo, d["length"], 1, (npj, None))
    nat.set_conditioning(xfp, xfo, d["length"], takes=2)
    x = d["x"].cuda()
    with pytest.raises(native.DcError, match="takes"):
        nat.denoise(x, [3] * d["n"])
    with pytest.raises(native.DcError, match="takes"):
        nat.debug_denoise(x, [3] * d["n"], 8, 0)
    with pytest.raises(native.DcError, match="takes"):
        nat.debug_layer(np.zeros((d["n"], T, 128), np.float32), [3] * d["n"], 0, 1, 1)
    nat.set_conditioning(xfp, xfo, d["length"])                # a plain conditioning switches takes off
    assert nat.takes == 1 and tuple(nat.denoise(x[:1].contiguous(), [3]).shape) == (1, T, P)
    m._cond_key = None
    gd = make_diffusion(S)
    kw = dict(noise=x, clip_denoised=False, progress=False, model_kwargs={"xf_proj": xfp, "xf_out": xfo, "length": torch.LongTensor(d["length"])})
    with pytest.raises(ValueError, match="takes x musics"):
        gd.ddim_sample_loop(m, (3, T, P), takes=2, **kw)
    with pytest.raises(ValueError, match="takes"):
        gd.ddim_sample_loop(m, (2, T, P), takes=0, **kw)
    with pytest.raises(ValueError, match="progressive"):
        next(gd.ddim_sample_loop_progressive(m, (2, T, P), takes=2, **kw))
    with pytest.raises(ValueError, match="takes"):
        gd.ddim_sample_loop(m, (2, T, P), takes=2, denoised_fn=lambda v: v, **kw)
    out = gd.ddim_sample_loop(m, (2, T, P), takes=2, **kw)                          # the sampler is as it was
    assert torch.equal(out, _loop(make_model("fp16"), d, tiled=True))


def test_generate_music_motion_takes():
    """5, end to end: DDPMTrainer.generate_music_motion(mel, takes=2) for 2 musics of 256 frames on `mixed`: [4, 256, 26] take-major,
    the bits of the call on the mel tiled twice, and the oracle's loop fed by the oracle's encode_music within 1e-3."""
    from diffusion_conductor_amd import DDPMTrainer
    tr = DDPMTrainer(Namespace(device="cuda", diffusion_steps=S, is_train=False), make_model("mixed"))
    mel = torch.from_numpy(batch_mel(2, 768, first=5))
    noise = torch.from_numpy(batch_noise(4, 256, first=900))
    out = tr.generate_music_motion(mel, P, noise=noise, takes=2).cpu()
    assert tuple(out.shape) == (4, 256, P)
    tiled = tr.generate_music_motion(mel.repeat(2, 1, 1), P, noise=noise).cpu()
    assert torch.equal(out, tiled)
    seeded = tr.generate_music_motion(mel, P, seed=3, takes=2).cpu()               # `seed` draws all takes * B clips
    assert tuple(seeded.shape) == (4, 256, P) and not torch.equal(seeded[0], seeded[2])
    p = oracle_params()
    with torch.no_grad():
        xfp, xfo = O.encode_music(p, mel)
        ref = O.ddim_sample_loop(p, noise, xfp.repeat(2, 1, 1), xfo.repeat(2, 1, 1), [256] * 4, S)
    errs = [rel_l2(out[c], ref[c]) for c in range(4)]
    print("generate_music_motion takes=2 (mixed): " + " ".join(f"{e:.3e}" for e in errs) + f"; takes of music 0 apart by {rel_l2(out[0], out[2]):.2f}")
    assert max(errs) <= 1e-3 and not torch.equal(out[0], out[2]) and not torch.equal(out[0], out[1])
