"""What a sampling loop reads but never recomputes, against fp64: the buffers dc_sampler_set_conditioning makes once per batch -
"pp" = linear(xf_proj), the per-clip, per-layer cross-attention matrices "a_ca" and their 16-token copy "a_ca16" - and the timestep
table "temb" of dc_sampler_finalize_params, read back with dc_sampler_debug_read and decoded from the writers' own indexing
(helpers.decode_*).  No scale factor turns out to be folded into the stored matrices: log2 e goes into the key
projection and exp2 takes it out again, so "a_ca" holds softmax(K)^T V itself and "pp" linear(xf_proj) itself.

Every bound comes from the reference side, per case, on the CPU (helpers.cond_reference, oracle arithmetic):
  A_ca from hi + lo, and pp:  rel-L2 per layer and clip (normalised by that clip's own norm) <= 4 x the error of the oracle's
                              split-bf16 emulation Emu("x3", film_store_f16=False) of the same computation against fp64;
  A_ca from hi alone:         <= 4 x the error of rounding the fp64 matrix to the storage type (fp16 / bf16);
  a_ca16:                     the bits of a_ca's hi fragments, re-ordered;
  temb:                       per row <= 4 x the error of the oracle's plain fp32 evaluation against fp64 on the same fp32 arguments.
The near-degenerate checkpoint's clips take the larger of the emulation's error and the error of the reference's own fp32 formulation:
there the reference is ill-conditioned itself, and only its own loss is forgiven; the two near-degenerate clips are held to 4 x the fp32
formulation's error alone as well (near_degenerate_failures).  Each comparison prints its figure beside its bound."""
import numpy as np
import pytest
import torch

from helpers import (DenoiserConfig, O, batch_music_features, cond_reference, colspace_state_dict, decode_a_ca, decode_a_ca16,
                     decode_pp, f16_bits_to_f64, peaky_state_dict, rankdef_state_dict, round_to_16, state_dict_np)
from diffusion_conductor_amd.synthetic import smooth_mel

pytestmark = pytest.mark.gpu
L, H = 8, 8
FMT = {"fp16": "f16", "bf16x3": "bf16"}          # precision -> storage type of A_ca
PRECISIONS = tuple(FMT)
PEAKY_FACTOR = 8.0                               # of ca_block.key.weight; raised until the fp64 reference's largest softmax weight exceeds 0.9
X3 = O.Emu("x3", film_store_f16=False)


# ---- checkpoints, samplers, features, references (each built once) -----------------------------------------------------------
def _long_state_dict(T=4032):
    sd = {k: np.asarray(v) for k, v in state_dict_np().items()}
    sd["sequence_embedding"] = np.concatenate([sd["sequence_embedding"]] * (-(-T // 1800)))[:T]
    return sd


_CKPT = {"seeded": lambda: {k: np.asarray(v) for k, v in state_dict_np().items()}, "peaky": lambda: peaky_state_dict(PEAKY_FACTOR),
         "colspace": lambda: colspace_state_dict()[0], "rankdef": rankdef_state_dict, "long": _long_state_dict}
_sd, _params, _refs = {}, {}, {}


def state_dict_of(ckpt):
    if ckpt not in _sd:
        _sd[ckpt] = _CKPT[ckpt]()
    return _sd[ckpt]


def params_of(ckpt, dtype):
    if (ckpt, dtype) not in _params:
        _params[ckpt, dtype] = O.to_torch_params(state_dict_of(ckpt), dtype)
    return _params[ckpt, dtype]


def new_sampler(ckpt, precision):
    from diffusion_conductor_amd import native
    nat = native.NativeSampler(DenoiserConfig(num_frames=4032 if ckpt == "long" else 1800), precision, 1000, 0)
    nat.load_state_dict(state_dict_of(ckpt))
    return nat


@pytest.fixture(scope="module")
def samplers():
    """(checkpoint, precision) -> NativeSampler, built on first use and kept: the long-clip model and the two modified checkpoints
    are packed once."""
    made = {}

    def get(ckpt, precision):
        if (ckpt, precision) not in made:
            made[ckpt, precision] = new_sampler(ckpt, precision)
        return made[ckpt, precision]
    yield get
    for nat in made.values():
        nat.close()


FAMILIES = ("unit", "x30", "off50", "tiny", "zero", "const", "loud", "relu", "encoder")


def clip_features(kind, T, clip):
    """One clip's music features [T, 64] of a family (`clip`: which seeded draw)."""
    x = batch_music_features(1, T, first=clip)[0]
    if kind == "unit":
        return x
    if kind == "x30":
        return x * np.float32(30)
    if kind == "off50":
        return x + np.float32(50)
    if kind == "tiny":
        return x * np.float32(1e-4)
    if kind == "zero":
        return np.zeros_like(x)
    if kind == "const":                 # every frame equal: every softmax weight is 1 / N
        return np.repeat(x[:1], T, 0)
    if kind == "loud":                  # one loud frame
        x = x.copy()
        x[T // 3] *= np.float32(100)
        return x
    if kind == "relu":                  # non-negative, as behind the encoder's last ReLU
        return np.maximum(x, 0)
    if kind == "encoder":               # the encoder's own output for a smooth mel
        with torch.no_grad():
            return O.encode_music(params_of("seeded", torch.float32), torch.from_numpy(smooth_mel(clip, n_frames=3 * T - 2)[None]))[1][0].numpy()
    raise KeyError(kind)


def near_degenerate_features(T, delta, clip):
    """Every frame -u + delta N(0,1) for the column-space checkpoint's u: linear(x) = delta W n."""
    u = colspace_state_dict()[1]
    return (-u[None] + np.float32(delta) * batch_music_features(1, T, first=clip)[0]).astype(np.float32)


def batch_of(kinds, T, first=0):
    """[B, T, 64] with clip b of family kinds[b] (a name of FAMILIES, or ("near", delta))."""
    rows = [near_degenerate_features(T, k[1], first + b) if isinstance(k, tuple) else clip_features(k, T, first + b)
            for b, k in enumerate(kinds)]
    return np.ascontiguousarray(np.stack(rows), np.float32)


def project(ckpt, xf):
    """(xf_proj, xf_out) as encode_music hands them on: xf_proj = proj(xf_out)."""
    p = params_of(ckpt, torch.float32)
    xfo = torch.from_numpy(xf)
    return torch.nn.functional.linear(xfo, p["proj.weight"], p["proj.bias"]).contiguous(), xfo


def _rel(a, b, axes):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    num = np.sqrt(((a - b) ** 2).sum(axes))
    den = np.sqrt((b ** 2).sum(axes))
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))


def a_err(A, A64):
    """rel-L2 per layer and clip [L, B], each normalised by that clip's own norm."""
    return _rel(A, A64, (2, 3, 4))


def pp_err(pp, pp64):
    return _rel(pp, pp64, (1, 2))


def reference(key, ckpt, xfp, xfo, own_fp32=False):
    """fp64 reference of one batch and, from the reference side alone, the error figures the bounds are made of.  Computed once per
    `key` and never modified.  own_fp32: also forgive the loss of the reference's own fp32 formulation (near-degenerate clips)."""
    if key in _refs:
        return _refs[key]
    p64, p32 = params_of(ckpt, torch.float64), params_of(ckpt, torch.float32)
    stats = {}
    pp64 = cond_reference(p64, xfp, num_layers=0)[0]
    _, A64 = cond_reference(p64, xfo, stats=stats)
    with torch.no_grad():
        pp_emu = X3.linear(xfp, p32["linear.weight"], p32["linear.bias"]).double().numpy()
    A_emu = cond_reference(p32, xfo, X3)[1]
    e_a = e_emu = a_err(A_emu, A64)
    e_own = a_err(cond_reference(p32, xfo)[1], A64) if own_fp32 else None
    if own_fp32:
        e_a = np.maximum(e_emu, e_own)
    r = {"pp64": pp64, "A64": A64, "A_emu": A_emu, "peak": stats["peak"], "e_pp": pp_err(pp_emu, pp64), "e_a": e_a, "e_emu": e_emu, "e_own": e_own,
         "e_r16": {f: a_err(round_to_16(A64, f), A64) for f in ("f16", "bf16")}}
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _refs[key] = r
    return r


# ---- reading the buffers and judging them ---------------------------------------------------------------------------------------
def read_raw(nat, B, want16=False):
    Tp = nat.clip_stride()
    G = (B * Tp + 31) // 32
    raw = {"Tp": Tp, "pp": nat.debug_read("pp", np.float32, G * 32 * 64 * 8), "a_ca": nat.debug_read("a_ca", np.uint16, L * B * 16 * 64 * 8)}
    if want16:
        raw["a_ca16"] = nat.debug_read("a_ca16", np.uint16, L * B * 8 * 64 * 8)
    return raw


def decode(raw, B, T, fmt):
    pp, past = decode_pp(raw["pp"], B, raw["Tp"])
    hi, lo, off = decode_a_ca(raw["a_ca"], L, B)
    d = {"pp": pp[:, :T], "pad": np.concatenate([pp[:, T:].ravel(), past.ravel()]), "hi_bits": hi, "off": off,
         "A_hi": f16_bits_to_f64(hi, fmt), "A": f16_bits_to_f64(hi, fmt) + f16_bits_to_f64(lo, fmt)}
    if "a_ca16" in raw:
        d["hi16_bits"], d["off16"] = decode_a_ca16(raw["a_ca16"], L, B)
    return d


def failures(d, ref, fmt, tag=""):
    """Every comparison of one decoded batch with its reference: prints figure and bound, returns the names of those that fail."""
    bad = []

    def judge(name, err, bound):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        print(f"  {tag} {name}: worst err {err[i]:.2e} / bound {bound[i]:.2e} = {ratio[i]:.2f} at {tuple(int(k) for k in i)}"
              f"  (err {err.min():.1e} .. {err.max():.1e}, bound {bound.min():.1e} .. {bound.max():.1e})")
        bad.extend(f"{name}{tuple(int(k) for k in at)}" for at in np.argwhere(~(err <= bound)))

    judge("pp[clip]", pp_err(d["pp"], ref["pp64"]), 4 * ref["e_pp"])
    judge("A_ca hi+lo[layer,clip]", a_err(d["A"], ref["A64"]), 4 * ref["e_a"])
    judge("A_ca hi[layer,clip]", a_err(d["A_hi"], ref["A64"]), 4 * ref["e_r16"][fmt])
    if d["pad"].size and np.any(d["pad"].view(np.uint32) != 0):
        bad.append("pp padding rows not zero")
    if np.any(d["off"] != 0):
        bad.append("a_ca cross-head entries not zero")
    if "hi16_bits" in d:
        same = np.array_equal(d["hi16_bits"], d["hi_bits"]) and not np.any(d["off16"] != 0)
        print(f"  {tag} a_ca16: bits of a_ca's hi fragments {'equal' if same else 'DIFFER'}")
        if not same:
            bad.append("a_ca16")
    return bad


def run_case(nat, precision, ckpt, key, xf, length=None, own_fp32=False, tag=None):
    B, T = xf.shape[:2]
    xfp, xfo = project(ckpt, xf)
    ref = reference(key, ckpt, xfp, xfo, own_fp32)
    nat.set_conditioning(xfp.cuda(), xfo.cuda(), length)
    want16 = precision == "fp16"
    d = decode(read_raw(nat, B, want16), B, T, FMT[precision])
    tag = tag or f"{ckpt} {precision} ({B},{T}) stride {nat.clip_stride()}"
    print()
    return failures(d, ref, FMT[precision], tag), d, ref


# ---- shapes, unit features ------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 31), (2, 32), (3, 33),            # one group, padded rows, first straddle
          (1, 224), (1, 256), (1, 257),                  # 7 / 8 / 9 groups of a pre-pass workgroup's 8: the last one partly idle
          (5, 77), (2, 1800), (9, 1800), (33, 300),      # 16-token form, narrow, wide
          (40, 777)]                                     # fp16: a clip stride that is not whole groups, in the wide form


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,T", SHAPES)
def test_conditioning_shapes(samplers, B, T, precision):
    nat = samplers("seeded", precision)
    bad, _, _ = run_case(nat, precision, "seeded", ("unit", B, T), batch_of(["unit"] * B, T))
    if (B, T) in ((5, 77), (3, 33)) or ((B, T) == (40, 777) and precision == "fp16"):
        assert nat.clip_stride() % 32 != 0, "this shape is here for groups that hold two clips' records"
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS)
def test_conditioning_long_clip_combine_loop(samplers, precision):
    """A clip of more than 64 groups: each of the combine's 8 eighths holds more than its 8 preloaded records and loops."""
    B, T = 2, 2500
    nat = samplers("long", precision)
    bad, _, _ = run_case(nat, precision, "long", ("unit", B, T), batch_of(["unit"] * B, T))
    assert (nat.clip_stride() // 32 + 7) // 8 > 8
    assert not bad, bad


def test_a_ca16_is_refused_where_it_is_not_held(samplers):
    from diffusion_conductor_amd import native
    nat = samplers("seeded", "bf16x3")
    xfp, xfo = project("seeded", batch_of(["unit"], 64))
    nat.set_conditioning(xfp.cuda(), xfo.cuda())
    with pytest.raises(native.DcError, match="not filled"):
        nat.debug_read("a_ca16", np.uint16, 64)
    nat = samplers("seeded", "fp16")
    nat.set_conditioning(xfp.cuda(), xfo.cuda())
    with pytest.raises(native.DcError, match="holds"):
        nat.debug_read("a_ca16", np.uint16, L * 8 * 1024 // 2 + 1)


# ---- contents: each clip of a batch carries another family -----------------------------------------------------------------------
CONTENT_BATCHES = {33: [("x30", "off50", "tiny"), ("zero", "const", "loud"), ("relu", "encoder", "unit")],
                   288: [("x30", "off50"), ("tiny", "zero"), ("const", "loud"), ("relu", "encoder")]}
CONTENT_CASES = [(T, kinds) for T, batches in CONTENT_BATCHES.items() for kinds in batches]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T,kinds", CONTENT_CASES, ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_conditioning_contents(samplers, T, kinds, precision):
    bad, _, _ = run_case(samplers("seeded", precision), precision, "seeded", ("seeded", kinds, T), batch_of(kinds, T, first=20))
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T,kinds", [(33, ("unit", "relu", "loud")), (288, ("unit", "encoder")), (1800, ("unit",))],
                         ids=lambda v: "-".join(v) if isinstance(v, tuple) else str(v))
def test_conditioning_peaky_checkpoint(samplers, T, kinds, precision):
    """Keys x PEAKY_FACTOR and log-normal text_norm gains: most of a softmax column's weight sits on one frame, and the units whose
    local maximum lies far below the clip's combine with weights that underflow."""
    bad, _, ref = run_case(samplers("peaky", precision), precision, "peaky", ("peaky", kinds, T), batch_of(kinds, T, first=30))
    print(f"  largest softmax weight of the fp64 reference: {ref['peak']:.4f}")
    assert ref["peak"] > 0.9
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("T", [33, 288])
def test_conditioning_near_degenerate_checkpoint(samplers, T, precision):
    """linear.bias = linear.weight @ u and frames near -u: linear(x) is nearly constant over its 512 outputs and text_norm's variance
    meets its eps.  As a quadratic form of x that variance cancels (tests/study_cond_rstd.py: rstd off by 1e-3 ... 4e-3), and so
    does the composed A x + d on split-bf16 operands (A_ca off by 1e-3 ... 4.4e-3, which the fp16 head's bound does not forgive):
    the pre-pass shifts the features by the least-squares u first (centre_linear).  One clip at delta = 1e-2,
    one at 1e-3, one of unit features."""
    kinds = (("near", 1e-2), ("near", 1e-3), "unit")
    bad, d, ref = run_case(samplers("colspace", precision), precision, "colspace", ("colspace", T), batch_of(kinds, T, first=40), own_fp32=True)
    bad += near_degenerate_failures(d, ref)
    assert not bad, bad


def near_degenerate_failures(d, ref):
    """Per clip, worst layer: the measured error of A_ca from hi + lo beside the two figures its bound is the larger of - the split-bf16
    emulation's error, which stands at 1e-3 ... 4e-3 on the near-degenerate clips, and the reference's own fp32 formulation's.
    The emulation's figure is the loss of an unshifted sum on split-bf16 operands, which the library no longer has, so the two
    near-degenerate clips are held to the tighter of the two as well: 4 x the error of the reference's own fp32 formulation, the
    only loss that is the reference's and not the library's (1.4e-5 ... 1.6e-4 here).  Without the shift they stand at 1e-3 ... 4.4e-3."""
    err, bad = a_err(d["A"], ref["A64"]), []
    for b, name in enumerate(("delta 1e-2", "delta 1e-3", "unit")):
        ratio = (err[:, b] / (4 * ref["e_own"][:, b])).max()
        print(f"  clip {b} ({name}): A_ca hi+lo err {err[:, b].max():.2e}; split-bf16 emulation {ref['e_emu'][:, b].max():.2e}, "
              f"reference's fp32 formulation {ref['e_own'][:, b].max():.2e} (err / (4 x fp32 formulation) = {ratio:.2f})")
        if b < 2 and not ratio <= 1:
            bad.append(f"A_ca hi+lo against the fp32 formulation alone, clip {b}")
    return bad


@pytest.mark.parametrize("precision", PRECISIONS)
def test_conditioning_rank_deficient_linear(samplers, precision):
    """A linear.weight without full column rank (column 1 = column 0): the normal equations of the pre-pass's least-squares shift are
    singular, the host keeps u = 0 and the constants of the unshifted form, and the buffers meet the same bounds."""
    kinds = ("unit", "relu", "x30")
    bad, _, _ = run_case(samplers("rankdef", precision), precision, "rankdef", ("rankdef", 33), batch_of(kinds, 33, first=50))
    assert not bad, bad


def test_the_bounds_catch_one_wrong_layer_or_clip():
    """On the reference side's own arrays (no GPU work): the split-bf16 emulation passes as a stand-in for the decoded buffers; one
    layer's or one clip's matrices off by 1e-4 relative fail, and name exactly that layer and clip."""
    B, T = 3, 33
    xfp, xfo = project("seeded", batch_of(["unit"] * B, T))
    ref = reference(("unit", B, T), "seeded", xfp, xfo)

    def verdict(A):
        d = {"pp": ref["pp64"], "pad": np.zeros(0, np.float32), "off": np.zeros(1, np.uint16), "A": A, "A_hi": round_to_16(A, "f16")}
        return failures(d, ref, "f16", "stand-in")
    assert verdict(ref["A_emu"]) == []
    A = ref["A_emu"].copy()
    A[5, 1] *= 1 + 1e-4
    assert verdict(A) == ["A_ca hi+lo[layer,clip](5, 1)"]
    A = ref["A_emu"].copy()
    A[:, 2] *= 1 + 1e-4
    assert verdict(A) == [f"A_ca hi+lo[layer,clip]({l}, 2)" for l in range(L)]
    A = ref["A_emu"].copy()
    A[3] *= 1 + 1e-4
    assert verdict(A) == [f"A_ca hi+lo[layer,clip](3, {b})" for b in range(B)]


# ---- the DC_COND_512=1 forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,T", [(3, 33), (1, 257), (40, 777)])
def test_conditioning_image_form(samplers, monkeypatch, B, T, precision):
    """DC_COND_512=1 (read per call): pp from fp32 FMAs (k_cond_embed<0>), the records from the normalised [tokens][512] image
    (k_cond_embed<1>, k_cond_ca_partials).  Same checks, same bounds; the two forms' mutual difference is printed beside them."""
    nat = samplers("seeded", precision)
    xf = batch_of(["unit"] * B, T)
    _, d64, ref = run_case(nat, precision, "seeded", ("unit", B, T), xf, tag=f"default form {precision} ({B},{T})")
    monkeypatch.setenv("DC_COND_512", "1")
    bad, d512, _ = run_case(nat, precision, "seeded", ("unit", B, T), xf, tag=f"DC_COND_512=1 {precision} ({B},{T})")
    monkeypatch.delenv("DC_COND_512")
    print(f"  between the forms: A_ca hi+lo {a_err(d512['A'], d64['A']).max():.2e}, pp {pp_err(d512['pp'], d64['pp']).max():.2e}"
          f"  (bounds vs fp64: {4 * ref['e_a'].min():.1e} .. {4 * ref['e_a'].max():.1e}, pp {4 * ref['e_pp'].min():.1e} .. {4 * ref['e_pp'].max():.1e})")
    assert not bad, bad


@pytest.mark.parametrize("precision", PRECISIONS)
def test_near_degenerate_image_form(samplers, monkeypatch, precision):
    """The image form normalises directly (two passes over the 512 outputs): the in-library comparison of the near-degenerate case."""
    kinds = (("near", 1e-2), ("near", 1e-3), "unit")
    monkeypatch.setenv("DC_COND_512", "1")
    bad, d, ref = run_case(samplers("colspace", precision), precision, "colspace", ("colspace", 33), batch_of(kinds, 33, first=40), own_fp32=True,
                           tag=f"DC_COND_512=1 colspace {precision} (3,33)")
    bad += near_degenerate_failures(d, ref)
    assert not bad, bad


# ---- properties, bit for bit --------------------------------------------------------------------------------------------------
def _set(nat, xf, length=None, ckpt="seeded"):
    xfp, xfo = project(ckpt, xf)
    nat.set_conditioning(xfp.cuda(), xfo.cuda(), length)
    return read_raw(nat, xf.shape[0], want16=nat.precision == "fp16")


def _same(a, b):
    return a["Tp"] == b["Tp"] and all(np.array_equal(a[k], b[k]) for k in a if k != "Tp")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B,T", [(3, 33), (2, 300)])
def test_a_ca_and_pp_do_not_depend_on_length(samplers, B, T, precision):
    """The reference never masks music frames (transformer.py:149-155 take no src_mask)."""
    nat = samplers("seeded", precision)
    xf = batch_of(["unit"] * B, T, first=3)
    full = _set(nat, xf)
    assert _same(full, _set(nat, xf, [1] + [T] * (B - 1)))
    assert _same(full, _set(nat, xf, [1] * B))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_clip_is_the_same_wherever_it_stands(samplers, precision):
    """Alone, first, last and in the reversed batch, on a padded clip stride: the clip's A_ca and pp rows, bit for bit."""
    T = 300
    nat = samplers("seeded", precision)
    xf = batch_of(["unit", "relu", "loud"], T, first=7)

    def clip(order, b):
        raw = _set(nat, np.ascontiguousarray(xf[order]))
        Tp = raw["Tp"]
        assert Tp % 32 == 0 and Tp > T
        pp, _ = decode_pp(raw["pp"], len(order), Tp)
        return raw["a_ca"].reshape(L, len(order), -1)[:, b].copy(), pp[b].copy()
    alone = clip([1], 0)
    for order, b in (([1, 0, 2], 0), ([0, 2, 1], 2), ([2, 1, 0], 1), ([0, 1, 2], 1)):
        got = clip(order, b)
        assert np.array_equal(alone[0], got[0]) and np.array_equal(alone[1], got[1]), (order, b)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_conditioning_is_replaced_and_reused_cleanly(samplers, precision):
    """A second call at the same shape with other features gives those features' result; after a larger (B, T) the smaller shape's
    buffers are a fresh sampler's, the pp rows of padding frames exactly zero; calling twice gives identical bytes."""
    B, T = 2, 290
    xa, xb = batch_of(["unit"] * B, T, first=11), batch_of(["x30", "relu"], T, first=13)
    fresh = new_sampler("seeded", precision)
    want_a, want_b = _set(fresh, xa), _set(fresh, xb)
    fresh.close()
    nat = samplers("seeded", precision)
    _set(nat, batch_of(["off50"] * 5, 700, first=17))          # larger, and full of other values
    got_a = _set(nat, xa)
    assert _same(got_a, want_a)
    assert _same(_set(nat, xa), got_a)
    assert _same(_set(nat, xb), want_b)
    assert _same(_set(nat, xa), want_a)
    pp, past = decode_pp(got_a["pp"], B, got_a["Tp"])
    assert got_a["Tp"] > T and not np.any(pp[:, T:].view(np.uint32)) and not np.any(past.view(np.uint32))


# ---- the timestep table ---------------------------------------------------------------------------------------------------------
def test_timestep_table_every_row(samplers):
    """All max_timesteps rows x 512 against fp64 time_embed on the reference's fp32 arguments (t * freqs is formed in fp32, cosine,
    sine and the MLP run in double), row by row: rows near t = 999 carry arguments of hundreds of radians and must not hide in the
    table's norm.  The table does not depend on the sampler's precision.
    freqs is the correctly rounded fp32 exp of the reference's fp32 exponent, which the library's table holds by construction.
    torch.exp itself is not reproducible to the ulp (on AVX-512 CPUs its fp32 result is one ulp off at k = 22): taken as the
    argument, that ulp times t = 999 is 4e-6 rad and reads as a row error of 4.8e-6 against bounds of 1.1 ... 1.6e-6 for every
    row from t = 275 on, of a table that is right.  So the test asserts that torch's freqs lie within one ulp of the correctly rounded
    ones, and both sides of the bound - the fp64 result and the plain fp32 evaluation - take the same correctly rounded arguments."""
    F = torch.nn.functional
    NT = 1000
    p32, p64 = params_of("seeded", torch.float32), params_of("seeded", torch.float64)
    t = torch.arange(NT)
    with torch.no_grad():
        expo = -np.log(10000.0) * torch.arange(0, 64, dtype=torch.float32) / 64
        freqs = torch.exp(expo.double()).float()
        assert torch.all((torch.exp(expo).view(torch.int32) - freqs.view(torch.int32)).abs() <= 1)
        args = t[:, None].float() * freqs[None]
        te64 = torch.cat([torch.cos(args.double()), torch.sin(args.double())], -1)
        ref = F.linear(F.silu(F.linear(te64, p64["time_embed.0.weight"], p64["time_embed.0.bias"])), p64["time_embed.2.weight"],
                       p64["time_embed.2.bias"]).numpy()
        te32 = torch.cat([torch.cos(args), torch.sin(args)], -1)          # O.timestep_embedding on these arguments
        own = F.linear(F.silu(F.linear(te32, p32["time_embed.0.weight"], p32["time_embed.0.bias"])), p32["time_embed.2.weight"],
                       p32["time_embed.2.bias"]).double().numpy()
    bound = 4 * _rel(own, ref, (1,))
    got = samplers("seeded", "fp16").debug_read("temb", np.float32, NT * 512).reshape(NT, 512)
    err = _rel(got, ref, (1,))
    ratio = err / bound
    i = int(np.argmax(ratio))
    print(f"\n  temb: worst row t={i}: err {err[i]:.2e} / bound {bound[i]:.2e} = {ratio[i]:.2f}  (err {err.min():.1e} .. {err.max():.1e}, "
          f"bound {bound.min():.1e} .. {bound.max():.1e}; rows 990..999 err {err[990:].max():.2e})")
    with torch.no_grad():      # beside it, unasserted: the distance from what the oracle itself computes, torch's own exp included
        te_o = O.timestep_embedding(t, 128)
        own_o = F.linear(F.silu(F.linear(te_o, p32["time_embed.0.weight"], p32["time_embed.0.bias"])), p32["time_embed.2.weight"],
                         p32["time_embed.2.bias"]).double().numpy()
        ref_o = F.linear(F.silu(F.linear(te_o.double(), p64["time_embed.0.weight"], p64["time_embed.0.bias"])), p64["time_embed.2.weight"],
                         p64["time_embed.2.bias"]).numpy()
    print(f"  temb against the oracle's own fp32 table (O.timestep_embedding, torch.exp): worst row {_rel(got, own_o, (1,)).max():.2e}; "
          f"against fp64 on the oracle's own cosines and sines {_rel(got, ref_o, (1,)).max():.2e}")
    other = new_sampler("seeded", "bf16")
    same = np.array_equal(other.debug_read("temb", np.float32, NT * 512).reshape(NT, 512), got)
    other.close()
    assert same, "the table of a bf16 sampler differs from an fp16 sampler's"
    assert np.all(err <= bound), np.argwhere(~(err <= bound)).ravel()[:10]
