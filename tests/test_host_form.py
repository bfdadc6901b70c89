"""The launch rule on the CPU: csrc/dc_form.h decides which form a denoiser evaluation takes (records, units, fusions, tiles), the
clip stride, the steps per graph, the precise tail and a whole loop's plan (its graphs, their keys and replays, the options of every
step) - pure integer arithmetic, no HIP.  tests/form_probe.cpp includes the header,
is compiled with the host compiler and prints the decision for the cases below; the expectations are DESIGN.md sections 4.3 and 5
at 256 compute units (fp16, linear attention, 8 layers unless said)."""
import pytest

from helpers import STEP_FORM_FIELDS, form_probe

from diffusion_conductor_amd import native

BASE = "B=32 Tx=1800 loop=1 graph_step=0 next_plain=1 g1_loop=1"     # a captured loop step with a plain successor, in a loop with a tail
FIELDS = ("stride", "bits", "error") + STEP_FORM_FIELDS              # of a `form` answer: the geometry, the switches and the launch form


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    run = form_probe(tmp_path_factory)

    def one_or_all(*cases):
        res = [{k: r[k] for k in FIELDS} if c.startswith("form ") else r for c, r in zip(cases, run(*cases))]
        return res if len(res) > 1 else res[0]
    return one_or_all


def form(spec, **kw):
    if "prec" in kw:
        kw["prec"] = native.DC_PREC[kw["prec"]]
    return "form " + spec + "".join(f" {k}={v}" for k, v in kw.items())


def test_wide_batches(probe):
    f = probe(form(BASE))
    assert f["stride"] == 1824 and f["wgr"] and not f["narrow"] and f["aligned"] and f["nwg"] == 256 and not f["error"]
    assert f["embed_next"] and f["fuse_embed"] and f["folded"] and f["g1_tiles"]
    f = probe(form(BASE, embedded=1))                 # the step after it: its front work is done
    assert not f["fuse_embed"] and not f["fuse_extra"] and not f["error"]
    f = probe(form("B=35 Tx=1800"))                   # aligned would be 280 workgroups = 2 rounds
    assert f["stride"] == 1824 and f["wgr"] and not f["narrow"] and not f["aligned"] and f["nwg"] == 250
    f = probe(form("B=36 Tx=1800"))                   # padding would cost a round: 257 against 254 workgroups
    assert f["stride"] == 1800 and not f["aligned"] and f["nwg"] == 254
    f = probe(form("B=18 Tx=1800"))
    assert f["stride"] == 1824 and f["wgr"] and not f["narrow"] and f["aligned"] and f["nwg"] == 144
    f = probe(form("B=128 Tx=900"))
    assert f["stride"] == 900 and f["wgr"] and not f["aligned"]


@pytest.mark.parametrize("B,nwg", [(17, 255), (9, 135)])
def test_narrow_batches(probe, B, nwg):
    f = probe(form(f"B={B} Tx=1800"))
    assert f["narrow"] and f["aligned"] and f["nwg"] == nwg and not f["layer16"] and f["fuse_extra"] and not f["fuse_embed"]


@pytest.mark.parametrize("B", [8, 1])
def test_layer16_batches(probe, B):
    f = probe(form(f"B={B} Tx=1800"))
    assert f["layer16"] and f["upc16"] == 29 and f["l16_shared"] and f["narrow"]
    f = probe(form(f"B={B} Tx=1800", env="DC_NO_LAYER16"))
    assert f["narrow"] and not f["layer16"] and not f["l16_shared"]
    for own in ({"env": "DC_L16_OWN_COMBINE"}, {"l16_own": 1}):
        f = probe(form(f"B={B} Tx=1800", **own))
        assert f["layer16"] and not f["l16_shared"]


def test_other_precisions_and_attention(probe):
    f = probe(form(BASE, prec="mixed"))
    assert f["stride"] == 1824 and f["ss"] and f["aligned"] and f["nwg"] == 256 and not f["narrow"] and f["mixed_form"]
    f = probe(form(BASE, no_eff=1))
    assert f["stride"] == 1800 and not (f["wgr"] or f["narrow"] or f["layer16"] or f["folded"])
    f, g = probe(form("B=39 Tx=20"), form("B=5 Tx=36"))
    assert (f["stride"], g["stride"]) == (32, 36) and not f["wgr"] and not g["wgr"]


@pytest.mark.parametrize("case", [BASE, "B=35 Tx=1800 loop=1 next_plain=1 g1_loop=1", "B=17 Tx=1800", "B=8 Tx=1800", "B=1 Tx=1800",
                                  "B=128 Tx=900 loop=1 next_plain=1 g1_loop=1", BASE + " prec=1"])
@pytest.mark.parametrize("hook", ["layers=3", "stage=2", "first=1"])
def test_hooks_keep_the_plain_forms(probe, case, hook):
    f = probe("form " + case + " " + hook)
    assert not (f["narrow"] or f["layer16"] or f["fuse_embed"] or f["fuse_extra"] or f["g1_tiles"] or f["embed_next"]), f


# switch -> the fields it changes on the base case (everything the named decision feeds), and their new values
SWITCHES = {
    "DC_NO_WGREC": dict(wgr=0, aligned=0, upc=0, nwg=228, rec_stride=0, embed_next=0, fuse_embed=0, g1_tiles=0, upd_flags=0),
    "DC_FLAT_UNITS": dict(aligned=0, upc=0, nwg=228, rec_stride=228 * 2 * 2304),
    "DC_ALIGN": dict(),                 # 32 x 1800 runs aligned units already (the rule: one round either way)
    "DC_NO_ALIGN": dict(aligned=0, upc=0, nwg=228, rec_stride=228 * 2 * 2304),
    "DC_NO_PAD": dict(stride=1800, aligned=0, upc=0, upc_narrow=15, nwg=225, rec_stride=225 * 2 * 2304),
    "DC_NO_FUSE_EMBED": dict(fuse_embed=0),
    "DC_NO_EMBED_NEXT": dict(embed_next=0, upd_flags=0),
    "DC_BEGIN_STEP": dict(folded=0),
}


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_each_switch_changes_its_field_and_the_graph_key(probe, name):
    base, f = probe(form(BASE), form(BASE, env=name))
    assert base["bits"] == 0 and f["bits"] != 0
    changed = {k: v for k, v in f.items() if v != base[k] and k != "bits"}
    want = {k: v for k, v in SWITCHES[name].items() if base[k] != v}
    assert changed == want


def test_align_switch_where_the_rule_says_flat(probe):
    base, f = probe(form("B=35 Tx=1800"), form("B=35 Tx=1800", env="DC_ALIGN"))
    assert not base["aligned"] and f["aligned"] and f["nwg"] == 280


def test_all_switch_bits_differ(probe):
    names = ["DC_NO_WGREC", "DC_NO_NARROW", "DC_NO_ALIGN", "DC_ALIGN", "DC_NO_FUSE_EMBED", "DC_FILM_STATIC", "DC_BEGIN_STEP", "DC_NO_PAD",
             "DC_NO_LAYER16", "DC_L16_OWN_COMBINE", "DC_L16_TEST_DROP_SLICE", "DC_TAIL_FILM_BF16", "DC_FLAT_UNITS", "DC_NO_EMBED_NEXT"]
    bits = [f["bits"] for f in probe(*[form(BASE, env=n) for n in names])]
    assert sorted(bits) == [1 << i for i in range(14)]


def tail(**kw):
    if "prec" in kw:
        kw["prec"] = native.DC_PREC[kw["prec"]]
    return "tail" + "".join(f" {k}={v}" for k, v in kw.items())


def test_loop_tail(probe):
    t = lambda **kw: probe(tail(**kw))
    assert t(prec="fp16", S=50) == {"tail": 1, "tail_all": 0}
    assert t(prec="bf16", S=50, Tx=1800) == {"tail": 6, "tail_all": 0}
    assert t(prec="bf16", S=50, Tx=99) == {"tail": 50, "tail_all": 1}         # short clips: every evaluation split
    assert t(prec="bf16", S=50, Tx=100) == {"tail": 6, "tail_all": 0}
    assert t(prec="fp16", S=50, flags=native.UPDATE_EPSILON) == {"tail": 50, "tail_all": 1}
    assert t(prec="fp16", S=1000, flags=native.UPDATE_EPSILON) == {"tail": 50, "tail_all": 1}
    assert t(prec="fp16", S=50, override=4) == {"tail": 4, "tail_all": 0}
    assert t(prec="fp16", S=50, flags=native.UPDATE_EPSILON, override=4) == {"tail": 4, "tail_all": 0}
    assert t(prec="fp16", S=50, tail_split=3) == {"tail": 3, "tail_all": 0}
    assert t(prec="fp16", S=1000, tail_split=60) == {"tail": 50, "tail_all": 0}      # clipped to the last graph's 50 steps
    assert t(prec="bf16", S=1000, Tx=1800) == {"tail": 6, "tail_all": 0}
    assert t(prec="fp16", S=50, split_model=0)["tail"] == 0
    assert t(prec="mixed", S=50)["tail"] == 0 and t(prec="bf16x3", S=50, override=4)["tail"] == 0


def test_steps_per_graph(probe):
    assert [r["steps_per_graph"] for r in probe("spg S=50", "spg S=1000", "spg S=67", "spg S=64", "spg S=128")] == [50, 50, 1, 64, 64]


# ---- the loop's plan (loop_plan, loop_step): B=1 Tx=1800 unless said; a part is (steps, split_n, launches) ---------------------------
KEY_G1, KEY_TAIL_SHIFT, KEY_SHARED = 1 << 39, 40, 1 << 28          # dc_form.h, GraphKey
ALL_SWITCHES = ["DC_NO_WGREC", "DC_NO_NARROW", "DC_NO_ALIGN", "DC_ALIGN", "DC_NO_FUSE_EMBED", "DC_FILM_STATIC", "DC_BEGIN_STEP", "DC_NO_PAD",
                "DC_NO_LAYER16", "DC_L16_OWN_COMBINE", "DC_L16_TEST_DROP_SLICE", "DC_TAIL_FILM_BF16", "DC_FLAT_UNITS", "DC_NO_EMBED_NEXT",
                "DC_GUIDE_FULL_FILM", "DC_TAKES_FULL_FILM"]          # DC_FORM_SWITCHES, in the list's order


def plan(spec="", **kw):
    if "prec" in kw:
        kw["prec"] = native.DC_PREC[kw["prec"]]
    return "plan " + spec + "".join(f" {k}={v}" for k, v in kw.items())


def parts(p):
    return [(q["steps"], q["split_n"], q["launches"]) for q in p["parts"]]


def keys(p):
    return [tuple(q["key"]) for q in p["parts"]]


def test_loop_plan_parts(probe):
    P = lambda **kw: probe(plan(**kw))
    for p, want in ((P(S=50), [(50, 1, 1)]), (P(S=1), [(1, 1, 1)]), (P(S=50, prec="bf16", Tx=1800), [(50, 6, 1)]),
                    (P(S=50, prec="bf16", Tx=99), [(50, 50, 1)]), (P(S=128), [(64, 0, 1), (64, 1, 1)]), (P(S=67), [(1, 0, 66), (1, 1, 1)])):
        assert parts(p) == want and p["g1_loop"] == 1 and p["eager"] == 0 and all(k[4] & KEY_G1 for k in keys(p)), p
        assert all((k[0], k[3]) == (1, want[0][0]) for k in keys(p)), p          # (clips, steps per graph)
    # no tail: one part however many replays, and the g1 bit clear
    for p, want in ((P(S=50, tail_split=0), [(50, 0, 1)]), (P(S=50, prec="mixed"), [(50, 0, 1)]), (P(S=1000, prec="mixed"), [(50, 0, 20)])):
        assert parts(p) == want and p["g1_loop"] == 0 and p["eager"] == 0 and keys(p)[0][4] & KEY_G1 == 0, p
        assert keys(p)[0][4] >> KEY_TAIL_SHIFT == 0
    # S > 64 with a tail: the last replay runs a second graph; the two keys differ in the tail field only, and both carry the g1 bit
    p = P(S=1000)
    (a, b) = keys(p)
    assert parts(p) == [(50, 0, 19), (50, 1, 1)] and a[:4] == b[:4] and a[5] == b[5] and a[4] & KEY_G1 and b[4] & KEY_G1
    assert a[4] ^ b[4] == 1 << KEY_TAIL_SHIFT and a[4] >> KEY_TAIL_SHIFT == 0
    assert b == keys(P(S=50))[0]                                     # the last 50 steps ARE the 50-step loop's graph
    # an EPSILON loop splits every evaluation: two parts of one key, i.e. one capture
    p = P(S=1000, flags=native.UPDATE_EPSILON)
    assert parts(p) == [(50, 50, 19), (50, 50, 1)] and keys(p)[0] == keys(p)[1] and keys(p)[0][4] >> KEY_TAIL_SHIFT == 50
    # eager loops: one part over the whole loop, no key
    for kw in (dict(profile=1), dict(no_graph=1)):
        p = P(S=1000, **kw)
        assert p["eager"] == 1 and p["g1_loop"] == 1 and parts(p) == [(1000, 1, 1)] and keys(p) == [(0,) * 6]
    p = P(S=1000, flags=native.UPDATE_EPSILON, no_graph=1)
    assert p["eager"] == 1 and parts(p) == [(1000, 1000, 1)]


def test_loop_plan_key(probe):
    """Everything a captured graph bakes in changes the key the library builds - and nothing else does."""
    key = lambda spec="", **kw: keys(probe(plan(spec, S=50, **kw)))[0]
    base = key()
    assert base == key() == (1, 1824, 1800, 50, KEY_G1 | 1 << KEY_TAIL_SHIFT, 0)
    switched = [key(env=n) for n in ALL_SWITCHES]
    assert len(set(switched + [base])) == len(ALL_SWITCHES) + 1
    for i, (n, k) in enumerate(zip(ALL_SWITCHES, switched)):
        assert k[4] ^ base[4] == 1 << i, n                           # one bit per switch, in the list's order
        assert (k[:4] == base[:4]) == (n != "DC_NO_PAD") and k[5] == base[5]         # (DC_NO_PAD changes the stride as well)
    assert key(flags=native.UPDATE_CLIP_DENOISED)[4] ^ base[4] == native.UPDATE_CLIP_DENOISED << 16
    assert key(l16_own=1)[4] ^ base[4] == 1 << 24
    assert [key(clip_aligned=m)[4] >> 25 & 3 for m in (-1, 0, 1)] == [0, 1, 2] and key(clip_aligned=-1) == base
    plain, guided, full = key("B=4 Tx=96"), key("B=4 Tx=96 guided=1"), key("B=4 Tx=96 guided=1", env="DC_GUIDE_FULL_FILM")
    assert len({plain, guided, full}) == 3 and plain[:4] == guided[:4] == full[:4]
    assert guided[4] ^ plain[4] == 1 << 27 | KEY_SHARED and guided[4] & KEY_SHARED and not full[4] & KEY_SHARED and full[4] & 1 << 27
    a, b, c = key("musics=2 takes=2 Tx=256"), key("musics=4 takes=1 Tx=256"), key("musics=1 takes=4 Tx=256")
    assert a[:5] == b[:5] == c[:5] and (a[5], b[5], c[5]) == (16, 0, 8)              # one geometry, three periods
    # the g1 bit: the plain 50-step graph of a 1000-step loop with a tail against the same graph of a loop without one
    with_tail, without = keys(probe(plan(S=1000)))[0], keys(probe(plan(S=1000, tail_split=0)))[0]
    assert with_tail[4] ^ without[4] == KEY_G1
    # the tail field: the last graph of a 1000-step loop with a tail of 1 and of 2, against its plain graph
    one, two = keys(probe(plan(S=1000, tail_split=1)))[1], keys(probe(plan(S=1000, tail_split=2)))[1]
    assert [k[4] >> KEY_TAIL_SHIFT for k in (with_tail, one, two)] == [0, 1, 2] and one[4] ^ two[4] == 3 << KEY_TAIL_SHIFT
    assert one[4] ^ with_tail[4] == 1 << KEY_TAIL_SHIFT
    # not in the key: the loop's length beyond its steps per graph, the compute units
    assert keys(probe(plan(S=100)))[1] == base and key(num_cu=304) == base


def test_loop_step_options(probe):
    """The steps of the part (50, 6, 1) - bf16, 1800 frames: split exactly from step 44, a plain successor exactly before step 43."""
    steps = probe(*[plan(S=50, prec="bf16", Tx=1800, part=0, step=i) for i in range(50)])
    for i, o in enumerate(steps):
        assert (o["split"], o["next_plain"], o["graph_step"]) == (int(i >= 44), int(i < 43), i), (i, o)
        assert o["loop_mode"] == 1 and o["g1_loop"] == 1 and o["embedded"] == 0 and (o["known"], o["guided"], o["takes"]) == (0, 0, 1)
    eager = probe(plan(S=50, prec="bf16", Tx=1800, no_graph=1, part=0, step=44), plan(S=50, prec="bf16", Tx=1800, profile=1, part=0, step=43))
    assert [(o["graph_step"], o["split"], o["next_plain"], o["profile"]) for o in eager] == [(-1, 1, 0, 0), (-1, 0, 0, 1)]
    o = probe(plan("musics=2 takes=2 Tx=256 guided=1", S=50, flags=64, part=0, step=0))          # DC_UPD_KNOWN
    assert (o["known"], o["guided"], o["takes"], o["split"], o["next_plain"]) == (1, 1, 2, 0, 1)
