"""Several takes per music, the host half (no GPU): the period / group rule of the shared FiLM GEMM (film_share, csrc/dc_form.h), the
launch form of every shape of tests/test_gpu_takes.py, the graph key, and takes = 1 against the rule as it was - through
tests/form_probe.cpp; takes = 1 also as the tests of guidance ask it, by the internal batch and for the fields recorded from the rule
before takes existed."""
import json
import os

import pytest

from helpers import GUIDED_FIELDS, ROOT, TAKES_FIELDS, loop_step_probe

UPD_EMBED_NEXT = 32          # dc_common.h
KEY_GUIDED, KEY_SHARED = 1 << 27, 1 << 28          # dc_form.h, guided_key_bits


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return loop_step_probe(tmp_path_factory, TAKES_FIELDS)


@pytest.fixture(scope="module")
def guided_probe(tmp_path_factory):
    return loop_step_probe(tmp_path_factory, GUIDED_FIELDS)


# (musics, takes, Tx, extra) of tests/test_gpu_takes.py, the form each is there for (256 compute units, fp16 unless said) and the period
# Gc = musics x stride / 32 the tile reads wrap at - None: one take is no whole number of groups (or the GEMM reads the S images), the
# GEMM covers every group
FORMS = [("layer16", 1, 2, 256, "", dict(layer16=1, narrow=1, stride=256), 8),
         ("narrow", 18, 4, 256, "", dict(layer16=0, narrow=1, aligned=1), 144),
         ("wide_aligned", 40, 4, 256, "", dict(narrow=0, wgr=1, aligned=1, embed_next=1), 320),
         ("wide_flat", 56, 2, 300, "", dict(narrow=0, wgr=1, aligned=0, embed_next=1, stride=300, nwg=132), 525),
         ("group_96", 2, 2, 96, "", dict(wgr=0, layer16=0, stride=96), 6),
         ("group_20", 3, 2, 20, "", dict(wgr=0, layer16=0, stride=32), 3),
         ("padded_300", 1, 3, 300, "", dict(layer16=1, stride=320), 10),
         ("odd_255", 1, 2, 255, "", dict(wgr=0, layer16=0, stride=255), None),
         ("no_eff", 2, 2, 96, " no_eff=1", dict(wgr=0, folded=0), 6),
         ("bf16", 1, 2, 256, " prec=0", dict(layer16=1, fs=0, ff=0), 8),
         ("mixed", 1, 2, 256, " prec=1", dict(ss=1, mixed_form=1, wgr=1, aligned=1), 8),
         ("bf16x3", 1, 2, 256, " prec=2", dict(ss=1, fuse_silu=0), None),
         ("tail", 1, 2, 256, " split=1 next_plain=0", dict(ss=1, layer16=0, narrow=0, wgr=1, aligned=1), 8),
         ("headline_8x4", 8, 4, 1800, "", dict(narrow=0, wgr=1, aligned=1, embed_next=1, stride=1824, nwg=256), 456)]
SHARE_FIELDS = ("fuse_embed", "fuse_extra", "shared_film", "film_groups", "film_period", "film_wrap", "key_period", "share_period",
                "share_wrap", "share_groups", "switch_bits")


@pytest.mark.parametrize("name,musics,takes,Tx,extra,want,period", FORMS, ids=[f[0] for f in FORMS])
def test_period_groups_and_form(probe, name, musics, takes, Tx, extra, want, period):
    tiled, f, full = probe(f"musics={musics * takes} takes=1 Tx={Tx}{extra}", f"musics={musics} takes={takes} Tx={Tx}{extra}",
                           f"musics={musics} takes={takes} Tx={Tx}{extra} env=DC_TAKES_FULL_FILM")
    assert not tiled["error"] and not f["error"] and not full["error"], (tiled, f, full)
    assert {k: f[k] for k in want} == want, f
    G = f["G"]
    assert tiled["G"] == G and tiled["B"] == f["B"] == musics * takes and tiled["stride"] == f["stride"]      # one internal geometry
    # nothing shared: the plain conditioning of the tiled music, and the switch
    for g in (tiled, full):
        assert (g["film_groups"], g["film_period"], g["film_wrap"], g["shared_film"], g["key_period"]) == (G, G, G, 0, 0), g
    shared = period is not None
    if shared:
        assert period == musics * f["stride"] // 32 and period * takes == G
        assert (f["film_groups"], f["film_period"], f["film_wrap"], f["shared_film"]) == (period, period, G, 1), f
        assert f["key_period"] == period          # the captured graph of the takes is not the tiled conditioning's
    else:
        assert (f["film_groups"], f["film_period"], f["film_wrap"], f["shared_film"], f["key_period"]) == (G, G, G, 0, 0), f
    assert (f["share_period"], f["share_wrap"], f["share_groups"]) == (f["film_period"], f["film_wrap"], f["film_groups"])
    assert f["key_bits"] == tiled["key_bits"] == 0
    assert full["switch_bits"] != f["switch_bits"] and f["switch_bits"] == tiled["switch_bits"]
    # given up: fuse_embed / fuse_extra exactly where the GEMM covers fewer groups than the layers; embed_next stays
    keep = 0 if shared else 1
    assert f["fuse_embed"] == tiled["fuse_embed"] * keep and f["fuse_extra"] == tiled["fuse_extra"] * keep
    assert f["embed_next"] == tiled["embed_next"] and f["upd_flags"] == tiled["upd_flags"]
    if want.get("embed_next"):
        assert f["upd_flags"] & UPD_EMBED_NEXT
    # ... and no other launch-form field changes
    for g in (f, full):
        assert {k: v for k, v in g.items() if k not in SHARE_FIELDS} == {k: v for k, v in tiled.items() if k not in SHARE_FIELDS}


def test_embedded_step_keeps_its_form(probe):
    """An embedded step of unguided takes (its front work done by the previous step's last layer): the FiLM launch is the bare GEMM
    with or without the shared tiles."""
    tiled, f = probe("musics=160 takes=1 Tx=256 embedded=1", "musics=40 takes=4 Tx=256 embedded=1")
    assert not f["error"] and f["fuse_embed"] == tiled["fuse_embed"] == 0 and f["embed_next"] == tiled["embed_next"] == 1
    assert f["film_groups"] == 320 and tiled["film_groups"] == 1280


GUIDED = [(2, 2, 256, 16, 32), (1, 3, 300, 10, 30), (36, 2, 256, 288, 576), (2, 2, 96, 6, 12), (1, 2, 255, None, None)]


@pytest.mark.parametrize("musics,takes,Tx,period,wrap", GUIDED)
def test_guided_takes(probe, musics, takes, Tx, period, wrap):
    """Guided: one take's groups and one more, the null column; DC_TAKES_FULL_FILM keeps the guided rule over the tiled clips,
    DC_GUIDE_FULL_FILM every group."""
    c = f"musics={musics} takes={takes} Tx={Tx} guided=1"
    f, tfull, gfull, tiled = probe(c, c + " env=DC_TAKES_FULL_FILM", c + " env=DC_GUIDE_FULL_FILM", f"musics={musics * takes} takes=1 Tx={Tx} guided=1")
    G = f["G"]
    assert not f["error"] and f["embed_next"] == 0 and f["guided"] == 1
    assert (gfull["film_groups"], gfull["film_period"], gfull["film_wrap"], gfull["key_period"]) == (G, G, G, 0)
    assert gfull["key_bits"] == KEY_GUIDED
    if period is None:
        assert (f["film_groups"], f["film_period"], f["film_wrap"], f["key_period"], f["key_bits"]) == (G, G, G, 0, KEY_GUIDED)
        return
    assert 2 * wrap == G and period * takes == wrap
    assert (f["film_groups"], f["film_period"], f["film_wrap"], f["key_period"]) == (period + 1, period, wrap, period)
    assert f["key_bits"] == KEY_GUIDED | KEY_SHARED and f["fuse_embed"] == 0 and f["fuse_extra"] == 0
    for g in (tfull, tiled):      # the guided rule as it is without takes: the shadows' one column behind all conditional groups
        assert (g["film_groups"], g["film_period"], g["film_wrap"], g["key_period"]) == (wrap + 1, wrap, wrap, 0), g
        assert g["key_bits"] == KEY_GUIDED | KEY_SHARED


def test_graph_keys_of_equal_internal_geometries_differ(probe):
    """2 takes x 2 musics and a plain conditioning of 4 clips: one (B, T, G), the same switches and key bits - and another period in
    the key.  Likewise guided, and 2 x 2 against 4 x 1 ... against 1 x 4."""
    a, b, c = probe("musics=2 takes=2 Tx=256", "musics=4 takes=1 Tx=256", "musics=1 takes=4 Tx=256")
    assert (a["B"], a["stride"], a["G"], a["switch_bits"], a["key_bits"]) == (b["B"], b["stride"], b["G"], b["switch_bits"], b["key_bits"])
    assert len({a["key_period"], b["key_period"], c["key_period"]}) == 3 and b["key_period"] == 0
    ga, gb = probe("musics=2 takes=2 Tx=256 guided=1", "musics=4 takes=1 Tx=256 guided=1")
    assert (ga["B"], ga["G"], ga["key_bits"]) == (gb["B"], gb["G"], gb["key_bits"]) and ga["key_period"] != gb["key_period"]


ONE_TAKE = ["musics=1 Tx=256", "musics=36 Tx=256", "musics=80 Tx=256", "musics=55 Tx=300", "musics=2 Tx=96", "musics=3 Tx=20",
            "musics=2 Tx=96 no_eff=1", "musics=1 Tx=256 prec=0", "musics=1 Tx=256 prec=1", "musics=1 Tx=256 prec=2", "musics=32 Tx=1800",
            "musics=1 Tx=300", "musics=1 Tx=255", "musics=1 Tx=256 split=1 next_plain=0", "musics=80 Tx=256 known=1", "musics=80 Tx=256 profile=1"]


def _case_without_takes(case, guided):
    """The same case as the rule without takes was asked: by B, the internal batch."""
    head, _, rest = case.partition(" ")
    return f"B={int(head.split('=')[1]) * (2 if guided else 1)} {rest} guided={guided}".replace("  ", " ")


@pytest.fixture(scope="module")
def parent_forms():
    """What the probe of guidance printed (GUIDED_FIELDS) for the cases of ONE_TAKE on the rule as it was before takes existed
    (recorded once)."""
    with open(os.path.join(ROOT, "tests", "golden", "takes_one_take_forms.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("case", ONE_TAKE)
@pytest.mark.parametrize("guided", [0, 1])
def test_one_take_is_the_rule_without_takes(probe, guided_probe, parent_forms, case, guided):
    """takes = 1 (what dc_sampler_set_conditioning / _guided set): every StepForm field, the stride, the switches and the key bits as
    recorded from the rule before takes - field for field, through both probes - and the mapping's new fields at their single-take
    values: the conditional clips' groups, no period in the key."""
    want = parent_forms[f"{case} guided={guided}"]
    new, = probe(f"{case} takes=1 guided={guided}")
    old, = guided_probe(_case_without_takes(case, guided))
    assert old == want
    assert {k: new[k] for k in want} == want
    G = new["G"]
    shared = bool(guided and new["shared_film"])
    cond = G // 2 if shared else G
    assert (new["film_period"], new["film_wrap"], new["key_period"]) == (cond, cond, 0)
    assert new["film_groups"] == (cond + 1 if shared else G)


def test_bad_takes_are_refused(probe):
    a, b = probe("musics=1 takes=0 Tx=256", "musics=2 takes=2 Tx=256 guided=1 env=DC_TAKES_FULL_FILM,DC_GUIDE_FULL_FILM")
    assert "takes" in a["error"]
    assert not b["error"] and b["film_groups"] == b["G"]


def test_reciprocal_is_exact(probe):
    """The layer kernels take g / period from a reciprocal prepared on the host (film_magic): exact for every g below the wrap, for
    the periods of the GPU test shapes, the headline's, primes, and the largest (period, takes) the rule lets share."""
    cases = [(3, 2), (6, 2), (8, 2), (10, 3), (16, 2), (144, 4), (320, 4), (456, 4), (457, 7), (525, 2), (4093, 64), (46340, 2), (65535, 1)]
    for (p, k), r in zip(cases, probe(*[f"magic_period={p} magic_takes={k}" for p, k in cases])):
        assert r["wrong"] == 0 and r["checked"] == p * k and r["unshared"] == 0
        assert (r["magic"] != 0) == (k > 1)


def test_takes_of_one_group_and_of_very_many_do_not_wrap(probe):
    """A take of ONE group (a single clip of at most 32 frames) has no 32-bit reciprocal, and past wrap x period = 2^32 the reciprocal
    is no longer exact: the GEMM then covers every conditional group, as under DC_TAKES_FULL_FILM."""
    one, two, big, ok = probe("musics=1 takes=3 Tx=20", "musics=2 takes=3 Tx=20", "musics=200 takes=40 Tx=1800 num_cu=256",
                              "musics=100 takes=4 Tx=1800")
    assert one["stride"] == 32 and (one["film_period"], one["film_wrap"], one["film_groups"], one["key_period"]) == (3, 3, 3, 0)
    assert (two["film_period"], two["film_wrap"], two["film_groups"], two["key_period"]) == (2, 6, 2, 2)
    G = big["G"]
    assert not big["error"] and (G // 40) * G >= 2 ** 32 and (big["film_period"], big["film_groups"], big["key_period"]) == (G, G, 0)
    assert ok["shared_film"] == 1 and ok["film_period"] * 4 == ok["G"]
