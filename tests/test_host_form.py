"""The launch rule on the CPU: csrc/dc_form.h decides which form a denoiser evaluation takes (records, units, fusions, tiles), the
clip stride, the steps per graph and the precise tail - pure integer arithmetic, no HIP.  tests/form_probe.cpp includes the header,
is compiled with the host compiler and prints the decision for the cases below; the expectations are DESIGN.md sections 4.3 and 5
at 256 compute units (fp16, linear attention, 8 layers unless said)."""
import json
import os
import shutil
import subprocess

import pytest

from helpers import ROOT

from diffusion_conductor_amd import native

BASE = "B=32 Tx=1800 loop=1 graph_step=0 next_plain=1 g1_loop=1"     # a captured loop step with a plain successor, in a loop with a tail


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("form") / "form_probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", native.CSRC, os.path.join(ROOT, "tests", "form_probe.cpp"), "-o", exe], check=True)

    def run(*cases):
        env = {k: v for k, v in os.environ.items() if not k.startswith("DC_")}
        out = subprocess.run([exe], input="\n".join(cases) + "\n", env=env, check=True, capture_output=True, text=True).stdout
        res = [json.loads(ln) for ln in out.splitlines()]
        assert len(res) == len(cases)
        return res if len(res) > 1 else res[0]
    return run


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
