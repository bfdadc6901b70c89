"""Host rules of the padding waves' barrier-only path (csrc/dc_form.h: Settings::idle_wave_path -> StepForm::idle_path and bit 29 of a
captured graph's key), through tests/idle_form_probe.cpp on the CPU.  The GPU side: tests/test_gpu_idle_waves.py."""
import json
import os
import shutil
import subprocess

import pytest

from helpers import ROOT


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    from diffusion_conductor_amd import native
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("idle") / "idle_form_probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", native.CSRC, os.path.join(ROOT, "tests", "idle_form_probe.cpp"), "-o", exe], check=True)

    def run(*cases):
        env = {k: v for k, v in os.environ.items() if not k.startswith("DC_")}
        out = subprocess.run([exe], input="\n".join(cases) + "\n", env=env, check=True, capture_output=True, text=True).stdout
        res = [json.loads(ln) for ln in out.splitlines()]
        assert len(res) == len(cases)
        return res
    return run


def test_the_path_is_on_by_default_in_the_wide_plain_form_only(probe):
    head, flat, off, small, wide_small, split, mixed, hook, stamps, per_group = probe(
        "B=32 Tx=1800", "B=32 Tx=1800 env=DC_FLAT_UNITS", "B=32 Tx=1800 idle=0", "B=3 Tx=264", "B=3 Tx=264 env=DC_NO_NARROW",
        "B=32 Tx=1800 split=1", "B=32 Tx=1800 prec=1", "B=32 Tx=1800 layers=3", "B=32 Tx=1800 stamps=1", "B=32 Tx=1800 env=DC_NO_WGREC")
    assert all(r["error"] == "" and r["default_on"] == 1 for r in (head, flat, off, small, wide_small, split, mixed, hook, stamps, per_group))
    # the headline: clip-aligned 8-wave units, 8 workgroups per clip - and its flat-unit form (the last workgroup's tail waves)
    assert head["idle_path"] == 1 and head["wgr"] == 1 and head["narrow"] == 0 and head["aligned"] == 1 and head["upc"] == 8
    assert flat["idle_path"] == 1 and flat["aligned"] == 0
    assert off["idle_path"] == 0 and {k: v for k, v in off.items() if k not in ("idle_path", "key_bits")} == \
        {k: v for k, v in head.items() if k not in ("idle_path", "key_bits")}
    # the wide form at a small batch (the GPU tests' shapes); the narrow form, split operands, hooks, stamps, per-group records: no such path
    assert wide_small["idle_path"] == 1 and wide_small["upc"] == 2
    assert small["narrow"] == 1 and small["idle_path"] == 0
    assert split["ss"] == 1 and split["idle_path"] == 0 and mixed["ss"] == 1 and mixed["idle_path"] == 0
    assert hook["idle_path"] == 0 and stamps["idle_path"] == 0
    assert per_group["wgr"] == 0 and per_group["idle_path"] == 0


def test_the_setting_has_its_own_key_bit_and_the_default_key_is_unchanged(probe):
    on, off = probe("B=32 Tx=1800", "B=32 Tx=1800 idle=0")
    assert on["key_bits"] >> 29 & 1 == 0                   # (the bit says OFF: every key captured with the default is what it was)
    assert off["key_bits"] == on["key_bits"] | 1 << 29     # a change re-captures, and changes nothing else of the key
