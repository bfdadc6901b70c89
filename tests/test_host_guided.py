"""Classifier-free guidance, the host half (no GPU): the checker of the GPU tests (helpers_guided.ddim_guided_loop) against the oracle's
own loop, and the launch rule with StepOpts::guided (csrc/dc_form.h through tests/form_probe.cpp) for the internal shapes of
tests/test_gpu_guided.py."""
import pytest
import torch

from helpers import GUIDED_FIELDS, O, batch_noise, loop_step_probe, oracle_params, rel_l2, xf_pair
from helpers_guided import ddim_guided_loop, null_pair

UPD_EMBED_NEXT = 32          # dc_common.h
KEY_GUIDED, KEY_SHARED = 1 << 27, 1 << 28          # dc_form.h, guided_key_bits


@pytest.fixture(scope="module")
def loops():
    """2 x 96, S = 25, seeded features: the unguided oracle loop and the checker at w = 1, 2, 3 (computed once)."""
    B, T, S = 2, 96, 25
    p, (xfp, xfo) = oracle_params(), xf_pair(B, T, first=60)
    x = torch.from_numpy(batch_noise(B, T, first=60))
    length = [96, 70]
    with torch.no_grad():
        ref = O.ddim_sample_loop(p, x, xfp, xfo, length, S, idxs=(0, 3))
    return ref, {w: ddim_guided_loop(p, x, xfp, xfo, length, S, w, idxs=(0, 3)) for w in (1.0, 2.0)}, S


def test_checker_at_scale_one_is_the_oracle_loop(loops):
    ref, got, S = loops
    for k in (0, 3, S):
        assert torch.isfinite(got[1.0][k]).all() and torch.equal(got[1.0][k], ref[k])


def test_guidance_moves_the_sample(loops):
    """Keeps the GPU tests from being vacuous: at w = 2 every clip differs from the unguided loop by rel-L2 >= 0.1 (measured 0.62
    and 0.53 at 2 x 96, S = 25, these seeded features)."""
    ref, got, S = loops
    for b in range(2):
        e = rel_l2(got[2.0][S][b], ref[S][b])
        print(f"w = 2 against unguided, clip {b}: {e:.3f}")
        assert e >= 0.1, (b, e)


def test_null_pair():
    p = oracle_params()
    npj, nout = null_pair(p)
    assert torch.equal(npj, torch.nn.functional.linear(torch.zeros(64), p["proj.weight"], p["proj.bias"])) and not nout.any()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return loop_step_probe(tmp_path_factory, GUIDED_FIELDS)


# the INTERNAL shapes (B = 2 x the caller's clips) of tests/test_gpu_guided.py, the form each is there for (256 compute units, fp16
# unless said) and the groups the FiLM GEMM covers: Gc + 1 where the conditional half is Gc whole groups, else all G
FORMS = [("B=2 Tx=256", dict(layer16=1, narrow=1), 9),                                        # 1 x 256
         ("B=72 Tx=256", dict(layer16=0, narrow=1, aligned=1), 289),                          # 36 x 256
         ("B=160 Tx=256", dict(narrow=0, wgr=1, aligned=1, embed_next=1), 641),               # 80 x 256
         ("B=110 Tx=300", dict(narrow=0, wgr=1, aligned=0, embed_next=1, stride=300), None),  # 55 x 300: 16500 tokens, no whole groups
         ("B=4 Tx=96", dict(wgr=0, layer16=0), 7),                                            # 2 x 96
         ("B=6 Tx=20", dict(wgr=0, layer16=0, stride=32), 4),                                 # 3 x 20
         ("B=4 Tx=96 no_eff=1", dict(wgr=0, folded=0), 7),                                    # no_eff 2 x 96
         ("B=6 Tx=35 no_eff=1", dict(wgr=0, folded=0, stride=35), None),                      # no_eff, odd T: 105 tokens per half
         ("B=2 Tx=256 prec=0", dict(layer16=1, fs=0, ff=0), 9),                               # bf16 1 x 256
         ("B=2 Tx=256 prec=1", dict(ss=1, mixed_form=1, wgr=1, aligned=1), 9),                # mixed 1 x 256
         ("B=2 Tx=256 prec=2", dict(ss=1, fuse_silu=0), None),                                # bf16x3: the GEMM reads the S images, all groups
         ("B=2 Tx=256 split=1 next_plain=0", dict(ss=1, layer16=0, narrow=0, wgr=1, aligned=1), 9),      # the precise tail's evaluation
         ("B=2 Tx=256 split=1 next_plain=0 prec=0", dict(ss=1, film_tail=1, wgr=1), 9),
         ("B=64 Tx=1800", dict(narrow=0, wgr=1, aligned=1, embed_next=1, stride=1824), 1825), # 32 x 1800, padded stride
         ("B=2 Tx=300", dict(layer16=1, stride=320), 11),                                     # 1 x 300, padded stride: padding lanes read the null column
         ("B=2 Tx=255", dict(wgr=0, layer16=0, stride=255), None),                            # 1 x 255: 6630 elements, no multiple of 4, no whole groups
         ("B=2 Tx=1800", dict(layer16=1, stride=1824), 58)]                                   # 1 x 1800, padded stride
GIVEN_UP = ("embed_next", "fuse_embed", "fuse_extra", "upd_flags", "guided", "shared_film", "film_groups", "key_bits")


@pytest.mark.parametrize("case,want,groups", FORMS, ids=[c for c, _, _ in FORMS])
def test_guided_bit_gives_up_embed_next_and_the_named_forms_only(probe, case, want, groups):
    base, f, full = probe(case, case + " guided=1", case + " guided=1 env=DC_GUIDE_FULL_FILM")
    assert not base["error"] and not f["error"] and not full["error"], (base, f, full)
    assert {k: base[k] for k in want} == want, base
    G = base["G"]
    assert base["guided"] == 0 and base["film_groups"] == G and base["shared_film"] == 0 and base["key_bits"] == 0
    # the shared-column rule, shared or full, per (B, T')
    shared = groups is not None
    assert f["guided"] == 1 and f["film_groups"] == (groups if shared else G) and f["shared_film"] == int(shared), f
    if shared:
        assert G % 2 == 0 and G // 2 + 1 == groups          # Gc + 1: the conditional half is Gc = G / 2 whole groups
    assert full["guided"] == 1 and full["film_groups"] == G and full["shared_film"] == 0
    # the guided bit and the shared-column bit are in the graph key; the switch is in the switches' bits
    assert f["key_bits"] == KEY_GUIDED | (KEY_SHARED if shared else 0) and full["key_bits"] == KEY_GUIDED
    assert full["switch_bits"] != f["switch_bits"] and f["switch_bits"] == base["switch_bits"]
    # given up: embed_next always; fuse_embed / fuse_extra exactly where the GEMM covers fewer groups than the layers
    for g in (f, full):
        assert g["embed_next"] == 0 and g["upd_flags"] == base["upd_flags"] & ~UPD_EMBED_NEXT
        keep = 0 if g["shared_film"] else 1
        assert g["fuse_embed"] == base["fuse_embed"] * keep and g["fuse_extra"] == base["fuse_extra"] * keep
        # ... and no other launch-form field changes
        assert {k: v for k, v in g.items() if k not in GIVEN_UP + ("switch_bits",)} == \
            {k: v for k, v in base.items() if k not in GIVEN_UP + ("switch_bits",)}
    if want.get("embed_next"):
        assert base["upd_flags"] & UPD_EMBED_NEXT


def test_guided_profile_pass_and_known(probe):
    """The profile pass keeps its separate launches either way; known values add their update bit to a guided step as to any other."""
    base, prof, kn = probe("B=160 Tx=256 guided=1", "B=160 Tx=256 guided=1 profile=1", "B=160 Tx=256 guided=1 known=1")
    assert prof["fuse_embed"] == 0 and base["fuse_embed"] == 0 and prof["film_groups"] == base["film_groups"] == 641
    assert kn["upd_flags"] == base["upd_flags"] | 64
    odd, = probe("B=3 Tx=256 guided=1")
    assert "even" in odd["error"]
