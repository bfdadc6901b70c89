"""Sampling around known values, the host half (no GPU): the coefficient table of dc_ddim_coefficients_known, the launch rule with the
DC_UPD_KNOWN bit (csrc/dc_form.h through tests/form_probe.cpp), the window planner of generate_long_music_motion, and the
checker of the GPU tests (helpers_known.ddim_known_loop) against the oracle's own loop."""
import numpy as np
import pytest
import torch

from helpers import O, batch_noise, loop_step_probe, oracle_params, xf_pair
from helpers_known import ddim_known_loop, known_levels, prefix_mask

from diffusion_conductor_amd import native
from diffusion_conductor_amd.harness import LONG_OVERLAP, plan_windows

UPD_EMBED_NEXT, UPD_KNOWN = 32, 64          # dc_common.h


@pytest.mark.parametrize("S", [1, 21, 50, 1000])      # (the linear schedule needs S > 20: beta_end = 20 / S)
@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_known_coefficients(S, eta):
    ac = native.linear_beta_schedule(S)["alphas_cumprod"]
    ck, start = native.ddim_coefficients_known(ac, eta)
    ex, c4 = native.ddim_coefficients(ac, eta), native.ddim_coefficients(ac)
    assert ck.shape == (S, 8) and ck.dtype == np.float32
    assert np.array_equal(ck[:, :5].view(np.uint32), ex[:, :5].view(np.uint32))            # the _ex row, bit for bit
    assert np.array_equal(ck[:, 5].view(np.uint32), c4[:, 3].view(np.uint32))              # sqrtf(1 - abar_prev), column 3's rounding
    assert ck[0, 5] == 0.0 and ck[0, 2] == 1.0                                             # t = 0: the final sample IS `known`
    a = ac.astype(np.float32)
    assert np.array_equal(ck[:, 6], np.sqrt(a)) and np.array_equal(ck[:, 7], np.sqrt(np.float32(1) - a))
    assert np.array_equal(start, ck[S - 1, 6:8])
    assert abs(float(start[0]) - np.sqrt(ac[S - 1])) <= 1e-7 and abs(float(start[1]) - np.sqrt(1 - ac[S - 1])) <= 1e-7
    assert np.array_equal(ex[:, 5:], np.zeros((S, 3), np.float32))                         # dc_ddim_coefficients_ex is what it was
    lv, (a0, b0) = known_levels(S)                                                         # the checker's levels: the same to an ulp
    assert np.allclose(lv.numpy(), ck[:, [2, 5]], rtol=2e-7, atol=0) and np.allclose([a0, b0], start, rtol=2e-7)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return loop_step_probe(tmp_path_factory)


# the shapes of tests/test_gpu_known.py and the form each is there for (256 compute units, fp16 unless said)
FORMS = [("B=2 Tx=256", dict(layer16=1, narrow=1)),
         ("B=72 Tx=256", dict(layer16=0, narrow=1, aligned=1)),
         ("B=160 Tx=256", dict(narrow=0, wgr=1, aligned=1, embed_next=1)),
         ("B=110 Tx=300", dict(narrow=0, wgr=1, aligned=0, embed_next=1, stride=300)),      # (33 x 300 is padded to 320 and runs narrow aligned units)
         ("B=2 Tx=96", dict(wgr=0, layer16=0)),
         ("B=3 Tx=20", dict(wgr=0, layer16=0, stride=32)),
         ("B=2 Tx=96 no_eff=1", dict(wgr=0, folded=0)),
         ("B=2 Tx=256 split=1 next_plain=0", dict(ss=1, layer16=0, narrow=0, wgr=1, aligned=1)),
         ("B=2 Tx=256 split=1 next_plain=0 prec=0", dict(ss=1, film_tail=1, wgr=1)),
         ("B=32 Tx=1800", dict(narrow=0, wgr=1, aligned=1, embed_next=1, nwg=256)),
         ("B=1 Tx=1800", dict(layer16=1))]


@pytest.mark.parametrize("case,want", FORMS, ids=[c for c, _ in FORMS])
def test_known_bit_changes_upd_flags_only(probe, case, want):
    base, f = probe(case, case + " known=1")
    assert not base["error"] and {k: base[k] for k in want} == want, base
    assert base["upd_flags"] & UPD_KNOWN == 0 and f["upd_flags"] == base["upd_flags"] | UPD_KNOWN
    assert {k: v for k, v in f.items() if k != "upd_flags"} == {k: v for k, v in base.items() if k != "upd_flags"}
    if want.get("embed_next"):
        assert f["embed_next"] and f["upd_flags"] & UPD_EMBED_NEXT              # no launch form is given up


def _check_plan(L, T, overlap):
    plan = plan_windows(L, T, overlap)
    done = 0                                  # frames [0, done) are generated
    for k, (s, kn) in enumerate(plan):
        assert 0 <= s and s + T <= L                                          # every window has T frames inside the piece
        assert kn == (0 if k == 0 else done - s) and 0 <= kn < T              # its known prefix is exactly what earlier windows produced
        assert s <= done                                                      # no gap: the windows cover [0, L)
        if 0 < k < len(plan) - 1:
            assert s == k * (T - overlap) and kn == overlap
        done = s + T
    assert plan[0] == (0, 0) and done == L and plan[-1][0] == L - T           # the last window ends at L
    return plan


def test_window_planner():
    T, ov = 1800, LONG_OVERLAP
    assert 0 < ov < T
    assert _check_plan(T, T, ov) == [(0, 0)]
    assert _check_plan(T + 1, T, ov) == [(0, 0), (1, T - 1)]
    assert _check_plan(2 * T - ov, T, ov) == [(0, 0), (T - ov, ov)]
    assert _check_plan(2 * T - ov + 1, T, ov) == [(0, 0), (T - ov, ov), (T - ov + 1, T - 1)]
    ten = _check_plan(9 * (T - ov) + T - 7, T, ov)
    assert len(ten) == 10 and ten[-1][1] == ov + 7
    assert len(_check_plan(640, 256, 64)) == 3 and _check_plan(640, 256, 0)[-1] == (384, 128)
    for L in range(256, 1200, 37):
        _check_plan(L, 256, 100)
    with pytest.raises(ValueError):
        plan_windows(T - 1, T, ov)
    with pytest.raises(ValueError):
        plan_windows(2 * T, T, T)


def test_checker_without_known_is_the_oracle_loop():
    B, T, S = 2, 24, 21          # (S > 20: the linear schedule's beta_end is 20 / S)
    p, (xfp, xfo) = oracle_params(), xf_pair(B, T, first=3)
    x = torch.from_numpy(batch_noise(B, T, first=3))
    z = torch.from_numpy(batch_noise(S * B, T, first=50)).view(S, B, T, 26)
    length = [T, 17]
    assert torch.isfinite(ddim_known_loop(p, x, xfp, xfo, length, S)).all()
    for kw in (dict(), dict(eta=0.5, step_noise=z, clip_denoised=True), dict(eps_model=True)):
        with torch.no_grad():
            ref = O.ddim_sample_loop(p, x, xfp, xfo, length, S, idxs=(0, 3), **kw)
        got = ddim_known_loop(p, x, xfp, xfo, length, S, idxs=(0, 3), **kw)
        zero = ddim_known_loop(p, x, xfp, xfo, length, S, known=torch.ones(B, T, 26), mask=torch.zeros(B, T, 26), eps=x, idxs=(0, 3), **kw)
        for k in (0, 3, S):
            assert torch.equal(got[k], ref[k]) and torch.equal(zero[k], ref[k])


def test_checker_returns_known_exactly():
    B, T, S = 2, 24, 21          # (S > 20: the linear schedule's beta_end is 20 / S)
    p, (xfp, xfo) = oracle_params(), xf_pair(B, T, first=4)
    x = torch.from_numpy(batch_noise(B, T, first=4))
    known, eps = torch.from_numpy(batch_noise(B, T, first=8)) * 0.5, torch.from_numpy(batch_noise(B, T, first=12))
    mask = prefix_mask(B, T, 26, [13, T])
    mask[0, :, 3:5] = 1
    res = ddim_known_loop(p, x, xfp, xfo, [T, T], S, known=known, mask=mask, eps=eps, idxs=(2,))
    assert torch.isfinite(res[S]).all() and torch.isfinite(res[2]).all()
    assert torch.equal(res[S][mask != 0], known[mask != 0])
    lv, _ = known_levels(S)
    want = lv[S - 1 - 2, 0] * known + lv[S - 1 - 2, 1] * eps                  # iteration 2 runs timestep S - 3
    assert torch.equal(res[2][mask != 0], want[mask != 0])
    plain = ddim_known_loop(p, x, xfp, xfo, [T, T], S)
    assert not torch.allclose(res[S][0, 13:, 5:], plain[0, 13:, 5:], atol=1e-4)      # the unknown elements see the known ones
