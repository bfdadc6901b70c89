"""Sampling a long piece's windows in one loop, the host half (no GPU): harness.window_weights, the checker of the GPU tests
(helpers_windows.ddim_windows_loop) against the oracle's own loop, the launch rule with StepOpts::windows (csrc/dc_form.h through
tests/form_probe_windows.cpp) for the internal shapes of tests/test_gpu_windows.py, and every plan dc_sampler_set_conditioning_windows
refuses (dc_windows_check: the host's check, before any launch)."""
import numpy as np
import pytest
import torch

from helpers import O, batch_noise, oracle_params, xf_pair
from helpers_windows import SHAPES, ddim_windows_loop, windows_probe

from diffusion_conductor_amd import native
from diffusion_conductor_amd.harness import plan_windows, window_weights

UPD_EMBED_NEXT = 32                                  # dc_common.h
KEY_GUIDED, KEY_SHARED, KEY_WINDOWS = 1 << 27, 1 << 28, 1 << 30          # dc_form.h: guided_key_bits, windows_key_bits
ULP = 2.0 ** -23


def _starts(L, T, overlap):
    return [s for s, _ in plan_windows(L, T, overlap)]


# ---- window_weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", ["tent", "uniform"])
@pytest.mark.parametrize("L,T,overlap", [(448, 256, 64), (600, 256, 128), (18000, 1800, 300), (447, 255, 63), (256, 256, 0), (512, 256, 0)])
def test_weights_sum_to_one_and_single_cover_is_exactly_one(L, T, overlap, blend):
    starts = _starts(L, T, overlap)
    w = window_weights(L, T, starts, blend)
    assert w.dtype == np.float32 and w.shape == (len(starts), T) and np.isfinite(w).all() and (w >= 0).all()
    total, cover = np.zeros(L, np.float64), np.zeros(L, np.int64)
    for k, s in enumerate(starts):
        total[s:s + T] += w[k].astype(np.float64)
        cover[s:s + T] += 1
    assert np.abs(total - 1.0).max() <= ULP                      # the fp64 sum, within one fp32 ulp at every frame
    assert cover.min() >= 1
    for k, s in enumerate(starts):
        single = cover[s:s + T] == 1
        assert (w[k][single] == np.float32(1.0)).all()           # exactly 1.0, not 1 - ulp
    native.windows_check(starts, w, T, L)                        # ... and the library accepts the plan


def test_tent_is_linear_across_a_two_cover_overlap():
    L, T, ov = 448, 256, 64
    starts = _starts(L, T, ov)
    assert starts == [0, 192]
    w = window_weights(L, T, starts, "tent")
    j = np.arange(ov, dtype=np.float64)
    # frames 192 .. 255: window 0 hands over to window 1 - raw weights 64 - j and j + 1, their sum 65 at every frame
    assert np.array_equal(w[0][192:256], ((ov - j) / (ov + 1)).astype(np.float32))
    assert np.array_equal(w[1][:ov], ((j + 1) / (ov + 1)).astype(np.float32))
    u = window_weights(L, T, starts, "uniform")
    assert (u[0][192:256] == 0.5).all() and (u[1][:ov] == 0.5).all() and (u[0][:192] == 1).all() and (u[1][ov:] == 1).all()


def test_three_cover_plan():
    L, T, ov = 600, 256, 128
    starts = _starts(L, T, ov)
    assert starts == [0, 128, 256, 344]
    w = window_weights(L, T, starts, "tent")
    cover = np.zeros(L, np.int64)
    for s in starts:
        cover[s:s + T] += 1
    assert cover.max() == 3 and (cover[344:384] == 3).all()
    f = 350                                                      # under windows 1, 2 and 3
    raw = [min(f - s + 1, T - (f - s)) for s in starts[1:]]
    assert np.array_equal(np.array([w[k + 1][f - s] for k, s in enumerate(starts[1:])]), (np.array(raw) / float(sum(raw))).astype(np.float32))


def test_weights_refuse_bad_plans():
    for starts in ([0, 300], [0, 192, 100], [10, 192], [0, 100], []):
        with pytest.raises(ValueError, match="starts"):
            window_weights(448, 256, starts)
    with pytest.raises(ValueError, match="blend"):
        window_weights(448, 256, [0, 192], "cosine")


# ---- the checker --------------------------------------------------------------------------------------------------------------------
S = 25


@pytest.fixture(scope="module")
def small():
    """2 x 96 features and noise, seeded."""
    xfp, xfo = xf_pair(2, 96, first=60)
    return oracle_params(), xfp, xfo, torch.from_numpy(batch_noise(2, 96, first=60))


def test_checker_with_one_window_is_the_oracle_loop(small):
    p, xfp, xfo, x = small
    ones = np.ones((1, 96), np.float32)
    with torch.no_grad():
        ref = O.ddim_sample_loop(p, x, xfp, xfo, [96, 96], S, idxs=(0, 3))
    got = ddim_windows_loop(p, x, xfp, xfo, [0], ones, S, idxs=(0, 3))
    for k in (0, 3, S):
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], ref[k])


def test_checker_without_overlap_is_independent_loops(small):
    """One piece of 192 frames under two windows that do not overlap: the two plain loops side by side."""
    p, xfp, xfo, x = small
    piece = torch.cat([x[0], x[1]]).unsqueeze(0)                 # [1, 192, 26]: window 0 = clip 0's noise, window 1 = clip 1's
    w = window_weights(192, 96, [0, 96])
    assert (w == 1).all()
    with torch.no_grad():      # (each loop alone, as the checker calls the model: a CPU GEMM's rounding depends on its batch)
        ref = [O.ddim_sample_loop(p, x[b:b + 1], xfp[b:b + 1], xfo[b:b + 1], [96], S, idxs=(3,)) for b in range(2)]
    got = ddim_windows_loop(p, piece, xfp, xfo, [0, 96], w, S, idxs=(3,))
    for k in (3, S):
        assert torch.equal(got[k].view(2, 96, 26), torch.cat([ref[0][k], ref[1][k]]))


def test_blending_moves_the_overlap(small):
    """Keeps the tests above from being vacuous: with an overlap the joint loop is not the two plain loops."""
    p, xfp, xfo, x = small
    L, starts = 160, [0, 64]
    piece = torch.from_numpy(batch_noise(1, L, first=90))
    got = ddim_windows_loop(p, piece, xfp, xfo, starts, window_weights(L, 96, starts), S)
    with torch.no_grad():
        alone = O.ddim_sample_loop(p, piece[:, :96].contiguous(), xfp[:1], xfo[:1], [96], S)
    assert torch.isfinite(got).all() and not torch.equal(got[:, :96], alone)


# ---- the launch rule ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    run = windows_probe(tmp_path_factory)
    return lambda *cases: run(*["form loop=1 graph_step=0 g1_loop=1 next_plain=1 " + c for c in cases])


# the INTERNAL shapes (W B windows x T, x 2 guided) of tests/test_gpu_windows.py and the form each is there for (256 compute units)
FORMS = [("layer16", "B=2 Tx=256", dict(layer16=1, narrow=1)),
         ("narrow", "B=72 Tx=256", dict(layer16=0, narrow=1, aligned=1)),
         ("wide_aligned", "B=160 Tx=256", dict(narrow=0, wgr=1, aligned=1, embed_next=1)),
         ("wide_flat", "B=110 Tx=300", dict(narrow=0, wgr=1, aligned=0, embed_next=1, stride=300)),
         ("group_96", "B=2 Tx=96", dict(wgr=0, layer16=0)),
         ("no_eff", "B=2 Tx=96 no_eff=1", dict(wgr=0, folded=0)),
         ("bf16", "B=2 Tx=256 prec=0", dict(layer16=1, fs=0, ff=0)),
         ("mixed", "B=2 Tx=256 prec=1", dict(ss=1, mixed_form=1, wgr=1, aligned=1)),
         ("three_cover", "B=4 Tx=256", dict(layer16=1, narrow=1)),
         ("odd", "B=2 Tx=255", dict(wgr=0, layer16=0, stride=255)),
         ("guided", "B=4 Tx=256 guided=1", dict(layer16=1, narrow=1, guided=1))]
GIVEN_UP = ("embed_next", "upd_flags", "windows", "key_bits")


def test_forms_cover_the_gpu_shapes():
    assert [n for n, _, _ in FORMS] == list(SHAPES)
    for name, case, _ in FORMS:
        _, B, T, _, L, W, w = SHAPES[name]
        assert f"B={W * B * (2 if w else 1)} Tx={T}" in case and len(plan_windows(L, T, SHAPES[name][3])) == W


@pytest.mark.parametrize("name,case,want", FORMS, ids=[n for n, _, _ in FORMS])
def test_windows_bit_gives_up_embed_next_and_nothing_else(probe, name, case, want):
    W = SHAPES[name][5]
    base, f = probe(case, case + f" windows={W}")
    assert not base["error"] and not f["error"], (base, f)
    assert {k: base[k] for k in want} == want, base
    assert base["windows"] == 0 and f["windows"] == 1
    assert f["embed_next"] == 0 and f["upd_flags"] == base["upd_flags"] & ~UPD_EMBED_NEXT
    assert {k: v for k, v in f.items() if k not in GIVEN_UP} == {k: v for k, v in base.items() if k not in GIVEN_UP}
    if want.get("embed_next"):
        assert base["upd_flags"] & UPD_EMBED_NEXT
    # the windows bit and the window count are in the graph key; the guided bits stay as they were
    assert f["key_bits"] == base["key_bits"] | KEY_WINDOWS | (W << 47)
    assert base["key_bits"] & ~(KEY_GUIDED | KEY_SHARED) == 0


def test_windows_compose_with_guidance_and_refuse_takes(probe):
    plain, guided, both, full = probe("B=4 Tx=256", "B=4 Tx=256 guided=1", "B=4 Tx=256 guided=1 windows=2",
                                      "B=4 Tx=256 guided=1 windows=2 env=DC_GUIDE_FULL_FILM")
    assert both["guided"] == 1 and both["windows"] == 1 and both["shared_film"] == guided["shared_film"] == 1
    assert both["film_groups"] == guided["film_groups"] == plain["G"] // 2 + 1           # the shared null column stays
    assert full["shared_film"] == 0 and full["film_groups"] == plain["G"]
    assert both["key_bits"] == KEY_GUIDED | KEY_SHARED | KEY_WINDOWS | (2 << 47)
    known, = probe("B=4 Tx=256 windows=2 known=1")
    assert known["upd_flags"] & 64
    takes, single, hook = probe("B=4 Tx=256 windows=2 takes=2", "B=4 Tx=256 windows=2 loop=0", "B=4 Tx=256 windows=2 layers=3")
    assert "takes" in takes["error"] and "loop step" in single["error"] and "loop step" in hook["error"]


def test_graph_key_names_the_plan_geometry(tmp_path_factory):
    run = windows_probe(tmp_path_factory)
    plain, a, b, c, t = run("plan B=6 Tx=256 S=25", "plan B=6 Tx=256 S=25 windows=2 win_L=448", "plan B=6 Tx=256 S=25 windows=3 win_L=448",
                            "plan B=6 Tx=256 S=25 windows=2 win_L=512", "plan B=6 Tx=256 S=25 takes=2")
    keys = [tuple(q["parts"][0]["key"]) for q in (plain, a, b, c, t)]
    assert len(set(keys)) == 5                                   # 2 windows x 3 pieces, 3 x 2, another piece length, takes, none: five graphs
    assert a["step_windows"] == 1 and plain["step_windows"] == 0
    assert keys[1][4] == keys[0][4] | KEY_WINDOWS | (2 << 47) and keys[1][5] == 448 and keys[0][5] == 0
    assert [len(q["parts"]) for q in (plain, a)] == [1, 1] and a["parts"][0]["steps"] == plain["parts"][0]["steps"] == 25


# ---- the plans the library refuses --------------------------------------------------------------------------------------------------
def _plan(L=448, T=256, overlap=64):
    starts = _starts(L, T, overlap)
    return starts, window_weights(L, T, starts), T, L


def test_good_plans_pass():
    native.windows_check(*_plan())
    native.windows_check(*_plan(600, 256, 128))
    native.windows_check([0], np.ones((1, 256), np.float32), 256, 256)


BAD = {"unordered": lambda s, w, T, L: ([0, 200, 192, 344], np.ones((4, T), np.float32), T, 600),
       "equal starts": lambda s, w, T, L: ([0, 0, 192], np.concatenate([w[:1] / 2, w[:1] / 2, w[1:]]), T, L),
       "gap": lambda s, w, T, L: ([0, 300], np.ones((2, T), np.float32), T, 556),
       "first start": lambda s, w, T, L: ([8, 192], w, T, L),
       "last start": lambda s, w, T, L: ([0, 184], w, T, L),
       "cover": lambda s, w, T, L: ([0, 32, 64, 96, 128], np.full((5, T), 0.2, np.float32), T, 128 + T),
       "negative": lambda s, w, T, L: (s, np.where(np.arange(T) == 200, -w, w).astype(np.float32), T, L),
       "nan": lambda s, w, T, L: (s, np.where(np.arange(T) == 10, np.nan, w).astype(np.float32), T, L),
       "inf": lambda s, w, T, L: (s, np.where(np.arange(T) == 10, np.inf, w).astype(np.float32), T, L),
       "sum": lambda s, w, T, L: (s, np.concatenate([w[:1], w[1:] * np.float32(1 + 8 * ULP)]), T, L),
       "sum single": lambda s, w, T, L: (s, w * np.float32(1 - 8 * ULP), T, L)}
REASON = {"unordered": "ascend", "equal starts": "ascend", "gap": "no window", "first start": "not 0", "last start": "L - T", "cover": "more than 4",
          "negative": "negative", "nan": "not finite", "inf": "not finite", "sum": "sum to", "sum single": "sum to"}


@pytest.mark.parametrize("what", list(BAD))
def test_bad_plans_are_refused_on_the_host(what):
    args = BAD[what](*_plan())
    with pytest.raises(ValueError, match=REASON[what]):
        native.windows_check(*args)
    assert REASON[what] in native.lib().dc_last_error().decode()


def test_four_ulp_is_the_sum_tolerance():
    s, w, T, L = _plan()
    up = w.copy()
    up[1][100] = np.float32(1 + 3 * ULP)                         # a single-cover frame at 1 + 3 ulp: inside
    native.windows_check(s, up, T, L)
    up[1][100] = np.float32(1 + 6 * ULP)
    with pytest.raises(ValueError, match="sum to"):
        native.windows_check(s, up, T, L)


def test_lengths_are_refused():
    s, w, T, L = _plan()
    with pytest.raises(ValueError, match="full"):
        native.windows_check(s, w, T, L, length=[T, T])
    # the raw entry point: DC_ERR_INVALID (-1) for an h_length, for a null plan and for a bad plan, without a sampler
    import ctypes as C
    st, wt = np.asarray(s, np.int32), np.ascontiguousarray(w, np.float32)
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    ln = np.asarray([T, T], np.int32)
    lib = native.lib()
    assert lib.dc_windows_check(st.ctypes.data_as(ip), wt.ctypes.data_as(fp), 2, T, L, ln.ctypes.data_as(ip)) == -1
    assert lib.dc_windows_check(None, wt.ctypes.data_as(fp), 2, T, L, None) == -1
    assert lib.dc_windows_check(st.ctypes.data_as(ip), wt.ctypes.data_as(fp), 2, T, L + 1, None) == -1
    assert lib.dc_windows_check(st.ctypes.data_as(ip), wt.ctypes.data_as(fp), 2, T, L, None) == 0
    # ... and a sampler that was never finalized refuses the call before it looks at anything else
    assert lib.dc_sampler_set_conditioning_windows(None, None, None, None, st.ctypes.data_as(ip), wt.ctypes.data_as(fp), 1, 2, T, L, None, None,
                                                   None) == -1
