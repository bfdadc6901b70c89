"""Every music against every motion on the MI355X (csrc/dc_m2snet.hip k_m2s_pairs, M2SNet.fuse_pairs) and what is built on it
(evaluate_dataset(retrieval=True), evaluate.sync_negatives).

The probabilities are compared bit for bit with `fuse` on the same pair, the counts exactly with counts taken from those
probabilities, and the sums with the float64 sum of the kernel's own fp32 probabilities.

The sum's bound.  A pair's sum is taken in one order (helpers_retrieval.ordered_sum restates it): inside a 32-frame tile a binary
tree of five levels over the lanes, then the tiles' partials one after the other in ascending order.  A probability therefore
passes through at most d = 5 + ceil(T / 32) - 1 fp32 additions, each of relative error at most u = 2^-24, all terms non-negative:
|sum - exact| <= ((1 + u)^d - 1) sum(p) <= (d + 1) u sum(p) for every d this file reaches (d u << 1).
The mean against the fp64 oracle adds FUSE_PROB_TOL of test_gpu_m2snet.py (6e-6 per probability, hence per mean) to that bound
divided by the frame count.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers_m2snet import oracle_head
from helpers_retrieval import (MusicOnlySampler, fuse_every_pair, latents, numbers_from_frames, ordered_sum, reduction_depth,
                               retrieval_keys)
from test_gpu_m2snet import FUSE_PROB_TOL

from diffusion_conductor_amd import evaluate as ev
from diffusion_conductor_amd import metrics
from diffusion_conductor_amd.m2snet import M2SNet
from diffusion_conductor_amd.native import DcError, NativeM2SNet, lib
from diffusion_conductor_amd.synthetic import batch_mel, synthetic_m2snet_state_dict, synthetic_motion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TS = (1, 31, 32, 33, 127, 128, 129, 257)                  # tile, workgroup (4 tiles) and two-workgroup edges
SHAPES = ((1, 1), (1, 3), (3, 1), (3, 5))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def weights():
    return synthetic_m2snet_state_dict(0)


@pytest.fixture(scope="module")
def net(weights):
    return M2SNet(DEV).load_state_dict(weights, strict=True)


@pytest.fixture(scope="module")
def share():
    return NativeM2SNet.pairs_share()


@pytest.fixture(scope="module")
def run(net):
    """(T, Bm, Bn) -> the latents, fuse_pairs' outputs as numpy, and `fuse` on every pair, computed once and left unchanged."""
    cache, lat = {}, {}

    def get(T, Bm, Bn):
        key = (T, Bm, Bn)
        if key not in cache:
            B = max(Bm, Bn)
            if (T, B) not in lat:
                lat[(T, B)] = latents(net, B, T)
            mus, mot = lat[(T, B)][0][:Bm].contiguous(), lat[(T, B)][1][:Bn].contiguous()
            r = net.fuse_pairs(mus, mot, return_frames=True)
            assert tuple(r["prob"].shape) == (Bm, Bn, T) and r["mean"].dtype == torch.float32 and r["above"].dtype == torch.int32
            cache[key] = (mus, mot, {k: v.cpu().numpy() for k, v in r.items()}, fuse_every_pair(net, mus, mot))
        return cache[key]
    return get


CASES = [(T, bm, bn) for T in TS for bm, bn in SHAPES]


def _straddle(share):
    return [(33, 2, bn) for bn in (share - 1, share, share + 1, 2 * share + 1)]


@pytest.mark.parametrize("T,Bm,Bn", CASES)
def test_frames_are_fuse_bit_for_bit(run, T, Bm, Bn):
    _, _, r, ref = run(T, Bm, Bn)
    assert r["prob"].dtype == np.float32 and np.array_equal(r["prob"].view(np.uint32), ref.view(np.uint32)), (T, Bm, Bn)
    assert 0 < ref.min() and ref.max() < 1


def test_frames_are_fuse_bit_for_bit_across_the_share(run, share):
    """Motions S - 1, S, S + 1 and 2 S + 1 for the S motions one wave walks: the last wave's share is short, full, one, one."""
    for T, Bm, Bn in _straddle(share):
        _, _, r, ref = run(T, Bm, Bn)
        assert np.array_equal(r["prob"].view(np.uint32), ref.view(np.uint32)), Bn
        total, above, below, count = numbers_from_frames(r["prob"])
        assert np.array_equal(r["sum"].view(np.uint32), total.view(np.uint32)), Bn
        assert np.array_equal(r["above"], above) and np.array_equal(r["below"], below) and np.array_equal(r["count"], count), Bn


@pytest.mark.parametrize("T,Bm,Bn", CASES)
def test_counts_are_the_strict_comparisons(run, T, Bm, Bn):
    _, _, r, _ = run(T, Bm, Bn)
    assert np.array_equal(r["above"], (r["prob"] > 0.5).sum(axis=2)) and np.array_equal(r["below"], (r["prob"] < 0.5).sum(axis=2))
    assert np.array_equal(r["count"], np.full((Bm, Bn), T)) and r["above"].dtype == np.int32 and r["below"].dtype == np.int32
    assert np.array_equal(r["above"] + r["below"] + (r["prob"] == 0.5).sum(axis=2), r["count"])


@pytest.mark.parametrize("T,Bm,Bn", CASES)
def test_sum_against_the_exact_sum(run, T, Bm, Bn):
    _, _, r, _ = run(T, Bm, Bn)
    exact = r["prob"].astype(np.float64).sum(axis=2)
    err = np.abs(r["sum"].astype(np.float64) - exact)
    bound = (reduction_depth(T) + 1) * U * exact
    print(f"pairs T={T} {Bm}x{Bn}: |sum - exact| max {err.max():.3e}, bound min {bound.min():.3e}")
    assert (err <= bound).all(), (T, Bm, Bn, float(err.max()), float(bound.min()))
    # and it is the stated order, bit for bit
    assert np.array_equal(r["sum"].view(np.uint32), numbers_from_frames(r["prob"])[0].view(np.uint32))
    assert np.array_equal(r["mean"].view(np.uint32), (r["sum"] / np.float32(T)).view(np.uint32))


@pytest.mark.parametrize("T,Bm,Bn", CASES)
def test_mean_against_the_fp64_oracle(run, weights, T, Bm, Bn):
    mus, mot, r, _ = run(T, Bm, Bn)
    m = mus.cpu().repeat_interleave(Bn, 0)                # pair (i, j) at i Bn + j
    y = mot.cpu().repeat(Bm, 1, 1)
    prob64 = oracle_head(weights, m, y)[1].reshape(Bm, Bn, T)
    mean64 = prob64.mean(axis=2)
    err = np.abs(r["mean"].astype(np.float64) - mean64)
    bound = FUSE_PROB_TOL + (reduction_depth(T) + 1) * U * prob64.sum(axis=2) / T + U      # (+ the division's own rounding, means < 1)
    print(f"pairs T={T} {Bm}x{Bn}: |mean - fp64| max {err.max():.3e}, |p - fp64| max {np.abs(r['prob'] - prob64).max():.3e}")
    assert (err <= bound).all(), (T, Bm, Bn, float(err.max()))


@pytest.fixture(scope="module")
def ragged(net, run):
    T, Bm, Bn = 129, 3, 5
    mus, mot, full, _ = run(T, Bm, Bn)
    lm, ln = np.array([1, T, 70], np.int32), np.array([T, 33, 1, 64, 100], np.int32)
    return T, mus, mot, full, lm, ln


def test_lengths_are_the_truncated_pair(net, ragged):
    """Ragged lengths, 1 and T among them: a pair's numbers are those of its first min(len) frames - from the full call's
    probabilities in the library's order, and from a call on the latents cut to min(len) frames."""
    T, mus, mot, full, lm, ln = ragged
    r = {k: v.cpu().numpy() for k, v in net.fuse_pairs(mus, mot, lm, ln, return_frames=True).items()}
    assert np.array_equal(r["prob"].view(np.uint32), full["prob"].view(np.uint32))         # every frame is written, valid or not
    total, above, below, count = numbers_from_frames(full["prob"], lm, ln)
    assert np.array_equal(r["count"], count) and count.min() == 1 and count.max() == T
    assert np.array_equal(r["sum"].view(np.uint32), total.view(np.uint32))
    assert np.array_equal(r["above"], above) and np.array_equal(r["below"], below)
    assert np.array_equal(r["mean"].view(np.uint32), (total / count.astype(np.float32)).view(np.uint32))
    quiet = {k: v.cpu().numpy() for k, v in net.fuse_pairs(mus, mot, lm, ln).items()}      # without the frames: empty tiles are skipped
    assert "prob" not in quiet
    for k in ("sum", "mean", "above", "below", "count"):
        assert np.array_equal(quiet[k].view(np.uint32), r[k].view(np.uint32)), k
    for i in range(3):
        for j in range(5):
            n = int(count[i, j])
            cut = net.fuse_pairs(mus[i:i + 1, :n].contiguous(), mot[j:j + 1, :, :n].contiguous(), return_frames=True)
            assert torch.equal(cut["prob"][0, 0].cpu(), torch.from_numpy(full["prob"][i, j, :n]))
            for k in ("sum", "above", "below"):
                assert cut[k].cpu().numpy()[0, 0].tobytes() == r[k][i, j].tobytes(), (i, j, k)
    # one side's lengths alone
    only = net.fuse_pairs(mus, mot, len_motion=ln)
    assert np.array_equal(only["count"].cpu().numpy(), np.broadcast_to(ln[None, :], (3, 5)))
    assert np.array_equal(only["sum"].cpu().numpy().view(np.uint32), numbers_from_frames(full["prob"], None, ln)[0].view(np.uint32))


def test_a_pair_does_not_depend_on_the_call(net, ragged):
    T, mus, mot, full, lm, ln = ragged
    keys = ("sum", "above", "below")
    again = {k: v.cpu().numpy() for k, v in net.fuse_pairs(mus, mot).items()}
    rev = {k: v.cpu().numpy() for k, v in net.fuse_pairs(mus.flip(0).contiguous(), mot.flip(0).contiguous()).items()}
    for k in keys:
        assert again[k].tobytes() == full[k].tobytes(), k                                   # two runs
        assert np.ascontiguousarray(rev[k][::-1, ::-1]).tobytes() == full[k].tobytes(), k   # rows and columns reversed
    for i in range(3):
        for j in range(5):
            one = net.fuse_pairs(mus[i:i + 1], mot[j:j + 1])
            for k in keys:
                assert one[k].cpu().numpy()[0, 0].tobytes() == full[k][i, j].tobytes(), (i, j, k)


def test_nan_stays_in_its_column(net, ragged):
    T, mus, mot, full, _, _ = ragged
    bad = mot.clone()
    bad[2, 17, 40] = float("nan")                             # one channel of one frame of motion 2
    r = {k: v.cpu().numpy() for k, v in net.fuse_pairs(mus, bad, return_frames=True).items()}
    hit = np.zeros((3, 5, T), bool)
    hit[:, 2, 40] = True
    assert np.array_equal(np.isnan(r["prob"]), hit)
    assert np.array_equal(r["prob"][~hit].view(np.uint32), full["prob"][~hit].view(np.uint32))
    assert np.isnan(r["sum"][:, 2]).all() and np.isnan(r["mean"][:, 2]).all()
    clean40 = full["prob"][:, 2, 40]
    assert np.array_equal(r["above"][:, 2], full["above"][:, 2] - (clean40 > 0.5)), "the NaN frame counted as above"
    assert np.array_equal(r["below"][:, 2], full["below"][:, 2] - (clean40 < 0.5)), "the NaN frame counted as below"
    assert np.array_equal(r["above"][:, 2] + r["below"][:, 2] + (full["prob"][:, 2] == 0.5).sum(axis=1), np.full(3, T - 1))
    others = [0, 1, 3, 4]
    for k in ("sum", "mean", "above", "below"):
        assert r[k][:, others].tobytes() == full[k][:, others].tobytes(), k


def test_refusals_leave_the_outputs_untouched(weights):
    T, Bm, Bn = 40, 2, 3
    L, ptr = lib(), lambda t: t.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    spare = torch.zeros(Bm * T * 64 + 4, device=DEV)
    mus, mot = spare[:Bm * T * 64].view(Bm, T, 64), torch.zeros(Bn, 64, T, device=DEV)
    total = torch.full((Bm, Bn), 7.0, device=DEV)
    above = torch.full((Bm, Bn), 7, dtype=torch.int32, device=DEV)
    below, prob = above.clone(), torch.full((Bm, Bn, T), 7.0, device=DEV)
    ip = C.POINTER(C.c_int32)

    def call(n, m=None, y=None, bm=Bm, bn=Bn, t=T, lm=None, ln=None, s=None, a=None, b=None):
        lens = [None if v is None else np.asarray(v, np.int32) for v in (lm, ln)]
        return L.dc_m2snet_fuse_pairs(n, ptr(mus) if m is None else m, ptr(mot) if y is None else y, bm, bn, t,
                                      *(None if v is None else v.ctypes.data_as(ip) for v in lens), ptr(total) if s is None else s,
                                      ptr(above) if a is None else a, ptr(below) if b is None else b, ptr(prob), stream)

    n = NativeM2SNet(0)
    assert call(n._h) == -1 and b"finalize" in L.dc_last_error()              # before finalize
    for k, v in weights.items():
        n.set_param(k, v)
    n.finalize()
    null = C.c_void_p(None)
    assert call(None) == -1
    for kw in ({"m": null}, {"y": null}, {"s": null}, {"a": null}, {"b": null}):
        assert call(n._h, **kw) == -1 and b"NULL" in L.dc_last_error(), kw
    assert call(n._h, m=C.c_void_p(ptr(spare) + 4)) == -1 and b"aligned" in L.dc_last_error()
    for kw in ({"bm": 0}, {"bn": 0}, {"t": 0}, {"bm": -1}):
        assert call(n._h, **kw) == -1, kw
    for kw in ({"lm": [0, T]}, {"lm": [T, T + 1]}, {"ln": [T, -3, T]}, {"ln": [1, 1, T + 1]}):
        assert call(n._h, **kw) == -1 and b"outside [1, 40]" in L.dc_last_error(), kw
    torch.cuda.synchronize()
    assert bool((total == 7).all()) and bool((above == 7).all()) and bool((below == 7).all()) and bool((prob == 7).all())
    with pytest.raises(DcError, match="error -1.*outside"):
        n.fuse_pairs(mus, mot, len_music=[T, T + 1])
    with pytest.raises(ValueError, match="len_motion must have shape"):
        n.fuse_pairs(mus, mot, len_motion=[T, T])
    assert call(n._h, lm=[1, T], ln=[T, 2, 3]) == 0                            # and the same arguments, in range, run
    torch.cuda.synchronize()
    assert bool((above + below <= 40).all()) and not bool((total == 7).any())
    n.close()


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    T, n = 96, 5
    mels, gts = batch_mel(n, 3 * T - 2), synthetic_motion(n, T, seed=21)
    roots = {}
    for name, order in (("forward", range(n)), ("reversed", reversed(range(n)))):
        root = tmp_path_factory.mktemp(name)
        for pos, i in enumerate(order):
            d = root / f"{pos:03d}"
            d.mkdir()
            np.save(d / "mel.npy", mels[i])
            np.save(d / "motion.npy", gts[i])
        roots[name] = str(root)
    return T, n, mels, gts, roots


TIMING_KEYS = ("seconds", "frames_per_s", "main_thread_s", "steady_frames_per_s", "metrics_s", "m2s_retrieval_s")
NEW_KEYS = ("m2s_r_precision_real", "m2s_r_precision_gen", "m2s_mean_rank_real", "m2s_mean_rank_gen", "m2s_sync_offdiag_gen",
            "m2s_margin_real", "m2s_margin_gen", "m2s_pair_accuracy_real", "m2s_pair_accuracy_gen")


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def test_evaluate_dataset_retrieval(net, dataset):
    T, n, mels, gts, roots = dataset
    tr = MusicOnlySampler(DEV)
    runs = {bs: ev.evaluate_dataset(tr, roots["forward"], 26, batch_size=bs, seed=5, verbose=False, m2snet=net, retrieval=True)
            for bs in (1, 2, 5)}
    # the keys from `fuse` on every pair, reduced and ranked on the host
    mus = net.music_latent(mels)
    pred = tr.generate_music_motion(mels, 26)
    mean, cnt = {}, {}
    for name, motion in (("real", gts), ("gen", pred.reshape(n, T, 13, 2))):
        total, above, below, count = numbers_from_frames(fuse_every_pair(net, mus, net.motion_latent(motion)))
        mean[name], cnt[name] = total / count.astype(np.float32), (above, below, count)
    want = retrieval_keys(mean["real"], mean["gen"], cnt["real"], cnt["gen"])
    assert sorted(want) == sorted(NEW_KEYS)
    for bs, r in runs.items():
        for k in NEW_KEYS:
            assert r[k] == want[k], (bs, k, r[k], want[k])
        assert len(r["m2s_r_precision_gen"]) == 3 and r["m2s_retrieval_s"] > 0
    print("retrieval keys: " + "  ".join(f"{k}={runs[5][k]}" for k in NEW_KEYS))
    # the clips in reverse order: the same numbers (no ties in these scores)
    back = ev.evaluate_dataset(tr, roots["reversed"], 26, batch_size=2, seed=5, verbose=False, m2snet=net, retrieval=True)
    assert np.unique(mean["gen"]).size == n * n and np.unique(mean["real"]).size == n * n
    for k in NEW_KEYS:
        if "rank" in k or "r_precision" in k or "accuracy" in k:
            assert back[k] == want[k], (k, back[k], want[k])          # integers over N
        else:
            assert abs(back[k] - want[k]) <= 1e-12, (k, back[k], want[k])          # float64 means of the same N^2 numbers, other order
    # without the flag: the keys that were there, bit for bit
    for bs in (1, 2, 5):
        base = ev.evaluate_dataset(tr, roots["forward"], 26, batch_size=bs, seed=5, verbose=False, m2snet=net)
        assert not any(k in base for k in NEW_KEYS + ("m2s_retrieval_s",))
        assert sorted(set(runs[bs]) - set(NEW_KEYS) - {"m2s_retrieval_s"}) == sorted(base)
        for k in base:
            if k not in TIMING_KEYS:
                assert _same(runs[bs][k], base[k]), (bs, k)
    with pytest.raises(ValueError, match="m2snet"):
        ev.evaluate_dataset(tr, roots["forward"], 26, batch_size=2, verbose=False, retrieval=True)


def test_sync_negatives_is_the_three_strategies_by_hand(net):
    """One batch of two clips of 13 s, windows of 1 s: each strategy's numbers are metrics.sync_stats of `forward` on the windows
    evaluate.negative_windows names (checked against the reference's PairBuilder in test_host_retrieval.py)."""
    L, c = 13, 1
    mel = torch.from_numpy(batch_mel(2, 90 * L, seed=3))
    motion = torch.from_numpy(synthetic_motion(2, 30 * L, seed=4))
    g = np.random.RandomState(0)
    draws, refused = {}, None
    for strategy, nu in ev.NEGATIVE_STRATEGIES.items():      # the first seeded draws whose windows the reference's torch.cat accepts
        while strategy not in draws:
            u = g.rand(nu)
            w = ev.negative_windows(strategy, u, L, c)
            frames = lambda k: w[k][1] - w[k][0]
            if all((frames("music_1") - 1) // 3 + 1 == frames(k) for k in ("motion_1", "motion_2")):
                draws[strategy] = u
            else:
                refused = (strategy, u)
    got = ev.sync_negatives(net, mel, motion, L, c, draws)
    assert sorted(got) == sorted(ev.NEGATIVE_STRATEGIES)
    for strategy, u in draws.items():
        w = ev.negative_windows(strategy, u, L, c)
        mel_1 = mel[:, w["music_1"][0]:w["music_1"][1]].contiguous()
        motion_1 = motion[:, w["motion_1"][0]:w["motion_1"][1]].contiguous()
        motion_2 = motion_1.flip(0).contiguous() if strategy == "easy" else motion[:, w["motion_2"][0]:w["motion_2"][1]].contiguous()
        p11, p12 = net(mel_1, motion_1), net(mel_1, motion_2)
        assert tuple(p11.shape) == (2, 30 * c, 1)
        want = metrics.sync_stats(p11, p12)
        assert got[strategy] == want, (strategy, got[strategy], want)
        tp, tf = int((p11.cpu().numpy() > 0.5).sum()), int((p12.cpu().numpy() < 0.5).sum())
        assert got[strategy]["accuracy"] == (tp + tf) / (2 * 2 * 30 * c)                   # M2SNet_eval.py:67
    if refused is not None:
        with pytest.raises(ValueError, match="torch.cat"):
            ev.sync_negatives(net, mel, motion, L, c, {refused[0]: refused[1]})
    assert ev.sync_negatives(net, mel, motion, L, c, {"easy": draws["easy"]}).keys() == {"easy"}
