"""metrics.retrieval_stats, metrics.pair_accuracy and evaluate.negative_windows against recorded outputs of the reference
(tests/golden/g20_retrieval.npz, tools/make_golden_retrieval.py: Diffusion_Stage/utils/metrics.py calculate_top_k and
Contrastive_Stage/utils/train_utils.py PairBuilder.build_pairs) and M2SNet_eval.py:65-68 on the matched / swapped pair set of
g13_m2snet_sync.npz.  No GPU."""
import numpy as np
import pytest

from helpers import golden
from helpers_retrieval import numbers_from_frames, ordered_sum, reduction_depth

from diffusion_conductor_amd import evaluate as ev
from diffusion_conductor_amd import metrics


@pytest.fixture(scope="module")
def g20():
    return golden("g20_retrieval.npz")


def test_top_k_table_is_the_references(g20):
    for n in g20["Ns"]:
        for kind in g20["kinds"]:
            s, ref = g20[f"score_{n}_{kind}"], g20[f"topk_{n}_{kind}"]
            st = metrics.retrieval_stats(s, (1, 2, 3))
            k = ref.shape[1]                                  # min(3, N): past it the reference indexes outside the matrix
            assert st["top_k_table"].shape == (n, 3) and st["top_k_table"].dtype == bool
            assert np.array_equal(st["top_k_table"][:, :k], ref), (n, kind)
            assert st["top_k_table"][:, k:].all(), (n, kind)  # every column found by rank N
            assert st["r_precision"][:k] == [float(ref[:, i].mean()) for i in range(k)], (n, kind)
            order = np.argsort(-s, axis=1, kind="stable")
            rank = np.array([int(np.where(order[i] == i)[0][0]) + 1 for i in range(n)], np.float64)
            assert np.array_equal(st["rank"], rank) and st["mean_rank"] == float(rank.mean())
            # the table is the rank, thresholded
            assert np.array_equal(st["top_k_table"], rank[:, None] <= np.arange(1, 4)[None, :])


def test_diagonal_best_worst_and_ties(g20):
    n = 7
    best = metrics.retrieval_stats(g20[f"score_{n}_diag_best"])
    assert best["r_precision"] == [1.0, 1.0, 1.0] and best["mean_rank"] == 1.0 and best["margin"] > 0
    worst = metrics.retrieval_stats(g20[f"score_{n}_diag_worst"])
    assert worst["r_precision"] == [0.0, 0.0, 0.0] and worst["mean_rank"] == float(n) and worst["margin"] < 0
    mid = metrics.retrieval_stats(g20[f"score_{n}_diag_middle"])
    # (the diagonal was set to the median of its row as drawn: it ties with the entry that had that value unless it was that entry,
    # with two or three of the other five above the pair - rank 3, 4 or 5, the tie going to the lower column)
    assert set(mid["rank"]) <= {3.0, 4.0, 5.0} and mid["r_precision"][:2] == [0.0, 0.0]
    # a constant matrix is one tie per row: the stable order is the column order, so row i's own column has rank i + 1
    flat = metrics.retrieval_stats(np.full((5, 5), 0.25))
    assert np.array_equal(flat["rank"], np.arange(1, 6)) and flat["r_precision"] == [0.2, 0.4, 0.6] and flat["margin"] == 0.0
    ties = g20[f"score_{n}_ties"]
    assert any(np.unique(r).size < n for r in ties) and any((r == r[i]).sum() > 1 for i, r in enumerate(ties))


def test_means_margin_and_shapes():
    s = np.array([[0.9, 0.1, 0.2], [0.3, 0.8, 0.4], [0.5, 0.6, 0.7]])
    st = metrics.retrieval_stats(s, top_k=(1, 3))
    assert st["r_precision"] == [1.0, 1.0] and st["top_k_table"].shape == (3, 3)
    assert st["diag_mean"] == np.mean([0.9, 0.8, 0.7]) and st["offdiag_mean"] == np.mean([0.1, 0.2, 0.3, 0.4, 0.5, 0.6])
    assert st["margin"] == st["diag_mean"] - st["offdiag_mean"]
    for bad in (np.zeros((2, 3)), np.zeros(4), np.zeros((0, 0))):
        with pytest.raises(ValueError, match="square"):
            metrics.retrieval_stats(bad)
    with pytest.raises(ValueError, match="top_k"):
        metrics.retrieval_stats(s, top_k=(0,))


def test_one_by_one_matrix():
    st = metrics.retrieval_stats(np.array([[0.3]]))
    assert st["r_precision"] == [1.0, 1.0, 1.0] and st["mean_rank"] == 1.0 and st["diag_mean"] == 0.3
    assert np.isnan(st["offdiag_mean"]) and np.isnan(st["margin"])
    assert metrics.pair_accuracy([[7]], [[2]], [[10]]) == 0.7


def test_nan_row_is_nan_not_a_place_in_the_order(g20):
    s = g20["score_7_random"].copy()
    clean = metrics.retrieval_stats(s)
    s[2, 5] = np.nan
    st = metrics.retrieval_stats(s)
    assert np.isnan(st["rank"][2]) and not st["top_k_table"][2].any()
    keep = np.arange(7) != 2
    assert np.array_equal(st["rank"][keep], clean["rank"][keep]) and np.array_equal(st["top_k_table"][keep], clean["top_k_table"][keep])
    assert all(np.isnan(v) for v in st["r_precision"]) and np.isnan(st["mean_rank"])
    assert np.isnan(st["offdiag_mean"]) and np.isnan(st["margin"]) and st["diag_mean"] == clean["diag_mean"]
    s = g20["score_7_random"].copy()
    s[3, 3] = np.nan                                          # on the diagonal
    st = metrics.retrieval_stats(s)
    assert np.isnan(st["rank"][3]) and np.isnan(st["diag_mean"]) and np.isnan(st["mean_rank"])


def test_pair_accuracy_is_the_references_expression():
    """M2SNet_eval.py:65-68 on the fixture's pair set: two clips against their own music (the diagonal) and with the motions swapped
    (the off-diagonal).  Matched and mismatched frames are equally many, so the balanced form 1/2 (TP / n + TF / n) is the
    reference's (TP + TF) / (2 n) up to the roundings of the two divisions and the sum: one ulp of a number in [0.5, 1]."""
    g13 = golden("g13_m2snet_sync.npz")
    matched, swapped = g13["stats_matched"][..., 0], g13["stats_mismatched"][..., 0]          # [2, T] each; swapped[i] = motion 1 - i
    prob = np.empty((2, 2, matched.shape[1]), np.float32)
    for i in range(2):
        prob[i, i], prob[i, 1 - i] = matched[i], swapped[i]
    _, above, below, count = numbers_from_frames(prob)
    acc = metrics.pair_accuracy(above, below, count)
    assert abs(acc - float(g13["stats_accuracy"])) <= 2.0 ** -53, (acc, float(g13["stats_accuracy"]))
    tp, tf = int((matched > 0.5).sum()), int((swapped < 0.5).sum())
    assert acc == 0.5 * (tp / matched.size + tf / swapped.size)
    # unequal weights: three mismatched pairs per matched one do not drown the matched side
    a, b, c = np.array([[8, 0], [0, 6]]), np.array([[0, 10], [10, 0]]), np.full((2, 2), 10)
    assert metrics.pair_accuracy(a, b, c) == 0.5 * (14 / 20 + 1.0)
    with pytest.raises(ValueError, match="square"):
        metrics.pair_accuracy(a, b[:1], c)


def test_negative_windows_are_pair_builders(g20):
    for L, c in g20["windows"]:
        for strategy in g20["strategies"]:
            us, ranges = g20[f"u_{L}_{c}_{strategy}"], g20[f"ranges_{L}_{c}_{strategy}"]
            assert us.shape[0] == 20 and ranges.shape == (20, 8)
            for u, r in zip(us, ranges):
                w = ev.negative_windows(str(strategy), u, int(L), int(c))
                got = [*w["music_1"], *w["motion_1"], *w["music_2"], *w["motion_2"]]
                assert got == [int(v) for v in r], (L, c, strategy, u)


def test_negative_windows_refuse():
    with pytest.raises(ValueError, match="strategy"):
        ev.negative_windows("medium", [0.5], 30, 5)
    with pytest.raises(ValueError, match="sample_length / 3"):
        ev.negative_windows("easy", [0.5], 30, 11)
    with pytest.raises(ValueError, match="uniform draw"):
        ev.negative_windows("hard", [0.5], 30, 5)


def test_ordered_sum_is_within_its_bound():
    """The order the GPU tests restate on the host: exact on integers, and within (d + 1) 2^-24 sum(p) of the float64 sum."""
    g = np.random.RandomState(5)
    for T in (1, 31, 32, 33, 129, 257):
        p = g.rand(T).astype(np.float32)
        for n in {1, T, (T + 1) // 2}:
            s = float(ordered_sum(p, n))
            exact = float(p[:n].astype(np.float64).sum())
            assert abs(s - exact) <= (reduction_depth(T) + 1) * 2.0 ** -24 * exact
        assert ordered_sum(np.ones(T, np.float32), T) == T
