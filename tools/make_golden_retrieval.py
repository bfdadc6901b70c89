#!/usr/bin/env python3
"""Generate tests/golden/g20_retrieval.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_retrieval.py [reference root]     (default: the parent of oracle/make_golden.py's REF; seconds)

What it does
  1. loads the reference's Diffusion_Stage/utils/metrics.py and Contrastive_Stage/utils/train_utils.py by file path (both live in a
     package called `utils`);
  2. for seeded score matrices [N, N], N in {1, 2, 7, 33}, of five kinds - "random", "ties" (scores rounded to a few values: exact
     ties, the diagonal's among them), "diag_best", "diag_worst", "diag_middle" - stores the matrix and the reference's
     calculate_top_k(np.argsort(-score, axis=1, kind="stable"), min(3, N)): the cumulative top-k table metrics.retrieval_stats
     must reproduce;
  3. for (sample_length, clip_length) in {(30, 5), (60, 20)} and each of PairBuilder.build_pairs' strategies, 20 draws under a seeded
     np.random: the uniform numbers it consumed (replayed from the same seed) and the index ranges it cut, read off index-valued
     tensors (value = frame index + 100000 x batch index) - what evaluate.negative_windows must reproduce draw by draw - and, for
     "easy", that the negative is the batch flipped.

Only data is written; no reference source text is copied.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "g20_retrieval.npz")
NS = (1, 2, 7, 33)
KINDS = ("random", "ties", "diag_best", "diag_worst", "diag_middle")
WINDOWS = ((30, 5), (60, 20))
STRATEGIES = (("easy", 1), ("hard", 2), ("super_hard", 2))
DRAWS = 20
BATCH_STRIDE = 100000


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def score_matrix(n, kind, seed):
    """The seeded score matrix of one (N, kind): float64 [N, N]."""
    g = np.random.RandomState(seed)
    s = g.rand(n, n)
    if kind == "ties":
        s = np.round(s * 3) / 3                       # four values: ties in every row of a 7 x 7
        s[::2, :] = np.round(s[::2, :])               # every other row: two values
    elif kind == "diag_best":
        s[np.arange(n), np.arange(n)] = 2.0
    elif kind == "diag_worst":
        s[np.arange(n), np.arange(n)] = -1.0
    elif kind == "diag_middle":
        s[np.arange(n), np.arange(n)] = np.median(s, axis=1)
    return s


def span(t):
    """(start, end, batch index of row 0) of an index-valued window [B, n, 1]."""
    v = t[0, :, 0].numpy().astype(np.int64)
    assert v.size and np.array_equal(np.diff(v), np.ones(v.size - 1, np.int64))
    return int(v[0] % BATCH_STRIDE), int(v[-1] % BATCH_STRIDE) + 1, int(v[0] // BATCH_STRIDE)


def main():
    from oracle.make_golden import REF
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(REF))
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    metrics = load(os.path.join(ref, "Diffusion_Stage", "utils", "metrics.py"), "ref_metrics")
    train_utils = load(os.path.join(ref, "Contrastive_Stage", "utils", "train_utils.py"), "ref_train_utils")
    out = {"Ns": np.array(NS), "kinds": np.array(KINDS), "windows": np.array(WINDOWS), "strategies": np.array([s for s, _ in STRATEGIES]),
           "batch_stride": BATCH_STRIDE}
    for n in NS:
        for ki, kind in enumerate(KINDS):
            s = score_matrix(n, kind, 1000 * n + ki)
            order = np.argsort(-s, axis=1, kind="stable")
            table = metrics.calculate_top_k(order, min(3, n))
            assert table.shape == (n, min(3, n)) and table.dtype == bool
            out[f"score_{n}_{kind}"], out[f"topk_{n}_{kind}"] = s, table
            print(f"N={n:2d} {kind:11s}: top-k hits {table.sum(axis=0)}")
    for L, c in WINDOWS:
        pb = train_utils.PairBuilder(types.SimpleNamespace(sample_length=L, clip_length=c))
        music = (torch.arange(L * 90, dtype=torch.float64)[None, :, None] + BATCH_STRIDE * torch.arange(2, dtype=torch.float64)[:, None, None])
        motion = (torch.arange(L * 30, dtype=torch.float64)[None, :, None] + BATCH_STRIDE * torch.arange(2, dtype=torch.float64)[:, None, None])
        for si, (strategy, nu) in enumerate(STRATEGIES):
            seed = 7000 + 100 * L + si
            np.random.seed(seed)
            us = np.random.RandomState(seed).rand(DRAWS, nu)          # the numbers build_pairs is about to draw, in its order
            rows = []
            for d in range(DRAWS):
                m1, m2, y1, y2 = pb.build_pairs(music, motion, strategy)
                (a0, a1, ab), (b0, b1, bb), (c0, c1, cb), (d0, d1, db) = span(m1), span(y1), span(m2), span(y2)
                assert (ab, bb) == (0, 0) and (cb, db) == ((1, 1) if strategy == "easy" else (0, 0))
                rows.append([a0, a1, b0, b1, c0, c1, d0, d1])
            assert np.array_equal(np.random.rand(3), np.random.RandomState(seed).rand(DRAWS * nu + 3)[-3:]), "draw count differs"
            out[f"u_{L}_{c}_{strategy}"], out[f"ranges_{L}_{c}_{strategy}"] = us, np.array(rows, np.int64)
            print(f"L={L} c={c} {strategy:10s}: first ranges {rows[0]}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
