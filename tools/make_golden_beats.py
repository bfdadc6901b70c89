#!/usr/bin/env python3
"""Generate tests/golden/g18_beats.npz by IMPORTING THE REFERENCE (the build container only; the GPU box never runs it).

Run:  python tools/make_golden_beats.py [reference Contrastive_Stage dir]     (default: beside oracle/make_golden.py's REF; seconds)

What it does
  1. imports the reference's Contrastive_Stage/M2SGAN_eval.py on the CPU with `librosa`, `cv2` and `torch.utils.tensorboard` stubbed in
     sys.modules (none of the three is touched by the two functions used; librosa is not installed here);
  2. for the seeded motion pairs of tests/helpers_beats.py (fixture_pair: three clips at every length of FIXTURE_T) calls
     M2SGAN_Evaluator.motion_peak_onehot(None, m) clip by clip (both functions ignore `self`) and stores the one-hots and the envelopes -
     the envelope recomputed as the reference's lines compute it (np.linalg.norm over the last axis, np.sum over the joints), since
     motion_peak_onehot does not return it;
  3. for the lengths of SCORED_T calls .alignment_score(None, music, one-hot, sigma=3) with the seeded music beats
     (helpers_beats.fixture_music: Lm = 3 T, a beat every 37 mel frames) and stores the float32 scores;
  4. asserts, on the reference alone:
       - the float32 summation order of tests/helpers_beats.py (envelope_f32) and of metrics.motion_beats_host reproduces the
         reference's envelope bit for bit ON THE NUMPY THIS RUNS UNDER (the order is numpy's pairwise reduction over 13 contiguous
         values; a plain left-to-right sum does not reproduce it, which is asserted too);
       - every clip of 300 or more frames has at least 5 motion beats, the real and the generated one-hots differ, and every stored BC
         lies strictly between 0.02 and 0.98 - so a test on this fixture can fail.

Motions and music beats are regenerated from their seeds by the tests; the file pins them by float64 digests (synthetic.array_digest).
Only data is written; no reference source text is copied.
"""
import os
import sys
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g18_beats.npz")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def main():
    from oracle.make_golden import REF
    import helpers_beats as H
    from diffusion_conductor_amd import metrics
    from diffusion_conductor_amd.synthetic import array_digest
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(REF)), "Contrastive_Stage")
    assert os.path.isdir(ref), f"{ref}: the reference is only present in the build container"
    warnings.filterwarnings("ignore")
    import torch.utils  # noqa: F401
    for name in ("librosa", "cv2"):
        if name not in sys.modules:
            _stub(name)
    _stub("torch.utils.tensorboard", SummaryWriter=object)
    sys.path.insert(0, ref)
    from M2SGAN_eval import M2SGAN_Evaluator as E

    out = {"lengths": np.array(H.FIXTURE_T), "scored_lengths": np.array(H.SCORED_T), "real_seed": H.REAL_SEED, "gen_seed": H.GEN_SEED,
           "numpy_version": np.array(np.__version__)}
    plain_differs = 0
    for T in H.FIXTURE_T:
        real, gen = H.fixture_pair(T)
        out[f"real_digest_T{T}"], out[f"gen_digest_T{T}"] = array_digest(real), array_digest(gen)
        for name, m in (("real", real), ("gen", gen)):
            onehot, env = [], []
            for i in range(H.CLIPS):
                oh = E.motion_peak_onehot(None, m[i])
                assert oh.dtype == bool and oh.shape == (T,)
                v = np.zeros_like(m[i], dtype=np.float32)                      # the envelope as the reference's lines compute it
                v[1:] = m[i][1:] - m[i][:-1]
                e = np.sum(np.linalg.norm(v, axis=2), axis=1)
                assert e.dtype == np.float32
                mine = H.envelope_f32(m[i])
                assert np.array_equal(e.view(np.uint32), mine.view(np.uint32)), f"summation order differs on numpy {np.__version__} at T={T}"
                assert np.array_equal(oh, H.minima(mine))
                n = np.linalg.norm(v, axis=2)
                left = np.zeros(T, np.float32)
                for j in range(13):
                    left = left + n[:, j]
                plain_differs += int((left.view(np.uint32) != e.view(np.uint32)).sum())
                onehot.append(oh)
                env.append(e)
            hb, he = metrics.motion_beats_host(m)
            assert np.array_equal(hb, np.stack(onehot)) and np.array_equal(he.view(np.uint32), np.stack(env).view(np.uint32))
            out[f"beats_{name}_T{T}"], out[f"envelope_{name}_T{T}"] = np.stack(onehot), np.stack(env)
            if T >= 300:
                assert min(int(o.sum()) for o in onehot) >= 5, (T, [int(o.sum()) for o in onehot])
        assert not np.array_equal(out[f"beats_real_T{T}"], out[f"beats_gen_T{T}"]) or T < 22, T
        if T in H.SCORED_T:
            mus = H.fixture_music(T)
            out[f"music_digest_T{T}"] = array_digest(mus)
            for name in ("real", "gen"):
                bc = np.array([E.alignment_score(None, mus, out[f"beats_{name}_T{T}"][i], sigma=H.SIGMA) for i in range(H.CLIPS)])
                assert bc.dtype == np.float32 and np.all((bc > 0.02) & (bc < 0.98)), bc
                ref64 = np.array([H.scores_f64(mus, out[f"beats_{name}_T{T}"][i])[0] for i in range(H.CLIPS)])
                n_mus = int(mus.sum())
                assert np.abs(bc - ref64).max() <= H.score_bound(n_mus), (bc, ref64)      # the reference against the fp64 oracle
                out[f"bc_{name}_T{T}"] = bc
                print(f"T={T} {name}: beats {[int(o.sum()) for o in out[f'beats_{name}_T{T}']]}  BC {bc}  vs fp64 {np.abs(bc - ref64).max():.2e}")
    for T in (300, 1800):
        assert not np.array_equal(out[f"beats_real_T{T}"], out[f"beats_gen_T{T}"])
    print(f"a plain left-to-right sum of the 13 norms differs from the reference's envelope in {plain_differs} frames")
    assert plain_differs > 0
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB")
    assert os.path.getsize(OUT) < 2 ** 20


if __name__ == "__main__":
    main()
