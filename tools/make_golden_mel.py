#!/usr/bin/env python3
"""Generate tests/golden/g21_mel.npz on the CPU: the seeded waveforms of the mel tests and their fp64 results.

Run:  python tools/make_golden_mel.py            (seconds; numpy only)

Neither librosa nor cv2 is installed where this project is built, so the file does NOT hold a run of the reference's
extract_mel_feature: it holds the fp64 oracle of tests/helpers_mel.py (written from librosa's and cv2's definitions) on the seeded
signals of that module, and pins both - the signal generator and the oracle - against drift.  What pins the oracle to the
reference is in tests/test_host_mel.py: librosa's documented example values, an independent STFT, a closed form, cv2's rule.

Stored, for each of the four signals (noise, chirp, tone, tone_silence) at N = 2304 samples (F = 10 frames, Tm = 9):
  wave_<name>_2304            fp32 [2304]
  power_<name>_2304_<pad>     fp64 [10, 128]     the mel power, pad = constant | reflect
  features_<name>_2304_<pad>  fp64 [9, 128]
and for the chirp at N = 22050 (F = 87, Tm = 90): the same with pad = constant.  Before writing, the tool asserts the anchors a
fixture can be trusted by: librosa's documented mel_frequencies / mel filter values, and that every filter is non-empty.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "g21_mel.npz")


def main():
    import helpers_mel as H
    mf = H.mel_frequencies(40, 0.0, 11025.0)
    assert np.allclose(mf[[0, 1, 2, 3, 12, 13]], [0.0, 85.317, 170.635, 255.952, 1024.856, 1119.114], atol=5e-4), mf
    fb = H.mel_filterbank()
    assert np.allclose(fb[0, :3], [0.0, 0.016, 0.032], atol=5e-4) and ((fb > 0).sum(1) >= 4).all()
    out = {}
    cases = [(name, 2304, pad) for name in H.SIGNALS for pad in ("constant", "reflect")] + [("chirp", 22050, "constant")]
    for name, n, pad in cases:
        out[f"wave_{name}_{n}"] = H.signal(name, n)
        out[f"power_{name}_{n}_{pad}"] = H.oracle(name, n, pad, "power")
        out[f"features_{name}_{n}_{pad}"] = H.oracle(name, n, pad, "features")
        assert out[f"features_{name}_{n}_{pad}"].shape == (H.out_frames(n), 128)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT) / 1e3:.1f} kB, {len(out)} arrays")
    assert os.path.getsize(OUT) < 2 ** 20


if __name__ == "__main__":
    main()
