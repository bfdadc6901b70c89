#!/usr/bin/env python3
"""Write the music beats of a dataset directory into one .npz, with librosa - the music half of beat consistency.

Run:  python tools/music_beats_librosa.py --data_root DIR --out FILE.npz

NEEDS librosa, which is neither on this project's build machine nor on its GPU box: this tool has never run there and no test covers
it.  Run it once per dataset wherever librosa is installed; `python -m diffusion_conductor_amd.evaluate --beats FILE.npz` (or
metrics.load_music_beats + evaluate_dataset(music_beats=)) reads the result.

For every clip `<id>/mel.npy` ([Lm, 128]) under DIR it stores, under the key `<id>`, the uint8 one-hot [Lm] of the beat frames the
reference's get_music_beat finds (Diffusion_Stage/tools/eval_new_metrics.py:319-344, Contrastive_Stage/M2SGAN_eval.py:369-394), with
the reference's parameters - FPS 90, hop length 512, so sr = 46080:
    envelope = librosa.onset.onset_strength(S=mel.T, sr=46080)
    librosa.onset.onset_detect(onset_envelope=envelope, sr=46080, hop_length=512)      # the reference calls it and drops the result
    tempo, beats = librosa.beat.beat_track(onset_envelope=envelope, sr=46080, hop_length=512, tightness=100)
The beats are a function of the mel alone - not of the model, the checkpoint, the seed or the sampled motion - so they are a property
of the dataset like mel.npy itself, and the numbers they lead to are the reference's exactly when the installed librosa is the
reference's."""
import argparse
import os
import sys

import numpy as np

FPS, HOP_LENGTH = 90, 512
SR = FPS * HOP_LENGTH


def music_beat_onehot(librosa, mel):
    """mel [Lm, n_mels] -> uint8 [Lm]."""
    envelope = librosa.onset.onset_strength(S=np.transpose(mel), sr=SR)
    librosa.onset.onset_detect(onset_envelope=envelope.flatten(), sr=SR, hop_length=HOP_LENGTH)
    _, beat_idxs = librosa.beat.beat_track(onset_envelope=envelope, sr=SR, hop_length=HOP_LENGTH, tightness=100)
    onehot = np.zeros(envelope.shape, np.uint8)
    onehot[beat_idxs] = 1
    return onehot


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data_root", required=True, help="directory of <id>/mel.npy + <id>/motion.npy")
    ap.add_argument("--out", required=True, help=".npz to write: one 1-D uint8 one-hot per clip id")
    args = ap.parse_args(argv)
    try:
        import librosa
    except ImportError:
        print("music_beats_librosa.py needs librosa (the reference's beat tracker), which is not installed here.  Run it where librosa "
              "is available; the project itself builds no beat tracker, because none could be shown to agree with librosa's.", file=sys.stderr)
        return 2
    ids = sorted(d for d in os.listdir(args.data_root) if os.path.isfile(os.path.join(args.data_root, d, "mel.npy")))
    if not ids:
        print(f"no <id>/mel.npy under {args.data_root}", file=sys.stderr)
        return 1
    beats = {}
    for cid in ids:
        beats[cid] = music_beat_onehot(librosa, np.load(os.path.join(args.data_root, cid, "mel.npy")))
        if not beats[cid].any():
            print(f"warning: no beat found in clip {cid}; beat consistency is undefined for it", file=sys.stderr)
    np.savez_compressed(args.out, **beats)
    print(f"wrote {args.out}: {len(ids)} clips, {sum(int(b.sum()) for b in beats.values())} beats")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
