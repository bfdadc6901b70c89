"""Drop-in for the sampling half of the reference's ``tools/visualization.py`` command line.

    python -m diffusion_conductor_amd.visualize --opt_path <.../opt.txt> --music_path <mel.npy | dir of *.npy | song.wav | dir of *.wav> \
        --npy_path out.npy --gpu_id 0 [--smooth] [--model latest.tar] [--seed 0] [--save_mel mel.npy]

Same flags and call sequence as Diffusion_Stage/tools/visualization.py:180-223: ``get_opt`` (this package's reader of the
training run's ``opt.txt``; the reference's is utils/get_opt.py:29-105) -> ``build_models`` (:169-178) -> ``DDPMTrainer`` ->
``trainer.load(<model_dir>/latest.tar)`` -> ``eval_mode`` -> ``generate_music_motion(mel, opt.dim_pose)`` -> reshape
``[T,13,2]`` (:217-218) -> (``smooth_motion(kernel=19)``, :126, with ``--smooth``) -> ``np.save(npy_path)``.

``--music_path`` takes the music in either form: the mel spectrogram itself - a ``.npy`` of shape ``[5400,128]`` (what
``extract_mel_feature`` :152-167 returns and the dataset stores as ``mel.npy``), or a directory of such files, which are sampled
as ONE batch - or the audio: a PCM ``.wav`` file, or a directory whose audio files are ``*.wav`` and which holds no ``*.npy``.
Audio goes through ``mel.load_audio`` (22050 Hz) and ``mel.MelSpectrogram.features`` on the GPU (csrc/dc_mel.hip) - several files
zero-padded to the longest and run as one batch with their lengths, a shorter file's mel rows behind its own length being 0 - and
from there into the code path a ``.npy`` takes; ``--save_mel PATH`` writes the mel that was computed (``[Tm,128]`` for one file,
``[B,Tm,128]`` for a directory).  ``load_mels`` itself still reads mels only.

What stays out (rendering is out of scope; the image has no librosa / cv2 / moviepy): mp3 decoding and the
video rendering.  The reference parses ``--npy_path`` but never writes it (``plot_music2motion`` :143 ignores the argument); here
it receives the keypoints: ``[T,13,2]`` for one clip, ``[B,T,13,2]`` for a directory.
"""
from __future__ import annotations

import argparse
import os
import re
from argparse import Namespace
from os.path import join as pjoin

import numpy as np

# opt.txt is what train.py writes (options/base_options.py:79-89): one "key: value" line per option between two banner lines.
# A value is a bool ("True" / "False"), a signed integer, a signed decimal with digits on both sides of the point, or text -
# anything else (a list, scientific notation) stays text, which is how the reference's reader (utils/get_opt.py:8-26, 37-48)
# types them too.
_LINE = re.compile(r"^\s*([^:\s][^:]*?)\s*:\s(.*?)\s*$")
_INT = re.compile(r"^[+-]?\d+$")
_DEC = re.compile(r"^[+-]?\d+\.\d+$")

# per dataset: (joints, frames per clip).  Only the conducting-motion dataset has a sampler here.
_DATASETS = {"ConductorMotion100": (13, 1800)}

# options the sampler reads, with the value an opt.txt that lacks them implies (utils/get_opt.py:50-59)
_SAMPLER_DEFAULTS = {"num_layers": 8, "latent_dim": 512, "diffusion_steps": 1000, "no_clip": False, "no_eff": False}


def _literal(text):
    if text in ("True", "False"):
        return text == "True"
    if _DEC.match(text):
        return float(text)
    if _INT.match(text):
        return int(text)
    return text


def get_opt(opt_path, device):
    """Reads a training run's ``opt.txt`` into the options object the sampling entry point needs (the role of
    utils/get_opt.py:29-105).  Every ``key: value`` line becomes an attribute (typed by `_literal`); on top of that the fields
    the sampler consumes are filled in: the denoiser's size (``num_layers``, ``latent_dim``, ``no_eff``, ``no_clip``),
    ``diffusion_steps``, the pose geometry of the dataset (``joints_num``, ``dim_pose``, ``max_motion_length``) and where the
    checkpoint lives (``model_dir`` = <checkpoints_dir>/<dataset_name>/<name>/model, trainers load ``latest.tar`` from it);
    inference is forced (``is_train`` / ``is_continue`` False, ``which_epoch`` "latest")."""
    print("Reading", opt_path)
    opt = Namespace(**_SAMPLER_DEFAULTS)
    with open(opt_path) as f:
        for raw in f:
            m = _LINE.match(raw)
            if m is None or raw.lstrip().startswith("-"):          # banner / blank lines
                continue
            setattr(opt, m.group(1), _literal(m.group(2)))
    for need in ("checkpoints_dir", "dataset_name", "name"):
        if not hasattr(opt, need):
            raise KeyError(f"{opt_path}: no '{need}' line")
    if opt.dataset_name not in _DATASETS:
        raise KeyError(f"Dataset not recognized: {opt.dataset_name!r} (this package samples {sorted(_DATASETS)})")
    opt.joints_num, opt.max_motion_length = _DATASETS[opt.dataset_name]
    opt.dim_pose = 2 * opt.joints_num
    opt.save_root = pjoin(opt.checkpoints_dir, opt.dataset_name, opt.name)
    opt.model_dir = pjoin(opt.save_root, "model")
    opt.which_epoch = "latest"
    opt.is_train = False
    opt.is_continue = False
    opt.device = device
    return opt


def build_models(opt, precision="fp16"):
    """tools/visualization.py:169-178."""
    from . import MotionTransformer
    return MotionTransformer(input_feats=opt.dim_pose, num_frames=opt.max_motion_length, num_layers=opt.num_layers,
                             latent_dim=opt.latent_dim, device=opt.device, no_clip=opt.no_clip, no_eff=opt.no_eff,
                             music_model_path=None, precision=precision)


def load_mels(music_path):
    """`--music_path`: one mel .npy [Tm,128], or a directory whose *.npy (sorted) form one batch [B,Tm,128]."""
    if os.path.isdir(music_path):
        files = sorted(f for f in os.listdir(music_path) if f.endswith('.npy'))
        if not files:
            raise FileNotFoundError(f"no .npy mel spectrograms under {music_path}")
        mels = [np.load(pjoin(music_path, f)) for f in files]
        if len({m.shape for m in mels}) != 1:
            raise ValueError(f"mel spectrograms under {music_path} differ in shape: {sorted({m.shape for m in mels})}")
        return np.stack(mels).astype(np.float32), files
    if not music_path.endswith('.npy'):
        raise ValueError("--music_path takes the mel spectrogram (.npy [5400,128]) or a directory of them: audio decoding "
                         "(librosa) is outside this package - run the reference's extract_mel_feature "
                         "(tools/visualization.py:152-167) and np.save its result")
    mel = np.load(music_path)
    if mel.ndim != 2 or mel.shape[1] != 128:
        raise ValueError(f"{music_path}: expected a [Tm,128] mel spectrogram, got {mel.shape}")
    return mel.astype(np.float32), [os.path.basename(music_path)]


def audio_files(music_path):
    """The WAV files `--music_path` names - the file itself, or the sorted *.wav of a directory that holds no *.npy -, or None when
    the path is `load_mels`'s to read."""
    if os.path.isdir(music_path):
        names = sorted(os.listdir(music_path))
        if any(f.endswith('.npy') for f in names):
            return None
        return [pjoin(music_path, f) for f in names if f.lower().endswith('.wav')] or None
    return [music_path] if music_path.lower().endswith('.wav') else None


def mels_from_audio(files, device, sr=22050):
    """WAV files -> (mel fp32 [Tm,128] for one file, [B,Tm,128] for several, their names): each file loaded at `sr`, the batch
    zero-padded to the longest and run through MelSpectrogram.features with the files' lengths."""
    from .mel import MelSpectrogram, load_audio
    waves = [load_audio(f, sr)[0] for f in files]
    batch = np.zeros((len(waves), max(w.shape[0] for w in waves)), np.float32)
    for i, w in enumerate(waves):
        batch[i, :w.shape[0]] = w
    mel = MelSpectrogram(device, sr).features(batch, [w.shape[0] for w in waves]).cpu().numpy()
    return (mel[0] if len(files) == 1 else mel), [os.path.basename(f) for f in files]


def make_parser():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument('--opt_path', type=str, required=True, help='Opt path')
    parser.add_argument('--music_path', type=str, required=True, help='mel spectrogram .npy [5400,128] (or a directory of them), or a PCM .wav file (or a directory of them)')
    parser.add_argument('--save_mel', type=str, default="", help='with audio in --music_path: where to np.save the mel that was computed')
    parser.add_argument('--motion_length', type=int, default=60, help='kept for compatibility (reference asserts <= 196)')
    parser.add_argument('--result_path', type=str, default="test_sample.gif", help='ignored: rendering is not part of this package')
    parser.add_argument('--npy_path', type=str, default="", help='Path to save the keypoints sequence')
    parser.add_argument('--gpu_id', type=int, default=0, help="which gpu to use")
    parser.add_argument('--model', type=str, default=None, help="checkpoint; default <model_dir>/latest.tar as in the reference")
    parser.add_argument('--smooth', action='store_true', help="Savitzky-Golay smoothing (kernel 19, order 5) as vis_motion applies it")
    parser.add_argument('--seed', type=int, default=None, help="seed of x_T (reproducible sampling)")
    parser.add_argument('--full_length', action='store_true',
                        help="conduct mels longer than one window (5400 frames = 60 s) whole, window by window around the frames "
                             "already generated (DDPMTrainer.generate_long_music_motion); without it only the first window is sampled")
    parser.add_argument('--joint', action='store_true',
                        help="with --full_length: sample all windows of a longer mel in ONE loop, blending their predictions over the "
                             "overlaps at every step (generate_long_music_motion, joint=True) instead of window by window")
    parser.add_argument('--blend', type=str, default="tent", choices=["tent", "uniform"], help="blend weights of --joint across an overlap")
    parser.add_argument('--precision', type=str, default="fp16", choices=["fp16", "mixed", "bf16x3", "bf16", "auto"])
    parser.add_argument('--steps', type=int, default=None, help="sample on this many of the schedule's timesteps (omitted: all of them)")
    parser.add_argument('--spacing', type=str, default="uniform", choices=["uniform", "logsnr"], help="how --steps picks them (use logsnr with dpmpp2m)")
    parser.add_argument('--solver', type=str, default="ddim", choices=["ddim", "dpmpp2m"], help="first-order DDIM or the second-order multistep update")
    parser.add_argument('--guidance_scale', type=float, default=None,
                        help="classifier-free guidance scale of the sampling loops (omitted: no guidance, the reference's sampling)")
    parser.add_argument('--takes', type=int, default=1,
                        help="samples per music: one output per take, --npy_path NAME.npy becomes NAME_take<j>.npy (the takes differ "
                             "through their noise and share the conditioning work of every step)")
    return parser


def main(argv=None):
    import torch
    from . import DDPMTrainer
    args = make_parser().parse_args(argv)
    if args.gpu_id == -1:
        raise SystemExit("this package has no CPU path: --gpu_id must name an MI355X")
    device = torch.device('cuda:%d' % args.gpu_id)
    opt = get_opt(args.opt_path, device)
    assert args.motion_length <= 196
    torch.cuda.set_device(device)
    encoder = build_models(opt, precision=args.precision).to(device)
    trainer = DDPMTrainer(opt, encoder)
    trainer.load(args.model if args.model else pjoin(opt.model_dir, 'latest.tar'))
    trainer.eval_mode()
    trainer.to(opt.device)
    gkw = {} if args.guidance_scale is None else {"guidance_scale": args.guidance_scale}
    if args.steps is not None or args.solver != "ddim":
        gkw.update(steps=args.steps, spacing=args.spacing, solver=args.solver)
    if args.takes < 1:
        raise SystemExit("--takes must be at least 1")
    with torch.no_grad():
        wavs = audio_files(args.music_path)
        mel, names = load_mels(args.music_path) if wavs is None else mels_from_audio(wavs, device)
        if args.save_mel:
            if wavs is None:
                raise SystemExit("--save_mel writes the mel computed from audio: --music_path names a mel already")
            np.save(args.save_mel, mel)
            print("saved", args.save_mel, mel.shape)
        if args.takes > 1:
            if args.full_length and mel.shape[-2] > 3 * opt.max_motion_length:
                raise SystemExit("--takes samples one window per take: it does not combine with --full_length on a longer mel")
            gkw["takes"] = args.takes
        # [B, T, 26] on the device; --smooth: smooth_motion(kernel=19) (:126) happens in the loop's final write
        if args.joint and not args.full_length:
            raise SystemExit("--joint blends the windows of a longer mel: it goes with --full_length")
        if args.full_length and mel.shape[-2] > 3 * opt.max_motion_length:
            jkw = {"joint": True, "blend": args.blend} if args.joint else {}      # (without --joint the trainer is called as before)
            pred_motions = trainer.generate_long_music_motion(mel, opt.dim_pose, seed=args.seed, smooth=19 if args.smooth else None, **gkw, **jkw)
        else:
            pred_motions = trainer.generate_music_motion(mel, opt.dim_pose, seed=args.seed, smooth=19 if args.smooth else None, **gkw)
        B, T = pred_motions.shape[0], pred_motions.shape[1]
        motion = pred_motions.view(B, T, 13, 2).cpu().numpy()
    if args.takes > 1:      # take-major rows (generate_music_motion): one output per take, each shaped as a single take's
        per_take = motion.reshape(args.takes, B // args.takes, T, 13, 2)
        outs = [m[0] if mel.ndim == 2 else m for m in per_take]
        print(" #%d frames x %d clip(s) x %d takes: %s" % (T, B // args.takes, args.takes, ", ".join(names)))
        if args.npy_path:
            stem, ext = os.path.splitext(args.npy_path)
            for j, o in enumerate(outs):
                np.save("%s_take%d%s" % (stem, j, ext or ".npy"), o)
                print("saved", "%s_take%d%s" % (stem, j, ext or ".npy"), o.shape)
        return np.stack(outs)
    out = motion[0] if mel.ndim == 2 else motion
    print(" #%d frames x %d clip(s): %s" % (T, B, ", ".join(names)))
    if args.npy_path:
        np.save(args.npy_path, out)
        print("saved", args.npy_path, out.shape)
    return out


if __name__ == '__main__':
    main()
