"""Seeded synthetic checkpoint and inputs (numpy only).

No trained checkpoint ships with the reference (README.md:125 points at external
downloads), and a freshly constructed reference model outputs exactly 0 because of
``zero_module`` (Diffusion_Stage/models/transformer.py:44-50,65,165,443).  Parity
tests, ``smoke()`` and ``bench.py`` therefore regenerate the same checkpoint and
inputs from seeds on whichever box they run, instead of committing 24 MB of weights.

Each tensor gets its own counter-based stream keyed by (seed, crc32(name)), so the
values do not depend on generation order.
"""
from __future__ import annotations

import zlib
from collections import OrderedDict

import numpy as np

from .param_spec import DenoiserConfig, param_shapes


def _rng(seed: int, tag: str, index: int = 0) -> np.random.Generator:
    key = [int(seed) & 0xFFFFFFFF, zlib.crc32(tag.encode()) & 0xFFFFFFFF]
    ctr = [int(index) & 0xFFFFFFFFFFFFFFFF, 0, 0, 0]
    return np.random.Generator(np.random.Philox(key=key, counter=ctr))


def synthetic_state_dict(cfg: DenoiserConfig = DenoiserConfig(), seed: int = 0):
    """name -> np.ndarray for every state_dict entry of the denoiser.

    Linear/conv weights and biases ~ U(-1/sqrt(fan_in), 1/sqrt(fan_in)) (the bound
    PyTorch's default initialiser uses), *including* the tensors the reference
    zero-initialises - otherwise every Stylization block, FFN and the output
    projection contribute nothing and parity would be vacuous.  Norm affine and
    BatchNorm running statistics are non-trivial.
    """
    out = OrderedDict()
    for name, shape in param_shapes(cfg).items():
        g = _rng(seed, name)
        if name.endswith("num_batches_tracked"):
            out[name] = np.asarray(1000, dtype=np.int64)
            continue
        leaf = name.rsplit(".", 1)[-1]
        if name == "sequence_embedding":
            a = g.standard_normal(shape)
        elif leaf == "running_mean":
            a = 0.1 * g.standard_normal(shape)
        elif leaf == "running_var":
            a = g.uniform(0.5, 1.5, shape)
        elif len(shape) == 1 and (".norm." in name or "text_norm" in name
                                  or "conv2d_layer.1." in name or "residual.1." in name
                                  or "conv4.1." in name):
            # LayerNorm / BatchNorm affine
            a = (1.0 + 0.1 * g.standard_normal(shape)) if leaf == "weight" \
                else 0.1 * g.standard_normal(shape)
        else:
            if leaf == "weight":
                fan_in = int(np.prod(shape[1:]))
            else:  # bias: fan_in of the sibling weight
                wshape = param_shapes(cfg)[name[:-4] + "weight"]
                fan_in = int(np.prod(wshape[1:]))
            bound = 1.0 / np.sqrt(fan_in)
            a = g.uniform(-bound, bound, shape)
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def synthetic_mel(clip: int, n_frames: int = 5400, n_bins: int = 128, seed: int = 1):
    """U[0,1) mel for clip index ``clip`` (real mels are normalised to [0,1]:
    Diffusion_Stage/tools/visualization.py:165)."""
    return _rng(seed, "mel", clip).random((n_frames, n_bins), dtype=np.float32)


def synthetic_noise(clip: int, T: int = 1800, P: int = 26, seed: int = 2):
    """x_T ~ N(0,1) for clip index ``clip``."""
    return _rng(seed, "x_T", clip).standard_normal((T, P), dtype=np.float32)


def synthetic_music_features(clip: int, T: int = 1800, C: int = 64, seed: int = 3):
    """Stand-in for MusicEncoder output [T,64] (used where encode_music is not under
    test): roughly unit-scale, like a BatchNorm'ed conv output."""
    return _rng(seed, "xf", clip).standard_normal((T, C), dtype=np.float32)


def batch_mel(B, n_frames=5400, n_bins=128, seed=1, first=0):
    return np.stack([synthetic_mel(first + b, n_frames, n_bins, seed) for b in range(B)])


def batch_noise(B, T=1800, P=26, seed=2, first=0):
    return np.stack([synthetic_noise(first + b, T, P, seed) for b in range(B)])


def batch_music_features(B, T=1800, C=64, seed=3, first=0):
    return np.stack([synthetic_music_features(first + b, T, C, seed) for b in range(B)])


def stress_state_dict(cfg: DenoiserConfig = DenoiserConfig(), seed: int = 0):
    """A "trained-like" stress variant of the synthetic checkpoint: trained denoisers are not at initialisation
    scale, so the parity tests also run on a draw with larger modulation / output weights, spread-out
    LayerNorm gains and a few outlier channels (tests/golden/g8_robust.npz):
      * StylizationBlock ``emb_layers`` / ``out_layers``, ``ffn.linear2`` and ``out`` weights x 3;
      * every LayerNorm gain log-normal with sigma = 0.5;
      * four 10x outlier channels in ``sequence_embedding`` and in ``joint_embed``.
    """
    sd = synthetic_state_dict(cfg, seed)
    for name in sd:
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "weight" and (".emb_layers.1." in name or ".out_layers.2." in name or name.endswith("ffn.linear2.weight")
                                 or name == "out.weight"):
            sd[name] = np.ascontiguousarray(sd[name] * 3.0, dtype=np.float32)
        elif leaf == "weight" and len(sd[name].shape) == 1 and (".norm." in name or "text_norm" in name):
            g = _rng(seed, "stress:" + name)
            sd[name] = np.exp(0.5 * g.standard_normal(sd[name].shape)).astype(np.float32)
    ch = _rng(seed, "stress:outliers").choice(cfg.latent_dim, size=8, replace=False)
    se = sd["sequence_embedding"].copy()
    se[:, ch[:4]] *= 10.0
    sd["sequence_embedding"] = se
    je = sd["joint_embed.weight"].copy()
    je[ch[4:], :] *= 10.0
    sd["joint_embed.weight"] = je
    return sd


def smooth_mel(clip: int, n_frames: int = 5400, n_bins: int = 128, seed: int = 1):
    """A mel in [0,1] with the smoothness of a real spectrogram (white noise low-pass filtered along time and
    frequency, then min-max normalised as tools/visualization.py:165 does) - ``synthetic_mel`` is white."""
    a = _rng(seed, "smooth_mel", clip).standard_normal((n_frames + 64, n_bins + 16))
    kt = np.hanning(65)
    kf = np.hanning(17)
    a = np.apply_along_axis(lambda v: np.convolve(v, kt / kt.sum(), mode="valid"), 0, a)
    a = np.apply_along_axis(lambda v: np.convolve(v, kf / kf.sum(), mode="valid"), 1, a)
    a = a[:n_frames, :n_bins]
    a = (a - a.min()) / (a.max() - a.min())
    return np.ascontiguousarray(a, dtype=np.float32)


def batch_step_noise(S, B, T=1800, P=26, seed=4, first=0):
    """Per-iteration DDIM noise z_i ~ N(0,1) (eta > 0), [S, B, T, P]: iteration i of clip b has its own stream."""
    return np.stack([np.stack([_rng(seed, f"z{i}", first + b).standard_normal((T, P), dtype=np.float32) for b in range(B)])
                     for i in range(S)])


def synthetic_motion_encoder_state_dict(seed: int = 0):
    """name -> np.ndarray for every state_dict entry of MotionEncoder_STGCN (motion_encoder.py): conv weights and biases
    ~ U(-1/sqrt(fan_in), 1/sqrt(fan_in)), BatchNorm affines and running statistics away from the identity, `st_gcn.A` the
    skeleton's normalised adjacency and edge importances 1 + 0.3 N(0, 1) (all-ones importances would leave that path untested)."""
    from .motion_encoder import motion_encoder_shapes, skeleton_adjacency
    out = OrderedDict()
    shapes = motion_encoder_shapes()
    for name, shape in shapes.items():
        g = _rng(seed, "stgcn:" + name)
        leaf = name.rsplit(".", 1)[-1]
        if leaf == "num_batches_tracked":
            out[name] = np.asarray(1000, dtype=np.int64)
            continue
        if name == "st_gcn.A":
            a = skeleton_adjacency()
        elif ".edge_importance." in name:
            a = 1.0 + 0.3 * g.standard_normal(shape)
        elif leaf == "running_mean":
            a = 0.1 * g.standard_normal(shape)
        elif leaf == "running_var":
            a = g.uniform(0.5, 1.5, shape)
        elif len(shape) == 1 and ("bn." in name or ".tcn.0." in name or ".tcn.3." in name or name.startswith("fc.1.")):
            a = (1.0 + 0.1 * g.standard_normal(shape)) if leaf == "weight" else 0.1 * g.standard_normal(shape)
        else:
            wshape = shapes[name if leaf == "weight" else name[:-4] + "weight"]
            bound = 1.0 / np.sqrt(int(np.prod(wshape[1:])))
            a = g.uniform(-bound, bound, shape)
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


MOTION_ENCODER_VARIANTS = ("seeded", "sparse_importance", "dense_adjacency", "bn_stress", "identity")


def motion_encoder_weight_variant(kind: str, seed: int = 1):
    """synthetic_motion_encoder_state_dict(seed) with one part of the weights moved to an edge the seeded weights never reach:
      seeded             unchanged;
      sparse_importance  edge importances with about a quarter of the entries zeroed and another quarter negated, plus in block l
                         the off-diagonal entries of column l zeroed and its self link negative (odd l) or the whole column l zeroed (even l);
      dense_adjacency    `st_gcn.A` a dense, non-symmetric random matrix (mixed signs) instead of the skeleton's;
      bn_stress          every BatchNorm with gains of both signs, running_var log-uniform in [1e-4, 2] (so eps = 1e-5 moves the
                         scale by up to 5 %; the gain scales with sqrt(var) so activations stay O(1)) and running_mean ~ 2 N(0, 1);
      identity           all-ones importances and identity BatchNorms (the control)."""
    if kind not in MOTION_ENCODER_VARIANTS:
        raise ValueError(f"unknown motion encoder weight variant {kind!r}")
    sd = synthetic_motion_encoder_state_dict(seed)
    g = _rng(seed, "stgcn_variant:" + kind)
    n = 13
    bns = sorted({k.rsplit(".", 1)[0] + "." for k in sd if k.endswith("running_var")})
    if kind == "sparse_importance":
        for l in range(10):
            e = sd[f"st_gcn.edge_importance.{l}"][0]
            u = g.random((n, n))
            e[u < 0.25] = 0.0
            e[(u >= 0.25) & (u < 0.5)] *= -1.0
            if l % 2:
                e[np.arange(n) != l, l] = 0.0
                e[l, l] = -0.8            # a negative self link as the column's only entry
            else:
                e[:, l] = 0.0
    elif kind == "dense_adjacency":
        sd["st_gcn.A"] = g.uniform(-0.15, 0.3, (1, n, n)).astype(np.float32)
    elif kind == "bn_stress":
        for p in bns:
            c = sd[p + "running_var"].shape[0]
            var = np.exp(g.uniform(np.log(1e-4), np.log(2.0), c))
            sd[p + "running_var"] = var.astype(np.float32)
            sd[p + "weight"] = (np.where(g.random(c) < 0.5, -1.0, 1.0) * g.uniform(0.7, 1.3, c) * np.sqrt(var)).astype(np.float32)
            sd[p + "running_mean"] = (2.0 * g.standard_normal(c)).astype(np.float32)
    elif kind == "identity":
        for l in range(10):
            sd[f"st_gcn.edge_importance.{l}"] = np.ones((1, n, n), np.float32)
        for p in bns:
            c = sd[p + "running_var"].shape[0]
            sd[p + "weight"], sd[p + "running_var"] = np.ones(c, np.float32), np.ones(c, np.float32)
            sd[p + "bias"], sd[p + "running_mean"] = np.zeros(c, np.float32), np.zeros(c, np.float32)
    return sd


MUSIC_ENCODER_VARIANTS = ("seeded", "bn_stress", "dead_channels", "identity")
MUSIC_ENCODER_DEAD_BIAS = -100.0          # BatchNorm bias of a dead channel: its pre-activation stays negative for any mel in [0, 1]


def music_encoder_weight_variant(kind: str, seed: int = 1):
    """synthetic_state_dict() (the seeded denoiser checkpoint, seed 0) with only its `music_encoder.*` entries replaced:
      seeded         those of synthetic_state_dict(seed=seed);
      bn_stress      ... and every BatchNorm (`residual.1` and `conv4.1` included) with gains of both signs, running_var log-uniform in
                     [1e-4, 2] (the gain scales with sqrt(var) so activations stay O(1)) and running_mean ~ 2 N(0, 1);
      dead_channels  ... and channels c % 4 == 1 of every ReLU layer pinned to zero by a BatchNorm bias of MUSIC_ENCODER_DEAD_BIAS (the
                     1x1 residual's BatchNorm of conv2.0 zeroed on the same channels, so the sum is 0 as well): the same channels in
                     every layer, so they are exactly 0 in every pool window - ties with each other and with the other channels' zeros;
      identity       ... and identity BatchNorms (the control)."""
    if kind not in MUSIC_ENCODER_VARIANTS:
        raise ValueError(f"unknown music encoder weight variant {kind!r}")
    sd = synthetic_state_dict(seed=0)
    for k, v in synthetic_state_dict(seed=seed).items():
        if k.startswith("music_encoder."):
            sd[k] = v.copy()
    g = _rng(seed, "music_encoder_variant:" + kind)
    bns = sorted({k.rsplit(".", 1)[0] + "." for k in sd if k.startswith("music_encoder.") and k.endswith("running_var")})
    if kind == "bn_stress":
        for p in bns:
            c = sd[p + "running_var"].shape[0]
            var = np.exp(g.uniform(np.log(1e-4), np.log(2.0), c))
            sd[p + "running_var"] = var.astype(np.float32)
            sd[p + "weight"] = (np.where(g.random(c) < 0.5, -1.0, 1.0) * g.uniform(0.7, 1.3, c) * np.sqrt(var)).astype(np.float32)
            sd[p + "running_mean"] = (2.0 * g.standard_normal(c)).astype(np.float32)
    elif kind == "dead_channels":
        for p in bns:
            dead = np.arange(sd[p + "bias"].shape[0]) % 4 == 1
            if ".conv2d_layer.1." in p:
                sd[p + "bias"][dead] = MUSIC_ENCODER_DEAD_BIAS
            elif ".residual.1." in p:
                sd[p + "weight"][dead] = 0.0
                sd[p + "bias"][dead] = 0.0
    elif kind == "identity":
        for p in bns:
            c = sd[p + "running_var"].shape[0]
            sd[p + "weight"], sd[p + "running_var"] = np.ones(c, np.float32), np.ones(c, np.float32)
            sd[p + "bias"], sd[p + "running_mean"] = np.zeros(c, np.float32), np.zeros(c, np.float32)
    return sd


def synthetic_motion(B, T, seed=5, first=0):
    """[B, T, 13, 2] fp32 smooth pose-like tracks (random walks around a random rest pose, in [-1, 1]-ish units)."""
    out = np.empty((B, T, 13, 2), np.float32)
    for b in range(B):
        g = _rng(seed, "motion", first + b)
        rest = g.uniform(-0.6, 0.6, (1, 13, 2))
        walk = np.cumsum(0.02 * g.standard_normal((T, 13, 2)), axis=0)
        out[b] = rest + walk
    return out


def synthetic_generated_motion(real, seed=13):
    """A stand-in for sampled motion beside `real` [n, T, 13, 2]: clip i plus a smooth random-walk perturbation whose size grows
    from 0.5x to 2x over the clips (so the latent-space scores between the two sets are non-trivial and differ per clip)."""
    n = real.shape[0]
    scale = np.linspace(0.5, 2.0, n)
    out = np.empty_like(real, dtype=np.float32)
    for i in range(n):
        walk = np.cumsum(0.03 * _rng(seed, "gen_motion", i).standard_normal(real.shape[1:]), axis=0)
        out[i] = real[i] + walk * scale[i]
    return out


def array_digest(a):
    """(sum, sum of |x|, sum of x * index) in float64 of an array's values: a compact fingerprint that pins a regenerable input
    without storing it."""
    x = np.asarray(a, np.float64).ravel()
    return np.array([x.sum(), np.abs(x).sum(), (x * np.arange(x.size)).sum()])


# gains of the seeded fuse head over PyTorch's default initialiser bound, and its last bias (see synthetic_m2snet_state_dict)
M2SNET_FUSE_GAIN = (6.0, 4.0, 8.0)
M2SNET_FUSE_LAST_BIAS = -1.0


def synthetic_m2snet_state_dict(seed: int = 0):
    """name -> np.ndarray for every state_dict entry of M2SNet (m2snet.py), in the reference module's order: the `music_encoder.*`
    entries of synthetic_state_dict(seed), synthetic_motion_encoder_state_dict(seed) under `motion_encoder.`, and a seeded fuse
    head.  With weights at the initialiser's scale every logit of the head lands in a narrow positive band - every frame "in
    sync", which tests nothing about the 0.5 threshold - so the head's weights are U(-1/sqrt(fan_in), 1/sqrt(fan_in)) times
    M2SNET_FUSE_GAIN per layer and the last bias is M2SNET_FUSE_LAST_BIAS: on the fixture's inputs (tools/make_golden_m2snet.py
    asserts it) the logits span more than [-2, 2] with at least 20 % of the frames on each side of 0, and both hidden layers have
    dead and live ReLU units."""
    from .m2snet import m2snet_shapes
    den = synthetic_state_dict(seed=seed)
    mot = synthetic_motion_encoder_state_dict(seed)
    out = OrderedDict()
    for name, shape in m2snet_shapes().items():
        if name.startswith("music_encoder."):
            out[name] = den[name]
        elif name.startswith("motion_encoder."):
            out[name] = mot[name[len("motion_encoder."):]]
        else:
            layer = int(name.split(".")[1]) // 2
            fan_in = 128 if layer == 0 else 64
            a = _rng(seed, "m2snet:" + name).uniform(-1.0, 1.0, shape) * (M2SNET_FUSE_GAIN[layer] / np.sqrt(fan_in))
            if name == "fuse_layer.4.bias":
                a = np.full(shape, M2SNET_FUSE_LAST_BIAS)
            out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


# the seeded M2S-GAN decoder (see synthetic_m2sgan_state_dict): gain of the temporal blocks' weight-norm magnitudes, size of the
# BatchNorm shifts that pin a few units dead / live, gains of TCN.linear and the three fc layers, gain of the noise branch
M2SGAN_CONV_GAIN = 0.5
M2SGAN_PIN_SHIFT = 6.0
M2SGAN_HEAD_GAIN = (1.0, 1.5, 2.0, 3.0)
M2SGAN_NOISE_GAIN = 3.0


def synthetic_m2sgan_state_dict(seed: int = 0):
    """name -> np.ndarray for every state_dict entry of the M2S-GAN Generator (generator.py), in the reference module's order: the
    `music_encoder.*` entries of synthetic_state_dict(seed) and a seeded decoder.  At the reference's own initialiser scale
    (normal_(0, 0.01)) every pose sits within 0.03 of 0.5, which tests nothing, so: `weight_v` ~ U(-1, 1) / sqrt(fan_in) and
    `weight_g` = M2SGAN_CONV_GAIN U(0.6, 1.6) - not |weight_v| -, BatchNorm affines and running statistics away from the identity,
    with two units per BatchNorm of the temporal blocks shifted by -/+ M2SGAN_PIN_SHIFT (dead / live on every frame), the head's
    weights U(-1, 1) / sqrt(fan_in) times M2SGAN_HEAD_GAIN per layer and the noise branch's times M2SGAN_NOISE_GAIN.  On the
    fixture's inputs (tools/make_golden_m2sgan.py asserts it) the poses span more than [0.2, 0.8], every ReLU of the temporal blocks
    has dead, live and switching units, and the latent moves the poses by more than 1e-2.  The `net.N.*` aliases equal their twins."""
    from .generator import ALIASES, m2sgan_shapes
    den = synthetic_state_dict(seed=seed)
    shapes = m2sgan_shapes()
    head = {"tcn.TCN.tcn.linear": 0, "tcn.fc.0": 1, "tcn.fc.2": 2, "tcn.fc.4": 3}
    out = OrderedDict()
    for name, shape in shapes.items():
        if name.startswith("music_encoder."):
            out[name] = den[name]
            continue
        canon = name
        for alias, twin in ALIASES:
            canon = canon.replace(f".{alias}.", f".{twin}.")
        if canon != name:
            out[name] = out[canon]
            continue
        g = _rng(seed, "m2sgan:" + name)
        mod, leaf = name.rsplit(".", 1)
        bn = ".bn" in name or name.startswith("noise_BN")
        if leaf == "num_batches_tracked":
            out[name] = np.asarray(1000, dtype=np.int64)
            continue
        if leaf == "running_mean":
            a = 0.1 * g.standard_normal(shape)
        elif leaf == "running_var":
            a = g.uniform(0.5, 1.5, shape)
        elif bn:
            a = (1.0 + 0.2 * g.standard_normal(shape)) if leaf == "weight" else 0.2 * g.standard_normal(shape)
            if leaf == "bias" and ".bn" in name:
                pin = _rng(seed, "m2sgan:pin:" + name).choice(shape[0], size=4, replace=False)
                a[pin[:2]], a[pin[2:]] = -M2SGAN_PIN_SHIFT, M2SGAN_PIN_SHIFT
        elif leaf == "weight_g":
            a = M2SGAN_CONV_GAIN * g.uniform(0.6, 1.6, shape)
        else:
            wshape = shapes[mod + (".weight_v" if (mod + ".weight_v") in shapes else ".weight")]
            # (ConvTranspose1d weights are [cin, cout, k]: fan_in = cin k)
            fan_in = wshape[0] * wshape[2] if name.startswith("noise_convTranspose") else int(np.prod(wshape[1:]))
            gain = M2SGAN_HEAD_GAIN[head[mod]] if mod in head else (M2SGAN_NOISE_GAIN if name.startswith("noise_convTranspose") else 1.0)
            a = g.uniform(-1.0, 1.0, shape) * (gain / np.sqrt(fan_in))
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out


# gain of the seeded BiLSTM decoder over torch's default ranges: U(+-1 / sqrt(128)) for the LSTM, U(+-1 / sqrt(fan_in)) for a Linear of
# the head (see synthetic_bilstm_state_dict)
BILSTM_GAIN = 3.0
BILSTM_HH_GAIN = 1.5      # on top of it for weight_hh: how far along a clip a frame is felt


def synthetic_bilstm_state_dict(seed: int = 0, input_size: int = 128):
    """name -> np.ndarray for every state_dict entry of PoseDecoderBiLSTM(input_size, 26) (generator.bilstm_shapes), in the reference
    module's order.  Every entry is drawn from torch's default range - U(-1, 1) / sqrt(128) for the LSTM of 128 hidden units,
    U(-1, 1) / sqrt(fan_in) for a Linear of the head - times BILSTM_GAIN, the recurrent weights times BILSTM_HH_GAIN more (at 1 the far end of a 30-frame clip moves a pose by
    3e-4, at 2 by 0.2 - the recurrence stops contracting): at the default range the gates stay in their linear part and the poses near 0.5; at this one (tools/make_golden_bilstm.py asserts it)
    every gate has pre-activations of both signs, the poses span more than [0.2, 0.8] and a frame's pose depends on the far end of
    the clip in both directions."""
    from .generator import bilstm_shapes
    shapes = bilstm_shapes(input_size)
    out = OrderedDict()
    for name, shape in shapes.items():
        g = _rng(seed, f"bilstm{input_size}:" + name)
        fan_in = 128 if name.startswith("LSTM.") else shapes[name.rsplit(".", 1)[0] + ".weight"][1]
        gain = BILSTM_GAIN * (BILSTM_HH_GAIN if "weight_hh" in name else 1.0)
        out[name] = np.ascontiguousarray(g.uniform(-1.0, 1.0, shape) * (gain / np.sqrt(fan_in)), dtype=np.float32)
    return out


def synthetic_m2sgan_bilstm_state_dict(seed: int = 0):
    """The CNN-LSTM baseline's Generator (generator.m2sgan_bilstm_shapes: `self.tcn = PoseDecoderBiLSTM(128, 26)`): the encoder and
    noise branch entries of synthetic_m2sgan_state_dict(seed) - the same tensors, so its features equal the TCN generator's - and
    synthetic_bilstm_state_dict(seed, 128) under `tcn.`, in the reference module's order."""
    from .generator import m2sgan_bilstm_shapes
    gan, dec = synthetic_m2sgan_state_dict(seed), synthetic_bilstm_state_dict(seed, 128)
    return OrderedDict((k, dec[k[4:]] if k.startswith("tcn.") else gan[k]) for k in m2sgan_bilstm_shapes())


# gains of the seeded critic over PyTorch's default initialiser bound, per convolution stage and per fc layer (see
# synthetic_discriminator_state_dict)
DISCRIMINATOR_CONV_GAIN = (6.0, 2.0, 2.0)
DISCRIMINATOR_FC_GAIN = (2.0, 3.0, 4.0)


def synthetic_discriminator_state_dict(seed: int = 0):
    """name -> np.ndarray for the 12 state_dict entries of the M2S-GAN critic (discriminator.py), in the reference module's order:
    weights U(-1, 1) / sqrt(fan_in) times DISCRIMINATOR_CONV_GAIN / DISCRIMINATOR_FC_GAIN, biases U(-1, 1) / sqrt(fan_in).  The
    gains keep the ReLUs switching and the pooled maxima away from 0 on pose-like inputs (values around 0.5 that move by
    hundredths per frame), so that a wrong tap, padding or pooling window moves the score (tools/make_golden_rhythm.py asserts it)."""
    from .discriminator import discriminator_shapes
    shapes = discriminator_shapes()
    out = OrderedDict()
    for name, shape in shapes.items():
        mod, leaf = name.rsplit(".", 1)
        wshape = shapes[mod + ".weight"]
        fan_in = int(np.prod(wshape[1:]))
        idx = int(mod.rsplit(".", 1)[1])
        gain = DISCRIMINATOR_CONV_GAIN[idx // 3] if mod.startswith("motion_encoder") else DISCRIMINATOR_FC_GAIN[idx // 2]
        a = _rng(seed, "discriminator:" + name).uniform(-1.0, 1.0, shape) * ((gain if leaf == "weight" else 1.0) / np.sqrt(fan_in))
        out[name] = np.ascontiguousarray(a, dtype=np.float32)
    return out
