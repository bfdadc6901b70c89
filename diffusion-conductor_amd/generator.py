"""The M2S-GAN generator, the baseline the diffusion denoiser is compared against, as a second model of the evaluation.

``Generator`` is a drop-in for the reference's class of the same name (Contrastive_Stage/models/Generator.py:52-86) in eval mode:
``forward(mel, noise)`` maps a mel [B, Tm, 128] and a latent [B, Ln, 8] to poses [B, T, 13, 2], T = (Tm-1)//3+1 = 30 Ln.  Its
MusicEncoder runs on the kernels of csrc/dc_music.hip with this checkpoint's own ``music_encoder.*`` weights, the noise branch,
the six dilated temporal blocks (models/TCN.py) and the head on csrc/dc_m2sgan.hip (dc_m2sgan_* in include/dc_ddim.h).
``PoseDecoderBiLSTM`` (Generator.py:7-31) is the decoder of the two CNN-LSTM baselines - ``Generator(decoder="bilstm")``, the
reference's `self.tcn = PoseDecoderBiLSTM(128, 26)` (:58), and ``Generator_CVPR_LSTM`` (:89-100) - on csrc/dc_bilstm.hip (dc_bilstm_*).
``GeneratorBaseline`` gives it a trainer's shape, so ``evaluate.evaluate_dataset`` scores it like the denoiser
(Contrastive_Stage/M2SGAN_eval.py scores it with the same latent metrics and the same M2SNet).  There is no CPU path.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from .m2snet import strip_module_prefix
from .motion_encoder import _to_numpy

N_BLOCKS, CHANNELS, KERNEL, LATENT_DIM, FRAMES_PER_STEP = 6, 64, 5, 8, 30
LSTM_HIDDEN, LSTM_MAX_INPUT = 128, 128      # nn.LSTM(In, 128, num_layers=2, bidirectional), Generator.py:20; In as dc_bilstm takes it
NOISE_CONVS = ((8, 16, 3), (16, 16, 11), (16, 32, 5), (32, 64, 6))      # ConvTranspose1d (cin, cout, kernel), Generator.py:60-63
BLOCK = "tcn.TCN.tcn.tcn.network.{}."
# a block's layers under their nn.Sequential names (TCN.py:36-38): the same tensors a second time
ALIASES = (("net.0", "conv1"), ("net.2", "bn1"), ("net.5", "conv2"), ("net.7", "bn2"))


def _bn(e, p, c=CHANNELS):
    for leaf in ("weight", "bias", "running_mean", "running_var"):
        e[f"{p}.{leaf}"] = (c,)
    e[f"{p}.num_batches_tracked"] = ()


def m2sgan_shapes():
    """name -> shape of every state_dict entry of the reference Generator (278 entries, in the module's order: music_encoder, tcn,
    noise_convTranspose, noise_BN), the `net.N.*` aliases of the temporal blocks and the BatchNorm counters included."""
    from .param_spec import param_shapes
    e = OrderedDict((k, v) for k, v in param_shapes().items() if k.startswith("music_encoder."))
    for i in range(N_BLOCKS):
        p = BLOCK.format(i)
        cin = 2 * CHANNELS if i == 0 else CHANNELS
        for names in (("conv1", "bn1", "conv2", "bn2"), ("net.0", "net.2", "net.5", "net.7")):
            for conv, bn, c in ((names[0], names[1], cin), (names[2], names[3], CHANNELS)):
                e[f"{p}{conv}.bias"] = (CHANNELS,)
                e[f"{p}{conv}.weight_g"] = (CHANNELS, 1, 1)
                e[f"{p}{conv}.weight_v"] = (CHANNELS, c, KERNEL)
                _bn(e, p + bn)
        if i == 0:
            e[p + "downsample.weight"] = (CHANNELS, cin, 1)
            e[p + "downsample.bias"] = (CHANNELS,)
    e["tcn.TCN.tcn.linear.weight"], e["tcn.TCN.tcn.linear.bias"] = (CHANNELS, CHANNELS), (CHANNELS,)
    for i, n in ((0, CHANNELS), (2, CHANNELS), (4, 26)):
        e[f"tcn.fc.{i}.weight"], e[f"tcn.fc.{i}.bias"] = (n, CHANNELS), (n,)
    for i, (cin, cout, k) in enumerate(NOISE_CONVS):
        e[f"noise_convTranspose.{2 * i}.weight"], e[f"noise_convTranspose.{2 * i}.bias"] = (cin, cout, k), (cout,)
    _bn(e, "noise_BN")
    return e


def bilstm_shapes(input_size):
    """name -> shape of every state_dict entry of the reference PoseDecoderBiLSTM(input_size, 26) (Generator.py:17-25), in the module's
    order: nn.LSTM's per layer and direction, then the head `out`."""
    if not 1 <= int(input_size) <= LSTM_MAX_INPUT:
        raise ValueError(f"the BiLSTM decoder takes 1 .. {LSTM_MAX_INPUT} features per frame, not {input_size}")
    e = OrderedDict()
    for layer in range(2):
        for suffix in ("", "_reverse"):
            e[f"LSTM.weight_ih_l{layer}{suffix}"] = (4 * LSTM_HIDDEN, 2 * LSTM_HIDDEN if layer else int(input_size))
            e[f"LSTM.weight_hh_l{layer}{suffix}"] = (4 * LSTM_HIDDEN, LSTM_HIDDEN)
            e[f"LSTM.bias_ih_l{layer}{suffix}"] = (4 * LSTM_HIDDEN,)
            e[f"LSTM.bias_hh_l{layer}{suffix}"] = (4 * LSTM_HIDDEN,)
    for i, (n, k) in ((0, (CHANNELS, 2 * LSTM_HIDDEN)), (2, (CHANNELS, CHANNELS)), (4, (26, CHANNELS))):
        e[f"out.{i}.weight"], e[f"out.{i}.bias"] = (n, k), (n,)
    return e


def m2sgan_bilstm_shapes():
    """name -> shape of every state_dict entry of the reference Generator with `self.tcn = PoseDecoderBiLSTM(128, 26)` (Generator.py:58,
    the CNN-LSTM baseline), in the module's order: music_encoder, tcn, noise_convTranspose, noise_BN."""
    gan = m2sgan_shapes()
    e = OrderedDict((k, v) for k, v in gan.items() if k.startswith("music_encoder."))
    e.update(("tcn." + k, v) for k, v in bilstm_shapes(2 * CHANNELS).items())
    e.update((k, v) for k, v in gan.items() if k.startswith("noise_"))
    return e


def _check_state_dict(what, spec, state_dict, strict):
    """nn.Module.load_state_dict's key and shape errors for the module `what`."""
    missing = [k for k in spec if k not in state_dict]
    unexpected = [k for k in state_dict if k not in spec]
    if strict and (missing or unexpected):
        raise RuntimeError(f"Error(s) in loading state_dict for {what}: missing keys {missing}, unexpected keys {unexpected}")
    for k, v in state_dict.items():
        if k in spec and tuple(np.shape(_to_numpy(v))) != spec[k]:
            raise RuntimeError(f"size mismatch for {k}: got {tuple(np.shape(_to_numpy(v)))}, expected {spec[k]}")


def _device_tensor(x, last, what, device):
    import torch
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    if t.dim() != 3 or t.shape[2] != last:
        raise ValueError(f"{what} must be [B, *, {last}], got {tuple(t.shape)}")
    return t.to(device, torch.float32).contiguous()


class PoseDecoderBiLSTM:
    """Eval-mode PoseDecoderBiLSTM(input_size, output_size) of the reference (Generator.py:7-31) on the MI355X: features fp32
    [B, T, input_size] (torch tensors or arrays) -> poses [B, T, 26] in [0, 1], a device tensor.  There is no CPU path."""

    def __init__(self, input_size, output_size=26, device="cuda:0"):
        import torch
        if output_size != 26:
            raise ValueError(f"the decoder's poses have 26 values per frame, not {output_size}")
        self.input_size, self.output_size = int(input_size), 26
        self._spec = bilstm_shapes(self.input_size)
        self.device = torch.device(device)
        self._native = None

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics for the keys: with strict=True a missing or unexpected key raises RuntimeError.  Every
        shape is checked."""
        from .native import NativeBiLSTM
        _check_state_dict("PoseDecoderBiLSTM", self._spec, state_dict, strict)
        missing = [k for k in self._spec if k not in state_dict]
        if missing:
            raise RuntimeError(f"PoseDecoderBiLSTM cannot run without {missing}")
        net = NativeBiLSTM(self.device.index or 0)
        for k in self._spec:
            net.set_param(k, _to_numpy(state_dict[k]).astype(np.float32))
        net.finalize()
        if self._native is not None:
            self._native.close()
        self._native = net
        return self

    def eval(self):
        return self

    def close(self):
        if self._native is not None:
            self._native.close()
            self._native = None

    def _net(self):
        if self._native is None:
            raise RuntimeError("PoseDecoderBiLSTM: load_state_dict first")
        return self._native

    def forward(self, features):
        """The reference's forward: poses [B, T, 26]."""
        net = self._net()
        return net.decode(_device_tensor(features, self.input_size, "features", self.device))

    def hidden(self, features, layers=2):
        """Test hook: self.LSTM's output [B, T, 256] cut after `layers` (1 or 2) layers."""
        net = self._net()
        return net.hidden(_device_tensor(features, self.input_size, "features", self.device), layers)

    __call__ = forward


class Generator:
    """Eval-mode M2S-GAN Generator on the MI355X.  mel: fp32 [B, Tm, 128]; noise: fp32 [B, Ln, 8] with (Tm-1)//3+1 = 30 Ln (> 128
    with the TCN decoder); torch tensors or arrays.  Results are device tensors.  `decoder`: "tcn", the reference's PoseDecoderTCN, or
    "bilstm", its commented-out `self.tcn = PoseDecoderBiLSTM(128, 26)` (Generator.py:57-58) - the CNN-LSTM baseline."""

    def __init__(self, device="cuda:0", decoder="tcn"):
        import torch
        if decoder not in ("tcn", "bilstm"):
            raise ValueError(f"decoder must be 'tcn' or 'bilstm', got {decoder!r}")
        self.device = torch.device(device)
        self.decoder = decoder
        self._native = None
        self._lstm = None

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics for the keys: with strict=True a missing or unexpected key raises RuntimeError.  Every
        shape is checked."""
        from .native import NativeM2SGAN
        bilstm = self.decoder == "bilstm"
        spec = m2sgan_bilstm_shapes() if bilstm else m2sgan_shapes()
        _check_state_dict("Generator", spec, state_dict, strict)
        lstm = None
        if bilstm:
            lstm = PoseDecoderBiLSTM(2 * CHANNELS, 26, self.device).load_state_dict(
                {k[4:]: v for k, v in state_dict.items() if k.startswith("tcn.") and k in spec}, strict=False)
        net = NativeM2SGAN(self.device.index or 0, decoder="none" if bilstm else "tcn")
        for k, v in state_dict.items():
            if k in spec and not (bilstm and k.startswith("tcn.")):
                net.set_param(k, _to_numpy(v).astype(np.float32))
        net.finalize()
        if self._native is not None:
            self._native.close()
        if self._lstm is not None:
            self._lstm.close()
        self._native, self._lstm = net, lstm
        return self

    def eval(self):
        return self

    def to(self, device):
        import torch
        if torch.device(device) != self.device and self._native is not None:
            raise RuntimeError("move the model before load_state_dict (its weights live on the device it was loaded on)")
        self.device = torch.device(device)
        return self

    def _net(self):
        if self._native is None:
            raise RuntimeError("Generator: load_state_dict first")
        return self._native

    def _tensor(self, x, last, what):
        return _device_tensor(x, last, what, self.device)

    def _inputs(self, mel, noise):
        mel, noise = self._tensor(mel, 128, "mel"), self._tensor(noise, LATENT_DIM, "noise")
        if noise.shape[0] != mel.shape[0]:
            raise ValueError(f"{mel.shape[0]} mels and {noise.shape[0]} latents")
        return mel, noise

    def features(self, mel, noise):
        """Generator.features: cat(music_encoder(mel), noise branch) [B, T, 128]."""
        net = self._net()
        return net.features(*self._inputs(mel, noise))

    def decode(self, features):
        """self.tcn on features [B, T, 128] the caller holds: poses [B, T, 13, 2]."""
        net = self._net()
        f = self._tensor(features, 2 * CHANNELS, "features")
        y = self._lstm.forward(f) if self._lstm is not None else net.decode(f)
        return y.view(f.shape[0], f.shape[1], 13, 2)

    def debug_blocks(self, features, n_blocks):
        """Test hook: the residual stream [B, T, 64] after the first `n_blocks` temporal blocks (TCN decoder only)."""
        return self._net().decode(self._tensor(features, 2 * CHANNELS, "features"), n_blocks=n_blocks)

    def forward(self, mel, noise):
        """The reference's forward: poses [B, T, 13, 2] in [0, 1]."""
        net = self._net()
        if self._lstm is not None:
            return self.decode(net.features(*self._inputs(mel, noise)))
        y = net.generate(*self._inputs(mel, noise))
        return y.view(y.shape[0], y.shape[1], 13, 2)

    __call__ = forward


class Generator_CVPR_LSTM:
    """Eval-mode Generator_CVPR_LSTM of the reference (Generator.py:89-100): `self.lstm = PoseDecoderBiLSTM(20, 26)` on 20 audio
    features per frame, which the caller supplies (the reference computes them with librosa).  x: fp32 [B, T, 20] -> poses
    [B, T, 13, 2]; `noise` is ignored, as in the reference."""
    INPUT_SIZE = 20

    def __init__(self, device="cuda:0"):
        self.lstm = PoseDecoderBiLSTM(self.INPUT_SIZE, 26, device)
        self.device = self.lstm.device

    def load_state_dict(self, state_dict, strict=True):
        spec = OrderedDict(("lstm." + k, v) for k, v in bilstm_shapes(self.INPUT_SIZE).items())
        _check_state_dict("Generator_CVPR_LSTM", spec, state_dict, strict)
        self.lstm.load_state_dict({k[5:]: v for k, v in state_dict.items() if k in spec}, strict=False)
        return self

    def eval(self):
        return self

    def forward(self, x, noise=None):
        y = self.lstm.forward(x)
        return y.view(y.shape[0], y.shape[1], 13, 2)

    __call__ = forward


def m2sgan_decoder_of(keys):
    """'bilstm' for the keys of a CNN-LSTM baseline's Generator checkpoint (`tcn.LSTM.weight_ih_l0` present), else 'tcn'."""
    return "bilstm" if "tcn.LSTM.weight_ih_l0" in keys else "tcn"


def load_m2sgan_generator(path, device="cuda:0"):
    """A generator checkpoint (the plain state_dict Contrastive_Stage/M2SGAN_eval.py:451 loads; a DataParallel `module.` prefix is
    stripped) -> a loaded Generator, with the decoder its keys name (m2sgan_decoder_of)."""
    import torch
    sd = strip_module_prefix(torch.load(path, map_location="cpu"))
    return Generator(device, decoder=m2sgan_decoder_of(sd)).load_state_dict(sd, strict=True)


def load_cvpr_lstm_generator(path, device="cuda:0"):
    """A Generator_CVPR_LSTM checkpoint (a plain state_dict, keys `lstm.*`; a `module.` prefix is stripped) -> a loaded model."""
    import torch
    sd = strip_module_prefix(torch.load(path, map_location="cpu"))
    return Generator_CVPR_LSTM(device).load_state_dict(sd, strict=True)


class GeneratorBaseline:
    """A Generator in a trainer's shape: `.device` and `generate_music_motion`, what evaluate.evaluate_dataset asks of its model.
    The generator has no sampling loop, so the loop's options are refused instead of ignored."""

    def __init__(self, generator):
        self.generator = generator
        self.device = generator.device

    def generate_music_motion(self, mel, dim_pose=26, noise=None, smooth=None, guidance_scale=None, steps=None, spacing="uniform",
                              solver="ddim", takes=1):
        """mel [B, Tm, 128] -> poses [B, T, 26] on the device.  `noise`: the latent [B, Ln, 8], or the diffusion noise [B, T, 26]
        evaluate_dataset draws per clip (evaluate.clip_noise), of which the latent is noise[:, :T // 30, :8] - standard normal draws
        that belong to the clip, so its motion does not depend on the batch it is generated in; None: fresh draws.
        `smooth` = k: Savitzky-Golay window k, order 5 (tools/visualization.py:126).  The trainer's sampling options raise."""
        import torch
        asked = [k for k, on in (("guidance_scale", guidance_scale is not None), ("steps", steps is not None), ("solver", solver != "ddim"),
                                 ("takes", takes != 1)) if on]
        if asked:
            raise ValueError(f"the M2S-GAN generator is one forward pass, not a sampling loop: {', '.join(asked)} do not apply to it")
        if dim_pose != 26:
            raise ValueError(f"the generator's poses have 26 values per frame, not {dim_pose}")
        mel = mel if torch.is_tensor(mel) else torch.as_tensor(np.asarray(mel))
        B, T = mel.shape[0], (mel.shape[1] - 1) // 3 + 1
        Ln = T // FRAMES_PER_STEP
        if noise is None:
            noise = torch.randn(B, Ln, LATENT_DIM)
        noise = noise if torch.is_tensor(noise) else torch.as_tensor(np.asarray(noise))
        if tuple(noise.shape) == (B, T, dim_pose):
            noise = noise[:, :Ln, :LATENT_DIM]
        elif noise.dim() != 3 or (noise.shape[0], noise.shape[2]) != (B, LATENT_DIM):
            raise ValueError(f"noise must be the latent [B, Ln, 8] or the diffusion noise {(B, T, dim_pose)}, got {tuple(noise.shape)}")
        pred = self.generator.forward(mel, noise).reshape(B, T, dim_pose)
        if smooth:
            from .native import savgol_filter
            pred = savgol_filter(pred.contiguous(), int(smooth), 5)
        return pred
