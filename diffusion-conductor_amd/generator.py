"""The M2S-GAN generator, the baseline the diffusion denoiser is compared against, as a second model of the evaluation.

``Generator`` is a drop-in for the reference's class of the same name (Contrastive_Stage/models/Generator.py:52-86) in eval mode:
``forward(mel, noise)`` maps a mel [B, Tm, 128] and a latent [B, Ln, 8] to poses [B, T, 13, 2], T = (Tm-1)//3+1 = 30 Ln.  Its
MusicEncoder runs on the kernels of csrc/dc_music.hip with this checkpoint's own ``music_encoder.*`` weights, the noise branch,
the six dilated temporal blocks (models/TCN.py) and the head on csrc/dc_m2sgan.hip (dc_m2sgan_* in include/dc_ddim.h).
``GeneratorBaseline`` gives it a trainer's shape, so ``evaluate.evaluate_dataset`` scores it like the denoiser
(Contrastive_Stage/M2SGAN_eval.py scores it with the same latent metrics and the same M2SNet).  There is no CPU path.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from .m2snet import strip_module_prefix
from .motion_encoder import _to_numpy

N_BLOCKS, CHANNELS, KERNEL, LATENT_DIM, FRAMES_PER_STEP = 6, 64, 5, 8, 30
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


class Generator:
    """Eval-mode M2S-GAN Generator on the MI355X.  mel: fp32 [B, Tm, 128]; noise: fp32 [B, Ln, 8] with (Tm-1)//3+1 = 30 Ln > 128;
    torch tensors or arrays.  Results are device tensors."""

    def __init__(self, device="cuda:0"):
        import torch
        self.device = torch.device(device)
        self._native = None

    def load_state_dict(self, state_dict, strict=True):
        """nn.Module.load_state_dict semantics for the keys: with strict=True a missing or unexpected key raises RuntimeError.  Every
        shape is checked."""
        from .native import NativeM2SGAN
        spec = m2sgan_shapes()
        missing = [k for k in spec if k not in state_dict]
        unexpected = [k for k in state_dict if k not in spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for Generator: missing keys {missing}, unexpected keys {unexpected}")
        for k, v in state_dict.items():
            if k in spec and tuple(np.shape(_to_numpy(v))) != spec[k]:
                raise RuntimeError(f"size mismatch for {k}: got {tuple(np.shape(_to_numpy(v)))}, expected {spec[k]}")
        net = NativeM2SGAN(self.device.index or 0)
        for k, v in state_dict.items():
            if k in spec:
                net.set_param(k, _to_numpy(v).astype(np.float32))
        net.finalize()
        if self._native is not None:
            self._native.close()
        self._native = net
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
        import torch
        t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
        if t.dim() != 3 or t.shape[2] != last:
            raise ValueError(f"{what} must be [B, *, {last}], got {tuple(t.shape)}")
        return t.to(self.device, torch.float32).contiguous()

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
        return net.decode(f).view(f.shape[0], f.shape[1], 13, 2)

    def debug_blocks(self, features, n_blocks):
        """Test hook: the residual stream [B, T, 64] after the first `n_blocks` temporal blocks."""
        return self._net().decode(self._tensor(features, 2 * CHANNELS, "features"), n_blocks=n_blocks)

    def forward(self, mel, noise):
        """The reference's forward: poses [B, T, 13, 2] in [0, 1]."""
        net = self._net()
        y = net.generate(*self._inputs(mel, noise))
        return y.view(y.shape[0], y.shape[1], 13, 2)

    __call__ = forward


def load_m2sgan_generator(path, device="cuda:0"):
    """A generator checkpoint (the plain state_dict Contrastive_Stage/M2SGAN_eval.py:451 loads; a DataParallel `module.` prefix is
    stripped) -> a loaded Generator."""
    import torch
    sd = torch.load(path, map_location="cpu")
    return Generator(device).load_state_dict(strip_module_prefix(sd), strict=True)


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
