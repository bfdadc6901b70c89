"""The fp64 oracle of M2SNet (Contrastive_Stage/models/M2SNet.py:31-36) for the tests of csrc/dc_m2snet.hip: the repository's two
fp64 encoder oracles (oracle/ddim_oracle.py music_encoder with M2SNet's own `music_encoder.*` entries, oracle/stgcn_oracle.py)
plus the fuse head, and the fixture's inputs regenerated from their seeds."""
import numpy as np
import torch

from diffusion_conductor_amd.synthetic import smooth_mel, synthetic_motion

from oracle import ddim_oracle as O
from oracle.stgcn_oracle import motion_encoder_latent

FIXTURE_TS = (2, 3, 17, 31, 32, 33, 64, 65, 90)
MEL_SEED, MOTION_SEED = 31, 32


def fixture_inputs(T, Tm=None, B=2):
    """(mel [B, Tm, 128], motion [B, T, 13, 2]) of the fixture at T frames (Tm = 3 T - 2 unless given; the clips of one T are its own)."""
    Tm = 3 * T - 2 if Tm is None else Tm
    mel = np.stack([smooth_mel(1000 * T + b, Tm, seed=MEL_SEED) for b in range(B)])
    return mel, synthetic_motion(B, T, seed=MOTION_SEED, first=1000 * T)


def _f64(v):
    return (v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(torch.float64)


def oracle_latents(sd, mel, motion):
    """fp64 (music latent [B, T, 64], motion latent [B, 64, T]) of the state_dict `sd` (M2SNet's keys, no `module.` prefix)."""
    p = {k: _f64(v) for k, v in sd.items() if k.startswith("music_encoder.") and not k.endswith("num_batches_tracked")}
    msd = {k[len("motion_encoder."):]: v for k, v in sd.items() if k.startswith("motion_encoder.")}
    with torch.no_grad():
        return O.music_encoder(p, _f64(mel), prefix="music_encoder"), motion_encoder_latent(msd, motion, torch.float64)


def oracle_head(sd, music_latent, motion_latent, hidden=False):
    """fp64 (logit [B, T], probability [B, T]) of the fuse head on latents [B, T, 64] and [B, 64, T] (any float dtype; computed in
    fp64).  hidden=True: the two pre-activations [B, T, 64] as well."""
    z = torch.cat([_f64(music_latent), _f64(motion_latent).transpose(1, 2)], dim=2)
    a1 = z @ _f64(sd["fuse_layer.0.weight"])[:, :, 0].T + _f64(sd["fuse_layer.0.bias"])
    a2 = torch.relu(a1) @ _f64(sd["fuse_layer.2.weight"])[:, :, 0].T + _f64(sd["fuse_layer.2.bias"])
    logit = (torch.relu(a2) @ _f64(sd["fuse_layer.4.weight"])[:, :, 0].T + _f64(sd["fuse_layer.4.bias"]))[..., 0]
    out = (logit.numpy(), torch.sigmoid(logit).numpy())
    return out + (a1.numpy(), a2.numpy()) if hidden else out


def oracle_score(sd, mel, motion):
    """fp64 (logit, probability), each [B, T], of M2SNet.forward."""
    return oracle_head(sd, *oracle_latents(sd, mel, motion))
