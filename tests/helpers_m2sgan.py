"""The fp64 oracle of the M2S-GAN Generator (Contrastive_Stage/models/Generator.py:52-86, models/TCN.py) for the tests of
csrc/dc_m2sgan.hip: the repository's fp64 music encoder oracle (oracle/ddim_oracle.py music_encoder with the generator's own
`music_encoder.*` entries) plus a restatement of the decoder - transposed convolutions, reflection-indexed dilated convolutions,
pool, residual, head -, and the fixture's inputs regenerated from their seeds."""
import numpy as np
import torch

from diffusion_conductor_amd.synthetic import _rng, smooth_mel

from oracle import ddim_oracle as O

# (T, Tm): 150 is the shortest length that runs (the reflections of both ends overlap at dilation 32) and the three Tm all give it;
# 150 / 180 / 240 / 480 are no whole 32-frame groups, 960 is
FIXTURE_CASES = ((150, 448), (150, 449), (150, 450), (180, 538), (240, 718), (480, 1438), (960, 2878))
MEL_SEED, LATENT_SEED = 41, 42
# the reference's fp32 features of the cases, in files of their own beside g15_m2sgan.npz (each under the size limit of a committed file)
FEATURE_FILES = {"g15_m2sgan_features_a.npz": FIXTURE_CASES[:4], "g15_m2sgan_features_b.npz": FIXTURE_CASES[4:6],
                 "g15_m2sgan_features_c.npz": FIXTURE_CASES[6:]}
BLOCK = "tcn.TCN.tcn.tcn.network.{}."
NOISE_CONVS = ((1, 1), (5, 3), (3, 1), (2, 2))          # (stride, padding) of the four ConvTranspose1d
BN_EPS = 1e-5


def case_name(T, Tm):
    return f"T{T}_Tm{Tm}"


def feature_file(T, Tm):
    return next(name for name, cases in FEATURE_FILES.items() if (T, Tm) in cases)


def load_fixture(golden):
    """g15_m2sgan.npz and its feature files as one dict (`golden`: helpers.golden)."""
    g = dict(golden("g15_m2sgan.npz"))
    for name in FEATURE_FILES:
        g.update(golden(name))
    return g


def fixture_inputs(T, Tm, B=2):
    """(mel [B, Tm, 128], latent [B, T // 30, 8]) of the fixture case (the clips of one (T, Tm) are its own)."""
    mel = np.stack([smooth_mel(10000 * T + 10 * Tm + b, Tm, seed=MEL_SEED) for b in range(B)])
    z = np.stack([_rng(LATENT_SEED, "m2sgan_latent", 10000 * T + 10 * Tm + b).standard_normal((T // 30, 8), dtype=np.float32) for b in range(B)])
    return mel, z


def _f64(v):
    return (v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(torch.float64)


def _np(v):
    return _f64(v).numpy()


def _bn(sd, p, x):
    """eval-mode BatchNorm1d `p` on x [..., C]."""
    return (x - _np(sd[p + ".running_mean"])) / np.sqrt(_np(sd[p + ".running_var"]) + BN_EPS) * _np(sd[p + ".weight"]) + _np(sd[p + ".bias"])


def fold_conv(g, v, cb, gamma, beta, mean, var):
    """One weight-normed Conv1d + eval-mode BatchNorm as one weight and bias, fp64: W [cout, k * cin] (column tap * cin + ci), b [cout]."""
    g, v, cb, gamma, beta, mean, var = (_np(a) for a in (g, v, cb, gamma, beta, mean, var))
    w = g.reshape(-1, 1, 1) * v / np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))
    s = gamma / np.sqrt(var + BN_EPS)
    return (w * s[:, None, None]).transpose(0, 2, 1).reshape(v.shape[0], -1), (cb - mean) * s + beta


def reflect_index(T, shift):
    """rho(t + shift) for t = 0 .. T - 1: the reflection about the clip's ends."""
    p = np.arange(T) + shift
    p = np.where(p < 0, -p, p)
    return np.where(p >= T, 2 * (T - 1) - p, p)


def dilated_conv(sd, cv, x, d):
    """The weight-normed Conv1d `cv` (kernel 5, dilation d, reflection padding 4 d, Chomp1d(4 d)) on x [B, T, cin] -> [B, T, 64]:
    y[t] = b + sum_j W[:, :, j] x[rho(t + (j - 2) d)]."""
    v = _np(sd[cv + ".weight_v"])
    w = _np(sd[cv + ".weight_g"]).reshape(-1, 1, 1) * v / np.sqrt((v * v).sum(axis=(1, 2), keepdims=True))
    T = x.shape[1]
    y = np.broadcast_to(_np(sd[cv + ".bias"]), x.shape[:2] + (w.shape[0],)).copy()
    for j in range(5):
        y += x[:, reflect_index(T, (j - 2) * d)] @ w[:, :, j].T
    return y


def temporal_block(sd, i, x, pre=None):
    """TemporalBlock i (dilation 2^i) on x [B, T, cin] -> [B, T, 64].  `pre`: a list that receives the two pre-activations."""
    p, d = BLOCK.format(i), 2 ** i
    a1 = _bn(sd, p + "bn1", dilated_conv(sd, p + "conv1", x, d))
    a2 = _bn(sd, p + "bn2", dilated_conv(sd, p + "conv2", np.maximum(a1, 0), d))
    if pre is not None:
        pre += [a1, a2]
    h = np.maximum(a2, 0)
    padded = np.pad(h, ((0, 0), (1, 1), (0, 0)))
    pooled = (padded[:, :-2] + padded[:, 1:-1] + padded[:, 2:]) / 3.0          # AvgPool1d(3, 1, 1), count_include_pad
    res = x
    if p + "downsample.weight" in sd:
        res = x @ _np(sd[p + "downsample.weight"])[:, :, 0].T + _np(sd[p + "downsample.bias"])
    return np.maximum(pooled + res, 0)


def oracle_blocks(sd, feat, n_blocks=6, pre=None):
    """fp64 residual stream [B, T, 64] after the first n_blocks temporal blocks of feat [B, T, 128] (any float dtype)."""
    x = _np(feat)
    for i in range(n_blocks):
        x = temporal_block(sd, i, x, pre)
    return x


def oracle_head(sd, h):
    y = h @ _np(sd["tcn.TCN.tcn.linear.weight"]).T + _np(sd["tcn.TCN.tcn.linear.bias"])
    y = np.maximum(y @ _np(sd["tcn.fc.0.weight"]).T + _np(sd["tcn.fc.0.bias"]), 0)
    y = np.maximum(y @ _np(sd["tcn.fc.2.weight"]).T + _np(sd["tcn.fc.2.bias"]), 0)
    return 1.0 / (1.0 + np.exp(-(y @ _np(sd["tcn.fc.4.weight"]).T + _np(sd["tcn.fc.4.bias"]))))


def oracle_decode(sd, feat, pre=None):
    """fp64 poses [B, T, 26] of features [B, T, 128] (any float dtype; computed in fp64)."""
    return oracle_head(sd, oracle_blocks(sd, feat, 6, pre))


def oracle_noise_branch(sd, z):
    """fp64 noise_BN(noise_convTranspose(z^T))^T: latent [B, Ln, 8] -> [B, 30 Ln, 64]."""
    x = _np(z)
    for i, (stride, pad) in enumerate(NOISE_CONVS):
        w, b = _np(sd[f"noise_convTranspose.{2 * i}.weight"]), _np(sd[f"noise_convTranspose.{2 * i}.bias"])      # [cin, cout, k]
        k, L = w.shape[2], x.shape[1]
        full = np.zeros((x.shape[0], (L - 1) * stride + k, w.shape[1]))
        for tap in range(k):                                # input frame ti lands on output frame ti * stride + tap (before the cut)
            full[:, tap:tap + (L - 1) * stride + 1:stride] += x @ w[:, :, tap]
        x = np.maximum(full[:, pad:full.shape[1] - pad] + b, 0)
    return _bn(sd, "noise_BN", x)


def oracle_features(sd, mel, z):
    """fp64 Generator.features [B, T, 128]."""
    p = {k: _f64(v) for k, v in sd.items() if k.startswith("music_encoder.") and not k.endswith("num_batches_tracked")}
    with torch.no_grad():
        hx = O.music_encoder(p, _f64(mel), prefix="music_encoder").numpy()
    return np.concatenate([hx, oracle_noise_branch(sd, z)], axis=2)


def oracle_generate(sd, mel, z, pre=None):
    """fp64 (features [B, T, 128], poses [B, T, 26]) of Generator.forward."""
    feat = oracle_features(sd, mel, z)
    return feat, oracle_decode(sd, feat, pre)
