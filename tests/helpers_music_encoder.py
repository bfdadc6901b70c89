"""The fp64 oracle of the MusicEncoder + proj (oracle/ddim_oracle.py music_encoder, transformer.py:313-340, 447-459) for the tests of
csrc/dc_music.hip, its two error measures, the shape lists the kernels' constants ask for, and the oracle restated layer by layer with
planted defects: what one wrong row of one layer does to the features, so that the bounds can be shown to see it (host only)."""
import numpy as np
import torch

from oracle import ddim_oracle as O

F = torch.nn.functional

# ---- bounds -----------------------------------------------------------------------------------------------------------------------
# Per clip (rel-L2 over a clip's [T, 64]): the project's measured bounds of the two activation formats, defined once in
# test_gpu_parity.py (importing that module needs no GPU).
# Per frame (rel-L2 over the 64 channels of one frame, so one wrong frame cannot hide in a long clip) and for k_me_proj alone: three
# times the worst case measured on an MI355X against the fp64 oracle over all cases of test_gpu_music_encoder_edges.py, rounded up to
# one digit (profiles/music_encoder_edges_gpu_tests.txt has the figures per group).
FORMATS = ("split", "f16")
FRAME_TOL = {"split": 4e-5, "f16": 2e-3}       # measured worst 1.24e-5 (unit impulses) and 6.23e-4 (20 x 648)
PROJ_TOL = 3e-5                                  # measured worst 6.7e-6 (unit impulses): bf16 hi/lo operands without the lo x lo product
LONG_CLIP_FRAME_GATE = FORMATS      # the formats whose per-frame bound gates the 30-s and 60-s clips


def clip_tol(fmt):
    from test_gpu_parity import TOL_ENC_F16, TOL_ENC_SPLIT
    return {"split": TOL_ENC_SPLIT, "f16": TOL_ENC_F16}[fmt]


# ---- shapes, from the kernels' constants ----------------------------------------------------------------------------------------
STEM_ROWS = 8           # launch_stem ROWS (k_me_stem: 8 x 64-pixel tiles over Tm x 128)
MID_ROWS = 8            # launch_mid ROWS (k_me_mid: 8 x 32 over Tm x 64)
CONV3_ROWS = 8          # launch_conv_t<32, 32, 1, 8, 1, SP> ROWS (conv3.0, conv3.1: 8 x 32 over T x 32)
POOL_NY = 24            # kPoolNY: output rows a pool thread walks (pool1 on Tm, pool2 and pool3 on T)
HEAD_WAVE = 32          # k_me_head / k_me_proj: frames per wave ...
HEAD_WG = 128           # ... and per workgroup, over B * T
CHUNK_FRAMES = 32 * 5400    # dc_music_encode: clips per pass = CHUNK_FRAMES / Tm (DC_ME_CHUNK overrides it)
MIN_TM = 4              # below it the reference's reflection padding raises, and so does the library


def frames(Tm):
    """dc_music_frames: the stride-3 pool's output rows."""
    return (Tm - 1) // 3 + 1


# Tm around STEM_ROWS / MID_ROWS (7 8 9, 15 16 17, 23 24 25, 47 48 49), CONV3_ROWS on T (T = 8 | 9 at Tm = 22 - 24 | 25 - 27; 16 | 17 at
# 47 - 48 | 49), POOL_NY on Tm (23 24 25, 47 48 49, 71 72 73) and on T (T = 24 | 25 at Tm = 70 - 72 | 73), HEAD_WAVE on B * T with B = 3
# (T = 32 | 33 at Tm = 94 - 96 | 97), HEAD_WG (T = 128 | 129 at Tm = 382 - 384 | 385), all three phases of the stride-3 pool, and the
# shortest mels (MIN_TM; 6 = two conv3 rows, the fewest reflection padding can take beside 4's)
TILE_TMS = (4, 6, 7, 8, 9, 11, 15, 16, 17, 22, 23, 24, 25, 26, 27, 47, 48, 49, 70, 71, 72, 73, 94, 96, 97, 382, 384, 385)
WEIGHT_SHAPES = ((3, 97), (2, 25), (1, 4))
NAN_TS = (0, 7, 8, 48, 96)              # at Tm = 97: the first tile's rows, its seam, the middle and the last row
IMPULSE_BINS = (0, 1, 31, 32, 63, 64, 126, 127)     # the stem's 64-bin and the mid's 32-column tile seams, and the image's edges


def impulse_ts(Tm):
    return (0, 1, STEM_ROWS - 1, STEM_ROWS, Tm - 2, Tm - 1)


def loop_batch(ncu, T=216):
    """The smallest B whose conv3 tiles, B ceil(T / CONV3_ROWS), exceed the largest persistent grid of the encoder, 2 CUs."""
    per = -(-T // CONV3_ROWS)
    return (2 * ncu) // per + 1


# ---- oracle ---------------------------------------------------------------------------------------------------------------------
def _f64(v):
    return (v.detach().cpu() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(torch.float64)


def oracle_params(sd):
    """The `music_encoder.*` and `proj.*` entries of a state_dict in fp64."""
    return {k: _f64(v) for k, v in sd.items()
            if (k.startswith("music_encoder.") or k.startswith("proj.")) and not k.endswith("num_batches_tracked")}


def oracle_features(sd, mel, defect=None, clean=None):
    """fp64 (xf_proj, xf_out), each [B, T, 64] numpy, of the state_dict `sd` (or oracle_params(sd)) on mel [B, Tm, 128]: O.music_encoder
    and the reference's `proj` on top of it.  `defect`: one of DEFECTS, planted into the layer-by-layer restatement instead (`clean`: see
    music_encoder_layers)."""
    p = sd if all(torch.is_tensor(v) and v.dtype == torch.float64 for v in sd.values()) else oracle_params(sd)
    with torch.no_grad():
        x = O.music_encoder(p, _f64(mel)) if defect is None and clean is None else music_encoder_layers(p, _f64(mel), defect, clean)
        xp = F.linear(x, p["proj.weight"], p["proj.bias"])
    return xp.numpy(), x.numpy()


def oracle_proj(sd, xf_out):
    """fp64 proj of given features (any float dtype) -> numpy [B, T, 64]."""
    with torch.no_grad():
        return F.linear(_f64(xf_out), _f64(sd["proj.weight"]), _f64(sd["proj.bias"])).numpy()


def errors(hip, ref):
    """(max per-clip rel-L2, max per-frame rel-L2 over a frame's 64 channels) of hip [B, T, 64] against ref [B, T, 64].  Plain frame
    norms: the oracle's frames are nowhere small (3.7 at least on smooth mel, 5.1 on white mel), which is asserted."""
    h = np.asarray(hip.detach().cpu() if torch.is_tensor(hip) else hip, np.float64)
    r = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, np.float64)
    assert h.shape == r.shape and r.ndim == 3 and r.shape[2] == 64, (h.shape, r.shape)
    fn = np.linalg.norm(r, axis=2)
    assert fn.min() > 1.0, f"an oracle frame of norm {fn.min():.3g}: the per-frame measure needs a floor here"
    d = h - r
    clip = np.linalg.norm(d.reshape(len(r), -1), axis=1) / np.linalg.norm(r.reshape(len(r), -1), axis=1)
    frame = np.linalg.norm(d, axis=2) / fn
    return float(clip.max()), float(frame.max())


def frame_errors(hip, ref):
    """[B, T] per-frame rel-L2."""
    h, r = np.asarray(hip, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(h - r, axis=2) / np.linalg.norm(r, axis=2)


# ---- the oracle layer by layer, with planted defects ----------------------------------------------------------------------------
HALO_ROW0 = 1024                       # the tile of the `halo` defects: rows 1024 - 1031 of the layer's image
DEFECT_LAYERS = ("conv1.0", "conv1.2", "conv2.1", "conv3.1")
DEFECTS = tuple(f"{l}:{k}" for k in ("bottom", "halo") for l in DEFECT_LAYERS) + ("pool2:zero_pad", "pool2:phase", "conv4:order")
# the one-row defects that leave <= 3.4e-4 of the whole tensor on white mel at Tm = 5400: under TOL_ENC_F16, the per-frame measure's reason
QUIET_DEFECTS = ("conv1.2:bottom", "conv2.1:bottom", "conv3.1:bottom", "conv1.2:halo", "conv2.1:halo", "conv3.1:halo")


def _layer(p, name, x, residual, defect=None):
    """ddim_oracle._conv_res_layer; `defect` ("bottom" | "halo") recomputes the one output row whose taps the defect changes:
    bottom  the reflected padding row below the image (row H - 2 again) is the replicated row H - 1: output row H - 1;
    halo    the tile of rows HALO_ROW0 .. + 7 reads the halo row below it one row too far (H0 + 9 for H0 + 8): output row H0 + 7."""
    pre = "music_encoder." + name
    y = O._conv_res_layer(p, pre, x, residual)
    if defect is None:
        return y
    H = x.shape[2]
    if defect == "bottom":
        r, rows = H - 1, [H - 2, H - 1, H - 1]
    else:
        r = HALO_ROW0 + 7
        assert r + 2 < H, "the halo defect needs an image past its tile"
        rows = [r - 1, r, r + 2]
    slab = F.pad(x[:, :, rows], (1, 1, 0, 0), mode="reflect")
    z = F.conv2d(slab, p[pre + ".conv2d_layer.0.weight"], p[pre + ".conv2d_layer.0.bias"])
    z = F.relu(O._bn(z, p, pre + ".conv2d_layer.1"))
    if residual == "identity":
        z = z + x[:, :, r:r + 1]
    elif residual == "conv":
        rr = F.conv2d(x[:, :, r:r + 1], p[pre + ".residual.0.weight"], p[pre + ".residual.0.bias"])
        z = z + O._bn(rr, p, pre + ".residual.1")
    y = y.clone()
    y[:, :, r:r + 1] = z
    return y


def _pool2(x, kind):
    if kind == "zero_pad":                      # padding that can win
        return F.max_pool2d(F.pad(x, (2, 2, 2, 2), value=0.0), (5, 5), (3, 2), 0)
    if kind == "phase":                         # windows one row late: rows 3 i - 1 .. 3 i + 3
        return F.max_pool2d(F.pad(x[:, :, 1:], (0, 0, 0, 1), value=-float("inf")), (5, 5), (3, 2), (2, 2))
    return F.max_pool2d(x, (5, 5), (3, 2), (2, 2))


def _conv4(p, x, kind):
    if kind == "order":                         # a frame's 512 features in (bin, channel) order against (channel, bin) columns
        x = x.permute(0, 2, 3, 1).flatten(start_dim=2).transpose(1, 2)
    else:
        x = x.transpose(1, 2).flatten(start_dim=2).transpose(1, 2)
    x = F.conv1d(x, p["music_encoder.conv4.0.weight"], p["music_encoder.conv4.0.bias"])
    return O._bn(x, p, "music_encoder.conv4.1").transpose(1, 2)


_STEPS = (("conv1.0", lambda p, x, k: _layer(p, "conv1.0", x, "none", k)),
          ("conv1.1", lambda p, x, k: _layer(p, "conv1.1", x, "identity", k)),
          ("conv1.2", lambda p, x, k: _layer(p, "conv1.2", x, "identity", k)),
          ("pool1", lambda p, x, k: F.max_pool2d(x, (5, 5), (1, 2), (2, 2))),
          ("conv2.0", lambda p, x, k: _layer(p, "conv2.0", x, "conv", k)),
          ("conv2.1", lambda p, x, k: _layer(p, "conv2.1", x, "identity", k)),
          ("pool2", lambda p, x, k: _pool2(x, k)),
          ("conv3.0", lambda p, x, k: _layer(p, "conv3.0", x, "identity", k)),
          ("conv3.1", lambda p, x, k: _layer(p, "conv3.1", x, "identity", k)),
          ("pool3", lambda p, x, k: F.max_pool2d(x, (3, 3), (1, 2), (1, 1))),
          ("conv4", lambda p, x, k: _conv4(p, x, k)))


def music_encoder_layers(p, mel, defect=None, clean=None):
    """O.music_encoder restated layer by layer (the same calls in the same order: identical results without a defect).  `clean`, a
    dict: without a defect it receives every layer's input, with one the layers before the defect are taken from it."""
    assert defect is None or defect in DEFECTS, defect
    where, kind = defect.split(":") if defect else (None, None)
    x = mel.unsqueeze(1)
    started = clean is None or defect is None
    for name, fn in _STEPS:
        if not started and name == where:
            x, started = clean[name], True
        if not started:
            continue
        if defect is None and clean is not None:
            clean[name] = x
        x = fn(p, x, kind if name == where else None)
    return x


def defect_frames(defect, Tm):
    """Output frames [lo, hi) that can differ under a time-axis defect (None: all).  The changed row of the layer, widened by the 3x3
    convolutions (+-1 row each) and 5-row / 3-row pools (+-2 / +-1) behind it, through the stride-3 pool."""
    where, kind = defect.split(":")
    if kind not in ("bottom", "halo"):
        return None
    T = frames(Tm)
    # rows of growth behind the layer, at mel resolution and at frame resolution
    mel_grow = {"conv1.0": 1 + 1 + 2 + 1 + 1, "conv1.2": 2 + 1 + 1, "conv2.1": 0}
    frm_grow = 1 + 1 + 1            # conv3.0, conv3.1, pool3
    if where == "conv3.1":
        r = T - 1 if kind == "bottom" else HALO_ROW0 + 7
        lo, hi = r - 1, r + 1       # pool3 only
    else:
        r = Tm - 1 if kind == "bottom" else HALO_ROW0 + 7
        a, b = r - mel_grow[where], r + mel_grow[where]
        # frame i pools mel rows 3 i - 2 .. 3 i + 2
        lo, hi = -(-(a - 2) // 3) - frm_grow, (b + 2) // 3 + frm_grow
    return max(lo, 0), min(hi + 1, T)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def ramp_mels(Tm):
    """[2, Tm, 128]: a ramp along time and a ramp along bins, both in [0, 1] (reflect and replicate padding differ on a ramp)."""
    t = np.linspace(0.0, 1.0, Tm, dtype=np.float32)[:, None] * np.ones((1, 128), np.float32)
    f = np.ones((Tm, 1), np.float32) * np.linspace(0.0, 1.0, 128, dtype=np.float32)[None, :]
    return np.stack([t, f])


def impulse_mels(Tm):
    """[len(impulse_ts) * len(IMPULSE_BINS), Tm, 128]: one unit impulse per clip, zero mel elsewhere."""
    cases = [(t, f) for t in impulse_ts(Tm) for f in IMPULSE_BINS]
    mel = np.zeros((len(cases), Tm, 128), np.float32)
    for i, (t, f) in enumerate(cases):
        mel[i, t, f] = 1.0
    return mel, cases


def nonfinite_run(xf):
    """(lo, hi): the frames [lo, hi) of one clip's features [T, 64] that are not finite - asserted to be one contiguous run with all 64
    channels of every frame in it."""
    bad = ~np.isfinite(np.asarray(xf, np.float64))
    rows = bad.any(axis=1)
    assert np.array_equal(bad, np.repeat(rows[:, None], bad.shape[1], axis=1)), "a frame with finite and non-finite channels"
    idx = np.nonzero(rows)[0]
    if not len(idx):
        return 0, 0
    assert len(idx) == idx[-1] - idx[0] + 1, f"non-finite frames {idx.tolist()} are not one run"
    return int(idx[0]), int(idx[-1]) + 1


def with_env(env, fn):
    """fn() with os.environ updated by `env` (the library reads DC_ME_PREC and DC_ME_CHUNK per call), restored afterwards."""
    import os
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
