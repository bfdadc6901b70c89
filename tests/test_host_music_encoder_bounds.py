"""Host-side checks behind tests/test_gpu_music_encoder_edges.py: the per-frame bound sees every planted defect that the whole-tensor
bound lets through, the oracle's clips are independent of their batch, the weight variants load and keep the frame norms the
per-frame measure divides by, and the footprint of a non-finite mel value in the oracle.  No GPU."""
import numpy as np
import pytest
import torch

import helpers_music_encoder as H
from helpers import batch_mel, state_dict_np

from diffusion_conductor_amd.param_spec import DenoiserConfig, param_shapes
from diffusion_conductor_amd.synthetic import MUSIC_ENCODER_VARIANTS, music_encoder_weight_variant, smooth_mel


@pytest.fixture(scope="module")
def long_clip():
    """White mel of one clip at Tm = 5400: the clean oracle features, every layer's clean input, and the parameters."""
    p = H.oracle_params(state_dict_np())
    mel = batch_mel(1, 5400)
    clean = {}
    ref = H.oracle_features(p, mel, clean=clean)
    return p, mel, ref, clean


def test_layerwise_oracle_is_the_oracle(long_clip):
    p, mel, ref, _ = long_clip
    plain = H.oracle_features(p, mel)
    assert np.array_equal(ref[0], plain[0]) and np.array_equal(ref[1], plain[1])


@pytest.mark.parametrize("defect", H.DEFECTS)
def test_frame_bound_catches_each_planted_defect(long_clip, defect):
    """Every planted defect exceeds FRAME_TOL of BOTH formats at a frame it touches (and, for a time-axis defect, touches no frame
    outside its receptive field), while the quiet ones stay under TOL_ENC_F16 of the whole tensor: today's metric passes them in the
    default format at production length."""
    p, mel, ref, clean = long_clip
    bad = H.oracle_features(p, mel, defect=defect, clean=clean)
    for k in range(2):
        fe = H.frame_errors(bad[k], ref[k])[0]
        whole = float(np.linalg.norm(bad[k] - ref[k]) / np.linalg.norm(ref[k]))
        span = H.defect_frames(defect, 5400)
        touched = np.nonzero(fe > 0)[0]
        print(f"{defect} {('xf_proj', 'xf_out')[k]}: whole {whole:.2e} worst frame {fe.max():.2e} frames touched {len(touched)}")
        assert fe.max() > max(H.FRAME_TOL.values()), (defect, fe.max())
        if span is not None:
            assert len(touched) and touched[0] >= span[0] and touched[-1] < span[1], (defect, touched, span)
        if defect in H.QUIET_DEFECTS:
            assert whole < H.clip_tol("f16"), (defect, whole)
    assert max(H.FRAME_TOL.values()) < 2.9e-3      # the smallest planted defect measured on white mel


def test_clip_independence_of_the_oracle():
    """A clip's oracle features do not depend on its batch (the GPU tests check only the chunk-edge clips of a large batch)."""
    sd = state_dict_np()
    mel = batch_mel(4, 97, first=20)
    whole = H.oracle_features(sd, mel)
    for idx in ([2], [3, 0]):
        part = H.oracle_features(sd, mel[idx])
        for k in range(2):
            d = np.abs(part[k] - whole[k][idx]).max()
            assert d <= 1e-12 * np.abs(whole[k]).max(), (idx, d)     # (fp64 GEMM blocking may change with the batch: last bits only)


@pytest.mark.parametrize("kind", MUSIC_ENCODER_VARIANTS)
def test_weight_variants_load_and_keep_frame_norms(kind):
    """Each variant has exactly the denoiser's keys and shapes (what MotionTransformer.load_state_dict(strict=True) asks for), replaces
    only `music_encoder.*`, differs from the seeded checkpoint there, and keeps every oracle frame norm above 1."""
    from diffusion_conductor_amd import MotionTransformer
    sd = music_encoder_weight_variant(kind, seed=1)
    base = state_dict_np()
    spec = param_shapes(DenoiserConfig())
    assert list(sd) == list(spec) and all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    m = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device="cpu", no_clip=True)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    changed = [k for k in sd if not np.array_equal(sd[k], base[k])]
    assert changed and all(k.startswith("music_encoder.") for k in changed)
    for B, Tm in H.WEIGHT_SHAPES:
        xp, xo = H.oracle_features(sd, batch_mel(B, Tm, first=80 + Tm))
        assert np.isfinite(xo).all() and min(np.linalg.norm(xo, axis=2).min(), np.linalg.norm(xp, axis=2).min()) > 1.0, (kind, B, Tm)
    with pytest.raises(ValueError):
        music_encoder_weight_variant("no such kind")


def test_dead_channels_tie_in_every_pool_window():
    """The dead channels are exactly 0 at every pool's input, so every window of theirs is a tie."""
    p = H.oracle_params(music_encoder_weight_variant("dead_channels", seed=1))
    clean = {}
    with torch.no_grad():
        H.music_encoder_layers(p, torch.from_numpy(batch_mel(1, 25)).double(), clean=clean)
    for pool in ("pool1", "pool2", "pool3"):
        x = clean[pool]
        dead = np.arange(x.shape[1]) % 4 == 1
        assert float(x[:, dead].abs().max()) == 0.0 and float(x[:, ~dead].abs().max()) > 0.0, pool


def test_special_inputs_keep_frame_norms():
    """The constant, ramp, impulse and smooth mels of the GPU tests: finite oracle features with frame norms above 1 (errors() asserts
    it), and exactly the same frame everywhere for a constant mel."""
    sd = state_dict_np()
    for value in (0.0, 0.37):
        xp, xo = H.oracle_features(sd, np.full((1, 49, 128), value, np.float32))
        H.errors(xo, xo), H.errors(xp, xp)
        assert np.abs(xo - xo[:, :1]).max() <= 1e-13 * np.abs(xo).max(), value
    mel, cases = H.impulse_mels(25)
    assert len(cases) == 48 and mel.sum() == 48.0
    for mel in (H.ramp_mels(49), mel, np.stack([smooth_mel(b, 271) for b in range(2)])):
        for r in H.oracle_features(sd, mel):
            H.errors(r, r)


@pytest.mark.parametrize("value", (np.nan, np.inf, -np.inf))
def test_nonfinite_footprint_of_the_oracle(value):
    """One non-finite value at mel[0, t, 64], Tm = 97: the oracle's non-finite frames are one contiguous run with all 64 channels -
    the receptive field of the frames, clipped (and reflected) at the clip's ends; NaN, +inf and -inf give the same runs."""
    sd = state_dict_np()
    want = {0: (0, 7), 7: (0, 9), 8: (0, 9), 48: (10, 23), 96: (26, 33)}
    assert tuple(want) == H.NAN_TS
    for t, run in want.items():
        mel = batch_mel(1, 97, first=91)
        mel[0, t, 64] = value
        xp, xo = H.oracle_features(sd, mel)
        assert H.nonfinite_run(xo[0]) == run and H.nonfinite_run(xp[0]) == run, (t, H.nonfinite_run(xo[0]))


def test_shape_lists_follow_the_kernel_constants():
    """The shape lists hold both sides of every tile edge they claim, and the second-round batch is 19 clips at 256 CUs (513 conv3 tiles)."""
    tms, T = set(H.TILE_TMS), H.frames
    for edge in (H.STEM_ROWS, 2 * H.STEM_ROWS, H.POOL_NY, 2 * H.POOL_NY, 3 * H.POOL_NY):
        assert {edge, edge + 1} <= tms and ({edge - 1} <= tms or {edge - 2} <= tms), edge
    for edge in (H.CONV3_ROWS, H.POOL_NY, H.HEAD_WAVE, H.HEAD_WG):
        ts = {T(tm) for tm in tms}
        assert {edge, edge + 1} <= ts, edge
    assert {tm % 3 for tm in tms} == {0, 1, 2} and min(tms) == H.MIN_TM
    assert H.loop_batch(256) == 19 and 19 * 27 == 513
    assert min(H.errors(np.ones((1, 2, 64)), np.full((1, 2, 64), 2.0))) == 0.5
    with pytest.raises(AssertionError):
        H.errors(np.zeros((1, 2, 64)), np.full((1, 2, 64), 0.1))
