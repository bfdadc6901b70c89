"""The ST-GCN motion encoder's HIP kernels (csrc/dc_stgcn.hip) against the fp64 oracle (oracle/stgcn_oracle.py) at the shapes, weights
and inputs where they can go wrong: lengths around every 30-frame tile edge of k_stgcn_block and every 32-frame wave of k_stgcn_fc,
batches around the 64-clip chunks of dc_motion_encoder_encode, weights away from the one seed of the fixture, a reused workspace,
`out=` slices, other streams, input forms and NaN frames.

Bounds.  Every latent is compared per clip (rel-L2 over [64, T]) and per frame (rel-L2 over the 64 channels of that frame, so one
wrong frame cannot hide in a long clip).  The fp32 kernel against fp64 measured at most 4.5e-7 per clip (motion x 1e3) and 6.3e-7
per frame (identity weights) over all cases here on an MI355X; the bounds are CLIP_TOL = 2e-6 and FRAME_TOL = 5e-6."""
import numpy as np
import pytest
import torch

from oracle.stgcn_oracle import motion_encoder_latent

from diffusion_conductor_amd.motion_encoder import MotionEncoder_STGCN
from diffusion_conductor_amd.native import NativeMotionEncoder
from diffusion_conductor_amd.synthetic import (MOTION_ENCODER_VARIANTS, motion_encoder_weight_variant, synthetic_motion,
                                               synthetic_motion_encoder_state_dict)

pytestmark = pytest.mark.gpu
CLIP_TOL, FRAME_TOL = 2e-6, 5e-6
CHUNK = 64            # SG_CHUNK of dc_stgcn.hip: clips per pass
RADIUS = 10           # 10 blocks, each a temporal conv of radius 1


@pytest.fixture(scope="module")
def weights():
    return synthetic_motion_encoder_state_dict()


@pytest.fixture(scope="module")
def enc(weights):
    return MotionEncoder_STGCN("cuda:0").load_state_dict(weights, strict=True)


def _encode(enc, m, **kw):
    out = enc.latent(torch.from_numpy(m) if isinstance(m, np.ndarray) else m, **kw)
    torch.cuda.synchronize()
    return out.cpu()


def _errors(hip, ref):
    """(max per-clip rel-L2, max per-frame rel-L2) of hip [B, 64, T] against ref [B, 64, T]."""
    h, r = np.asarray(hip, np.float64), np.asarray(ref, np.float64)
    clip = np.linalg.norm((h - r).reshape(len(r), -1), axis=1) / np.maximum(np.linalg.norm(r.reshape(len(r), -1), axis=1), 1e-30)
    frame = np.linalg.norm(h - r, axis=1) / np.maximum(np.linalg.norm(r, axis=1), 1e-30)
    return float(clip.max()), float(frame.max())


def _check(hip, ref, what):
    assert tuple(hip.shape) == tuple(ref.shape), (what, tuple(hip.shape), tuple(ref.shape))
    assert bool(torch.isfinite(hip).all()), what
    ec, ef = _errors(hip, ref)
    print(f"{what}: clip {ec:.2e} frame {ef:.2e}")
    assert ec <= CLIP_TOL and ef <= FRAME_TOL, (what, ec, ef)
    return ec, ef


def _worst(group, errs):
    print(f"== {group}: worst clip {max(e[0] for e in errs):.2e}, worst frame {max(e[1] for e in errs):.2e}")


TILE_TS = (29, 30, 31, 32, 33, 59, 60, 61, 62, 64, 65, 89, 91, 127, 128, 129, 1799, 1800, 1801)


def test_lengths_around_every_tile_edge(enc, weights):
    """B = 3 whole clips (the middle one at a non-zero offset): a partial last tile after full tiles, its halo, zero padding and
    residual; the fc's 32-frame waves and 128-frame workgroups.  T = 1800 whole, no windows."""
    errs = []
    for T in TILE_TS:
        m = synthetic_motion(3, T, seed=31, first=T)
        errs.append(_check(_encode(enc, m), motion_encoder_latent(weights, m), f"T={T}"))
    _worst("tile edges", errs)


@pytest.fixture(scope="module")
def chunk_case(enc, weights):
    """130 clips at two ragged lengths, their oracle latents and the HIP latents of each clip encoded alone."""
    out = {}
    for T in (31, 61):
        m = synthetic_motion(130, T, seed=41, first=T)
        alone = {i: _encode(enc, m[i:i + 1])[0] for i in (0, 62, 63, 64, 65, 127, 128, 129)}
        out[T] = (m, motion_encoder_latent(weights, m), alone)
    return out


@pytest.mark.parametrize("B", (63, 64, 65, 128, 129, 130))
def test_batches_around_the_clip_chunks(enc, chunk_case, B):
    """The second chunk and a ragged last chunk: whole batches against the oracle, and the first clip of the second chunk and the
    last clip bit-identical to the same clips encoded alone."""
    errs = []
    for T, (m, ref, alone) in chunk_case.items():
        hip = _encode(enc, m[:B])
        errs.append(_check(hip, ref[:B], f"B={B} T={T}"))
        for i in {0, min(CHUNK - 1, B - 1), min(CHUNK, B - 1), B - 1}:
            assert torch.equal(hip[i], alone[i]), (B, T, i)
    _worst(f"chunks B={B}", errs)


def test_second_chunk_at_full_length(enc, weights):
    """B = 65 at T = 1800: the second chunk (one clip) of long clips.  The oracle is checked on the chunk edges (a clip's oracle
    latent does not depend on its batch: test_motion_metrics_host.py)."""
    m = synthetic_motion(65, 1800, seed=43)
    hip = _encode(enc, m)
    idx = [0, 1, 62, 63, 64]
    e = _check(hip[idx], motion_encoder_latent(weights, m[idx]), "B=65 T=1800")
    assert torch.equal(hip[64], _encode(enc, m[64:65])[0])
    _worst("chunks B=65 T=1800", [e])


@pytest.mark.parametrize("kind", MOTION_ENCODER_VARIANTS)
def test_weight_variants(kind):
    """Weights loaded through load_state_dict with zeroed, negative and whole-column-zero importances, a dense non-symmetric A,
    BatchNorms with negative gains / running_var down to 1e-4 / large running_mean, a second seed and the identity control."""
    sd = motion_encoder_weight_variant(kind, seed=1)
    e = MotionEncoder_STGCN("cuda:0").load_state_dict(sd, strict=True)
    errs = []
    for B, T in ((3, 61), (2, 127), (1, 1)):
        m = synthetic_motion(B, T, seed=47, first=T)
        errs.append(_check(_encode(e, m), motion_encoder_latent(sd, m), f"{kind} B={B} T={T}"))
    _worst(f"weights {kind}", errs)


def test_constant_motion_shows_the_zero_padding(enc, weights):
    """All-zero and constant motions: interior frames (at least RADIUS from either end) see the same inputs and run the same
    arithmetic, so they are bit-identical; each of the first and last RADIUS frames sees zero padding and differs from them."""
    T = 91
    m = np.zeros((2, T, 13, 2), np.float32)
    m[1] = np.float32(0.37)
    hip = _encode(enc, m)
    e = _check(hip, motion_encoder_latent(weights, m), "constant")
    for i in range(2):
        inner = hip[i, :, RADIUS:T - RADIUS]
        assert torch.equal(inner, inner[:, :1].expand_as(inner)), (i, float((inner - inner[:, :1]).abs().max()))
        for f in list(range(RADIUS)) + list(range(T - RADIUS, T)):
            assert not torch.equal(hip[i, :, f], inner[:, 0]), (i, f)
    _worst("constant motion", [e])


def test_large_motion(enc, weights):
    m = synthetic_motion(3, 65, seed=53) * np.float32(1e3)
    _worst("motion x 1e3", [_check(_encode(enc, m), motion_encoder_latent(weights, m), "x1e3")])


def test_workspace_grows_and_shrinks(weights):
    """One encoder through growing and shrinking (B, T) (the workspace is only reallocated when it grows): each result equals a
    fresh encoder's bit for bit and the oracle within the bounds."""
    e = MotionEncoder_STGCN("cuda:0").load_state_dict(weights, strict=True)
    errs = []
    for B, T in ((2, 1800), (65, 31), (3, 61), (130, 29), (1, 1)):
        m = synthetic_motion(B, T, seed=59, first=B)
        hip = _encode(e, m)
        fresh = MotionEncoder_STGCN("cuda:0").load_state_dict(weights, strict=True)
        assert torch.equal(hip, _encode(fresh, m)), (B, T)
        errs.append(_check(hip, motion_encoder_latent(weights, m), f"workspace B={B} T={T}"))
    _worst("workspace sequence", errs)


@pytest.mark.parametrize("T", (1, 31, 33, 61))
def test_out_slice_keeps_its_neighbours(enc, T):
    """latent(out=big[1:1+B]) into a NaN-filled tensor: the clips before and after stay NaN (no fc store past a clip)."""
    B = 3
    m = torch.from_numpy(synthetic_motion(B, T, seed=61, first=T)).cuda()
    big = torch.full((B + 2, 64, T), float("nan"), device="cuda:0")
    r = enc.latent(m, out=big[1:1 + B])
    torch.cuda.synchronize()
    assert r.data_ptr() == big[1].data_ptr()
    assert torch.isnan(big[0]).all() and torch.isnan(big[B + 1]).all()
    assert torch.equal(big[1:1 + B].cpu(), _encode(enc, m))


def test_reload_follows_new_weights(weights):
    """A second load_state_dict, and a second set_param + finalize on one native encoder (its parameter image is re-uploaded in
    place): the next call follows the new weights."""
    other = motion_encoder_weight_variant("seeded", seed=2)
    m = synthetic_motion(2, 61, seed=67)
    e = MotionEncoder_STGCN("cuda:0").load_state_dict(weights, strict=True)
    first = _encode(e, m)
    e.load_state_dict(other, strict=True)
    second = _encode(e, m)
    _check(second, motion_encoder_latent(other, m), "reloaded")
    assert not torch.equal(first, second)
    n = NativeMotionEncoder(0)
    x = torch.from_numpy(m).cuda()
    for sd in (weights, other):
        for k, v in sd.items():
            n.set_param(k, v)
        n.finalize()
        got = n.encode(x)
        torch.cuda.synchronize()
        assert torch.equal(got.cpu(), first if sd is weights else second)
    n.close()


def test_non_default_stream(enc):
    x = torch.from_numpy(synthetic_motion(3, 61, seed=71)).cuda()
    ref = _encode(enc, x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = enc.latent(x)
    s.synchronize()
    assert torch.equal(got.cpu(), ref)


def test_input_forms(enc):
    """[B, T, 26], a numpy array, a CPU tensor, fp64 input and a non-contiguous slice all equal the contiguous fp32 device call."""
    m = synthetic_motion(3, 33, seed=73)
    ref = _encode(enc, torch.from_numpy(m).cuda())
    wide = torch.from_numpy(synthetic_motion(5, 40, seed=73)).cuda()
    wide[1:4, 3:36] = torch.from_numpy(m).cuda()
    view = wide[1:4, 3:36]
    assert not view.is_contiguous()
    for what, x in (("[B, T, 26]", torch.from_numpy(m.reshape(3, 33, 26)).cuda()), ("numpy", m), ("cpu", torch.from_numpy(m)),
                    ("fp64", torch.from_numpy(m.astype(np.float64)).cuda()), ("slice", view)):
        assert torch.equal(_encode(enc, x), ref), what


NAN_TS = (0, 4, 29, 30, 59, 60, 80, 90)


def test_nan_frame_spreads_as_in_the_reference(enc, weights):
    """One NaN at (clip 1, frame t, one joint): the non-finite latents of clip 1 are the oracle's, frames [t - 10, t + 10] in all
    64 channels, and every other latent (the other clips included) is bit-identical to the clean run.  torch.relu keeps NaN; a
    ReLU that drops it (max(NaN, 0) = 0) gives finite latents here."""
    T = 91
    m = synthetic_motion(3, T, seed=79)
    clean = _encode(enc, m)
    for t in NAN_TS:
        bad = m.copy()
        bad[1, t, 4, 1] = np.nan
        hip = _encode(enc, bad)
        mask = ~torch.isfinite(hip[1])
        want = np.zeros((64, T), bool)
        want[:, max(0, t - RADIUS):min(T, t + RADIUS + 1)] = True
        ref_mask = ~np.isfinite(motion_encoder_latent(weights, bad[1:2])[0].numpy())
        assert np.array_equal(ref_mask, want), t
        assert np.array_equal(mask.numpy(), want), (t, np.nonzero(mask.any(0).numpy())[0])
        assert torch.equal(hip[[0, 2]], clean[[0, 2]]), t
        assert torch.equal(hip[1][~mask], clean[1][~mask]), t
