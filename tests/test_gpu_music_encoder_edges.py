"""The MusicEncoder's HIP kernels (csrc/dc_music.hip) against the fp64 oracle (oracle/ddim_oracle.py music_encoder + proj) at the
shapes, weights and inputs where they can go wrong, in both activation formats (split bf16 planes, one fp16 plane): lengths around
every tile edge of every kernel, batches that make the persistent tile loops run a second round, tile seams deep inside a long clip,
chunks of clips, weights away from the one seed, constant / ramp / impulse / smooth / large mels, non-finite mels, a reused workspace,
`out=` slices and other streams.  Shape lists: tests/helpers_music_encoder.py, beside the kernel constants they come from.

Bounds.  Every result - xf_out and xf_proj - is compared per clip (rel-L2 over [T, 64]: TOL_ENC_SPLIT = 1e-4, TOL_ENC_F16 = 6e-4 of
test_gpu_parity.py) and per frame (rel-L2 over the 64 channels of one frame, so one wrong frame cannot hide in a long clip:
FRAME_TOL), and xf_proj against the fp64 proj of the GPU's own xf_out (k_me_proj alone: PROJ_TOL).  FRAME_TOL and PROJ_TOL are three
times the worst case measured on an MI355X over all cases here, rounded up to one digit (helpers_music_encoder.py;
profiles/music_encoder_edges_gpu_tests.txt has the worst cases per group):
  split planes  per clip 9.7e-6 (unit impulses)   per frame 1.24e-5 (unit impulses)      -> FRAME_TOL 4e-5
  fp16 plane    per clip 5.4e-4 (constant mel)    per frame 6.23e-4 (20 x 648 white mel)  -> FRAME_TOL 2e-3
  k_me_proj alone, per frame, either format: 6.7e-6 (unit impulses)                       -> PROJ_TOL 3e-5
A planted one-row defect of one layer leaves 2.9e-3 at least on a frame of white mel (tests/test_host_music_encoder_bounds.py)."""
import numpy as np
import pytest
import torch

import helpers_music_encoder as H
from helpers import batch_mel, state_dict_np

from diffusion_conductor_amd.synthetic import (MUSIC_ENCODER_VARIANTS, music_encoder_weight_variant, smooth_mel,
                                               synthetic_m2snet_state_dict)

pytestmark = pytest.mark.gpu
WORST = {}              # group -> format -> [clip, frame, proj alone]: printed when the module is done


def _model(sd=None):
    from diffusion_conductor_amd import MotionTransformer
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    sd = state_dict_np() if sd is None else sd
    m = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device="cuda", no_clip=True, precision="fp16")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return m.to("cuda").eval()


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for group, per in WORST.items():
        for fmt, (c, f, p) in per.items():
            print(f"== {group:34s} {fmt:5s} worst clip {c:.2e}  frame {f:.2e}  proj alone {p:.2e}")


_refs = {}


def _oracle(key, sd, mel):
    """oracle_features, computed once per `key` and left unchanged."""
    if key not in _refs:
        _refs[key] = H.oracle_features(sd, mel)
    return _refs[key]


def _encode(m, mel, fmt, env=None, out=None):
    """(xf_proj, xf_out) of the sampler's encoder in format `fmt`, as host tensors."""
    x = torch.from_numpy(mel) if isinstance(mel, np.ndarray) else mel
    x = x.to("cuda", torch.float32).contiguous()

    def run():
        res = m._ensure_native("cuda:0").encode_music(x, out=out)
        torch.cuda.synchronize()
        return res
    xp, xo = H.with_env({"DC_ME_PREC": fmt, **(env or {})}, run)
    return xp.cpu(), xo.cpu()


class Group:
    """The cases of one test: every case's figures are printed and recorded, and done() fails if any case missed a bound."""

    def __init__(self, name, frame_gate=H.FORMATS):
        self.name, self.failed, self.frame_gate = name, [], frame_gate

    def check(self, got, ref, fmt, what, sd=None):
        (xp, xo), (rxp, rxo) = got, ref
        assert tuple(xo.shape) == rxo.shape and tuple(xp.shape) == rxp.shape, (what, tuple(xo.shape), rxo.shape)
        assert bool(torch.isfinite(xo).all()) and bool(torch.isfinite(xp).all()), what
        (co, fo), (cp, fp) = H.errors(xo, rxo), H.errors(xp, rxp)
        pa = float(H.frame_errors(xp.numpy(), H.oracle_proj(state_dict_np() if sd is None else sd, xo)).max())
        print(f"{self.name} {what} {fmt}: xf_out clip {co:.2e} frame {fo:.2e}  xf_proj clip {cp:.2e} frame {fp:.2e}  proj alone {pa:.2e}")
        w = WORST.setdefault(self.name, {}).setdefault(fmt, [0.0, 0.0, 0.0])
        w[:] = [max(w[0], co, cp), max(w[1], fo, fp), max(w[2], pa)]
        if max(co, cp) > H.clip_tol(fmt) or (fmt in self.frame_gate and max(fo, fp) > H.FRAME_TOL[fmt]) or pa > H.PROJ_TOL:
            self.failed.append((what, fmt, co, cp, fo, fp, pa))

    def done(self):
        assert not self.failed, self.failed


def test_lengths_around_every_tile_edge(model):
    """B = 3 (the middle clip at a non-zero offset) at every Tm of TILE_TMS: the 8-row tiles of the stem and mid kernels on Tm and of
    conv3 on T, the pools' 24-row strips on Tm and on T, the head's 32-frame waves and 128-frame workgroups on B T, all three phases of
    the stride-3 pool, down to the reference's minimum of 4 mel frames."""
    g = Group("tile edges")
    for Tm in H.TILE_TMS:
        mel = batch_mel(3, Tm, first=Tm)
        ref = _oracle(("white", 3, Tm, Tm), state_dict_np(), mel)
        for fmt in H.FORMATS:
            g.check(_encode(model, mel, fmt), ref, fmt, f"Tm={Tm}")
    g.done()


@pytest.mark.parametrize("env", ({"DC_ME_NO_STEM": "1"}, {"DC_ME_NO_MID": "1"}, {"DC_ME_NO_STEM": "1", "DC_ME_NO_MID": "1"}),
                         ids=("no_stem", "no_mid", "neither"))
def test_separate_launches_around_the_tile_edges(model, env):
    """The split format's separate launches - conv1 as conv1.0 (k_me_conv10, bf16x3 MFMAs where the fused stem runs fp32 FMAs) and two
    tiled launches, conv2 as two tiled launches that leave their result in the other buffer - at B = 3 and Tm around the 8-row tiles,
    down to 4 mel frames: the fused forms' bounds, per clip and per frame."""
    g = Group("separate launches " + "+".join(sorted(env)))
    for Tm in (4, 7, 8, 9, 25, 97):
        assert Tm in H.TILE_TMS
        mel = batch_mel(3, Tm, first=Tm)
        g.check(_encode(model, mel, "split", env), _oracle(("white", 3, Tm, Tm), state_dict_np(), mel), "split", f"Tm={Tm}")
    g.done()


def test_second_round_of_the_persistent_tile_loops(model):
    """grid = min(tiles, k CUs): with T = 216 frames per clip (27 conv3 tiles) and the smallest B whose B x 27 tiles exceed 2 CUs, every
    persistent kernel - conv3 included - runs tiles in a second round (the stem and mid kernels have over 3 000 tiles); one clip more
    ends the last round at another place."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    Tm, B = 648, H.loop_batch(ncu)
    T = H.frames(Tm)
    per = -(-T // H.CONV3_ROWS)
    assert T == 216 and B * per > 2 * ncu >= (B - 1) * per, (B, per, ncu)
    mel = batch_mel(B + 1, Tm, first=7)
    rxp, rxo = _oracle(("white", B + 1, Tm, 7), state_dict_np(), mel)
    g = Group("second round")
    for n in (B, B + 1):
        for fmt in H.FORMATS:
            g.check(_encode(model, mel[:n], fmt), (rxp[:n], rxo[:n]), fmt, f"B={n} Tm={Tm} ({ncu} CUs)")
    g.done()


@pytest.mark.parametrize("Tm", (5400, 2700))
def test_tile_seams_deep_in_a_clip(model, Tm):
    """One clip of 60 s / 30 s with the per-frame bound on every frame: a wrong row at a tile seam a thousand rows into the clip is
    5e-4 of the whole tensor and 1e-2 of its frame (the planted defects of test_host_music_encoder_bounds.py)."""
    mel = batch_mel(1, Tm, first=3)
    ref = _oracle(("white", 1, Tm, 3), state_dict_np(), mel)
    g = Group(f"deep seams Tm={Tm}", frame_gate=H.LONG_CLIP_FRAME_GATE)
    for fmt in H.FORMATS:
        g.check(_encode(model, mel, fmt), ref, fmt, f"Tm={Tm}")
    g.done()


@pytest.mark.parametrize("B", (4, 5, 8, 9))
def test_chunks_of_four_clips(model, B):
    """DC_ME_CHUNK=4 at Tm = 25: whole, ragged and several chunks against the oracle; the clips at the chunk edges bit-identical to the
    same clip encoded alone, the whole batch bit-identical to the unchunked call."""
    Tm = 25
    mel = batch_mel(9, Tm, first=50)
    rxp, rxo = _oracle(("white", 9, Tm, 50), state_dict_np(), mel)
    g = Group("chunks of 4")
    for fmt in H.FORMATS:
        got = _encode(model, mel[:B], fmt, {"DC_ME_CHUNK": "4"})
        g.check(got, (rxp[:B], rxo[:B]), fmt, f"B={B}")
        whole = _encode(model, mel[:B], fmt)
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1]), (B, fmt)
        for i in sorted({0, 3, min(4, B - 1), B - 1}):
            alone = _encode(model, mel[i:i + 1], fmt)
            assert torch.equal(got[0][i], alone[0][0]) and torch.equal(got[1][i], alone[1][0]), (B, fmt, i)
    g.done()


def test_natural_chunk_edge_at_full_length(model):
    """B = 33 at Tm = 5400: the library's own chunk of 32 clips, and one clip in a second pass.  The oracle on clips 0, 31 and 32 (a
    clip's oracle features do not depend on its batch: test_host_music_encoder_bounds.py); clip 32 bit-identical to itself alone."""
    Tm, B = 5400, H.CHUNK_FRAMES // 5400 + 1
    assert B == 33
    mel = torch.from_numpy(batch_mel(B, Tm, first=100)).cuda()
    idx = [0, B - 2, B - 1]
    ref = _oracle(("white edge", B, Tm), state_dict_np(), mel[idx].cpu().numpy())
    g = Group("chunk edge 33 x 5400", frame_gate=H.LONG_CLIP_FRAME_GATE)
    for fmt in H.FORMATS:
        xp, xo = _encode(model, mel, fmt)
        g.check((xp[idx], xo[idx]), ref, fmt, f"B={B} clips {idx}")
        ap, ao = _encode(model, mel[B - 1:], fmt)
        assert torch.equal(xp[B - 1], ap[0]) and torch.equal(xo[B - 1], ao[0]), fmt
    g.done()


def test_a_clip_does_not_depend_on_its_batch(model):
    """Tiles never span clips and the head's rows are independent: a clip's bits are the same in a reversed batch and alone."""
    mel = batch_mel(5, 97, first=60)
    for fmt in H.FORMATS:
        xp, xo = _encode(model, mel, fmt)
        rp, ro = _encode(model, mel[::-1].copy(), fmt)
        assert torch.equal(rp.flip(0), xp) and torch.equal(ro.flip(0), xo), fmt
        ap, ao = _encode(model, mel[2:3], fmt)
        assert torch.equal(ap[0], xp[2]) and torch.equal(ao[0], xo[2]), fmt


@pytest.mark.parametrize("value", (0.0, 0.37))
def test_constant_mel_gives_constant_frames(model, value):
    """Reflection padding of a constant is that constant and -inf padding never wins a pool, so every frame sees the same values in the
    same arithmetic: all frames bit-identical to frame 0 (the oracle is exactly constant), and within the bounds.  Zero padding
    anywhere, or padding that wins a max-pool, breaks this at the clip's ends."""
    mel = np.full((2, 49, 128), value, np.float32)
    ref = _oracle(("const", value), state_dict_np(), mel)
    g = Group("constant mel")
    for fmt in H.FORMATS:
        xp, xo = _encode(model, mel, fmt)
        g.check((xp, xo), ref, fmt, f"mel={value}")
        assert torch.equal(xo, xo[:1, :1].expand_as(xo)) and torch.equal(xp, xp[:1, :1].expand_as(xp)), (fmt, value)
    g.done()


def test_ramps_tell_reflect_from_replicate(model):
    mel = H.ramp_mels(49)
    ref = _oracle(("ramps", 49), state_dict_np(), mel)
    g = Group("ramps")
    for fmt in H.FORMATS:
        g.check(_encode(model, mel, fmt), ref, fmt, "time, bins")
    g.done()


def test_unit_impulses_at_the_tile_seams(model):
    """One unit impulse per clip in a zero mel at Tm = 25: rows 0, 1, 7, 8, Tm - 2, Tm - 1 (the image's edges, the first row tile's
    seam) x bins 0, 1, 31, 32, 63, 64, 126, 127 (the image's edges, the stem's 64-bin and the mid kernel's 32-column seams)."""
    mel, cases = H.impulse_mels(25)
    ref = _oracle(("impulses", 25), state_dict_np(), mel)
    g = Group("impulses")
    for fmt in H.FORMATS:
        g.check(_encode(model, mel, fmt), ref, fmt, f"{len(cases)} impulses")
    g.done()


def test_smooth_mel(model):
    mel = np.stack([smooth_mel(b, 271) for b in range(2)])
    ref = _oracle(("smooth", 2, 271), state_dict_np(), mel)
    g = Group("smooth mel")
    for fmt in H.FORMATS:
        g.check(_encode(model, mel, fmt), ref, fmt, "B=2 Tm=271")
    g.done()


def test_large_mel_on_split_planes(model):
    """White mel x 1e3 in the split format only: bf16 planes have fp32's range, while the fp16 plane may legitimately overflow at
    this scale (65 504; the sampler's overflow rescue re-encodes on split planes, test_gpu_robust.py)."""
    mel = batch_mel(2, 97, first=70) * np.float32(1e3)
    g = Group("mel x 1e3")
    g.check(_encode(model, mel, "split"), _oracle(("x1e3", 2, 97), state_dict_np(), mel), "split", "B=2 Tm=97")
    g.done()


@pytest.mark.parametrize("kind", MUSIC_ENCODER_VARIANTS)
def test_weight_variants(kind):
    """Weights loaded through load_state_dict(strict=True): another seed, BatchNorms with negative gains / running_var down to 1e-4 /
    large running_mean (residual.1 and conv4.1 included), a quarter of every layer's channels dead (exact ties in every pool window)
    and the identity-BatchNorm control."""
    sd = music_encoder_weight_variant(kind, seed=1)
    m = _model(sd)
    g = Group(f"weights {kind}")
    for B, Tm in H.WEIGHT_SHAPES:
        mel = batch_mel(B, Tm, first=80 + Tm)
        ref = H.oracle_features(sd, mel)
        for fmt in H.FORMATS:
            g.check(_encode(m, mel, fmt), ref, fmt, f"B={B} Tm={Tm}", sd=sd)
    g.done()


def test_proj_alone(model):
    """k_me_proj against the fp64 proj of the GPU's own xf_out (every case above checks this too; here on features of both formats and
    on a partial wave and a partial workgroup)."""
    g = Group("proj alone")
    for B, Tm in ((1, 4), (3, 97), (1, 385)):
        mel = batch_mel(B, Tm, first=Tm)
        ref = _oracle(("white", B, Tm, Tm), state_dict_np(), mel)
        for fmt in H.FORMATS:
            g.check(_encode(model, mel, fmt), ref, fmt, f"B={B} Tm={Tm}")
    g.done()


def _nan_case(model, value, chunk=None):
    Tm = 97
    mel = batch_mel(3, Tm, first=90)
    sd = state_dict_np()
    env = {"DC_ME_CHUNK": chunk} if chunk else None
    for fmt in H.FORMATS:
        clean = _encode(model, mel, fmt, env)
        for t in H.NAN_TS:
            bad = mel.copy()
            refs = {}
            for v in (np.nan, value):
                bad[1, t, 64] = v
                refs[str(v)] = _oracle(("nonfinite", t, str(v)), sd, bad[1:2].copy())
            lo, hi = H.nonfinite_run(refs["nan"][1][0])
            assert hi > lo and H.nonfinite_run(refs["nan"][0][0]) == (lo, hi)
            xp, xo = _encode(model, bad, fmt, env)
            for got, ref, cl in ((xp, refs[str(value)][0], clean[0]), (xo, refs[str(value)][1], clean[1])):
                if np.isnan(value):          # exactly the oracle's run, in all 64 channels
                    assert H.nonfinite_run(got[1].numpy()) == (lo, hi), (fmt, t, H.nonfinite_run(got[1].numpy()), (lo, hi))
                else:                        # every frame the oracle makes non-finite is; nothing outside the NaN case's run differs
                    assert not np.isfinite(got[1].numpy()[~np.isfinite(ref[0])]).any(), (fmt, t, value)
                assert torch.equal(got[[0, 2]], cl[[0, 2]]), (fmt, t, value)
                keep = np.r_[0:lo, hi:got.shape[1]]
                assert torch.equal(got[1][keep], cl[1][keep]), (fmt, t, value)


def test_nan_spreads_as_in_the_reference(model):
    """One NaN at mel[1, t, 64] of three clips at Tm = 97 (a log-mel of digital silence holds -inf, and NaN after min-max
    normalisation): torch.relu and max_pool2d keep NaN, so the reference returns NaN for the frames whose receptive field holds it.
    The non-finite frames of clip 1 are exactly the oracle's run, in all 64 channels of xf_out and xf_proj; clips 0 and 2 and the
    finite frames of clip 1 are bit-identical to the clean run.  A ReLU or a pool that drops NaN (fmaxf) returns finite, wrong
    features here - and hides what the sampler's fp16 overflow rescue looks for."""
    _nan_case(model, np.nan)


@pytest.mark.parametrize("value", (np.inf, -np.inf))
def test_infinite_mel(model, value):
    """+-inf at the same places: every frame the oracle makes non-finite is non-finite, and nothing outside the NaN case's run differs
    from the clean run (an infinity may be a NaN a layer earlier than in the reference: inf as two bf16 planes is inf + NaN)."""
    _nan_case(model, value)


def test_nan_beside_a_chunk_edge(model):
    """DC_ME_CHUNK=1: the NaN clip is a pass of its own between two others."""
    _nan_case(model, np.nan, chunk="1")


WORKSPACE_SHAPES = ((2, 97), (1, 2700), (40, 25), (3, 97), (1, 4))


def test_workspace_grows_in_clips_and_in_frames():
    """One sampler through shapes that grow the activation planes' clip capacity and frame capacity independently and then shrink:
    each result is bit-identical to that of a sampler which has seen no other shape."""
    used = _model()
    for B, Tm in WORKSPACE_SHAPES:
        mel = batch_mel(B, Tm, first=B + Tm)
        fresh = _model()
        for fmt in H.FORMATS:
            got, want = _encode(used, mel, fmt), _encode(fresh, mel, fmt)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (fmt, B, Tm)


def test_non_default_stream(model):
    mel = torch.from_numpy(batch_mel(3, 97, first=95)).cuda()
    for fmt in H.FORMATS:
        ref = _encode(model, mel, fmt)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())

        def run():
            with torch.cuda.stream(s):
                out = model._ensure_native("cuda:0").encode_music(mel)
            s.synchronize()
            return out
        xp, xo = H.with_env({"DC_ME_PREC": fmt}, run)
        assert torch.equal(xp.cpu(), ref[0]) and torch.equal(xo.cpu(), ref[1]), fmt


@pytest.mark.parametrize("Tm", (4, 25, 97))
def test_out_slices_keep_their_neighbours(model, Tm):
    """encode_music(out=(big_p[1:1 + B], big_o[1:1 + B])) into NaN-filled tensors, T = 2, 9, 33, whole and in chunks of 2 clips: the
    clips before and after stay NaN (neither the head nor proj stores past a pass's B T frames), the slice holds the plain result."""
    B, T = 3, H.frames(Tm)
    mel = batch_mel(B, Tm, first=97 + Tm)
    for fmt in H.FORMATS:
        ref = _encode(model, mel, fmt)
        for env in (None, {"DC_ME_CHUNK": "2"}):
            big = [torch.full((B + 2, T, 64), float("nan"), device="cuda:0") for _ in range(2)]
            _encode(model, mel, fmt, env, out=(big[0][1:1 + B], big[1][1:1 + B]))
            for k in range(2):
                assert torch.isnan(big[k][0]).all() and torch.isnan(big[k][B + 1]).all(), (fmt, Tm, env)
                assert torch.equal(big[k][1:1 + B].cpu(), ref[k]), (fmt, Tm, env)


def test_sampler_and_m2snet_share_one_encoder(model):
    """The same `music_encoder.*` weights behind two handles: the sampler's xf_out on split planes and M2SNet.music_latent are
    bit-identical at (3, 97).  M2SNet's encoder is pinned to split planes (its latents feed a learned score), so DC_ME_PREC=f16
    changes the sampler's result and not M2SNet's.  (Generator against M2SNet: test_gpu_m2sgan.py.)"""
    from diffusion_conductor_amd.m2snet import M2SNet
    sd = synthetic_m2snet_state_dict(seed=0)
    for k, v in state_dict_np().items():
        if k.startswith("music_encoder.") and not k.endswith("num_batches_tracked"):
            assert np.array_equal(sd[k], v), k
    net = M2SNet("cuda:0").load_state_dict(sd, strict=True)
    mel = batch_mel(3, 97, first=99)
    split = _encode(model, mel, "split")[1]
    for fmt in H.FORMATS:
        lat = H.with_env({"DC_ME_PREC": fmt}, lambda: net.music_latent(mel))
        torch.cuda.synchronize()
        assert torch.equal(lat.cpu(), split), fmt
    assert not torch.equal(_encode(model, mel, "f16")[1], split)
