"""Shared test utilities (tests may import oracle/; the product may not)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ddim_oracle as O  # noqa: E402
from diffusion_conductor_amd.param_spec import DenoiserConfig  # noqa: E402
from diffusion_conductor_amd.synthetic import (batch_mel, batch_music_features, batch_noise,  # noqa: E402,F401
                                               synthetic_state_dict)

GOLDEN = os.path.join(ROOT, "tests", "golden")
_cache = {}


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def rel_l2(a, b):
    a = np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, np.float64)
    b = np.asarray(b.detach().cpu() if torch.is_tensor(b) else b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def cpu_gemm_probe():
    """One float32 F.linear on seeded operands (K = 512, as in the denoiser's GEMMs): its bits tell which CPU GEMM kernel runs."""
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((8, 512), dtype=np.float32))
    w = torch.from_numpy(rng.standard_normal((512, 512), dtype=np.float32) / np.float32(np.sqrt(512)))
    b = torch.from_numpy(rng.standard_normal(512, dtype=np.float32))
    return torch.nn.functional.linear(x, w, b).numpy()


def cpu_gemm_matches_fixtures():
    """The golden fixtures carry the float32 rounding of the CPU GEMMs of the machine that made them (MKL's AVX-512 sgemm).  True
    when this machine's GEMM reproduces g0_cpu_gemm_probe.npz bit for bit: the oracle tests then ask for the fixtures' exact bits.
    Where another kernel sums in another order (MKL takes its AVX2 kernels on AMD CPUs), only a float32 rounding bound can hold."""
    if "gemm" not in _cache:
        _cache["gemm"] = bool(np.array_equal(cpu_gemm_probe(), golden("g0_cpu_gemm_probe.npz")["y"]))
    return _cache["gemm"]


def form_probe(tmp_path_factory):
    """tests/form_probe.cpp, compiled once per session with the host compiler: run(*cases) -> what csrc/dc_form.h decides for each
    case, a list of dicts (one JSON line per case; DC_* variables of the caller's environment do not reach the probe)."""
    import pytest

    from diffusion_conductor_amd import native
    if "form_probe" not in _cache:
        cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
        if not os.path.exists(cxx):
            pytest.skip("no C++ compiler")
        exe = str(tmp_path_factory.mktemp("form") / "form_probe")
        subprocess.run([cxx, "-std=c++17", "-O1", "-I", native.CSRC, os.path.join(ROOT, "tests", "form_probe.cpp"), "-o", exe], check=True)
        _cache["form_probe"] = exe

    def run(*cases):
        env = {k: v for k, v in os.environ.items() if not k.startswith("DC_")}
        out = subprocess.run([_cache["form_probe"]], input="\n".join(cases) + "\n", env=env, check=True, capture_output=True, text=True).stdout
        res = [json.loads(ln) for ln in out.splitlines()]
        assert len(res) == len(cases)
        return res
    return run


# the fields of StepForm tests/form_probe.cpp prints for every step (the modules that compare whole answers name the ones they mean)
STEP_FORM_FIELDS = ("ss", "film_tail", "fs", "ff", "fuse_silu", "folded", "adapt", "wgr", "narrow", "aligned", "layer16", "l16_shared", "upc",
                    "upc16", "upc_narrow", "nwg", "rec_stride", "mixed_form", "embed_next", "fuse_embed", "fuse_extra", "g1_tiles", "upd_flags",
                    "nl_run", "stop_stage")
# ... and what the tests of guidance and of takes compare of a step (the probe prints more: a module names the fields it means)
GUIDED_FIELDS = ("stride", "G", "error", "switch_bits", "key_bits") + STEP_FORM_FIELDS + ("guided", "shared_film", "film_groups")
TAKES_FIELDS = ("B", "stride", "G", "error", "switch_bits", "key_bits", "key_period", "share_period", "share_wrap", "share_groups") + \
    STEP_FORM_FIELDS + ("guided", "shared_film", "film_groups", "film_period", "film_wrap")


def loop_step_probe(tmp_path_factory, fields=None):
    """form_probe for cases that are a captured loop step with a plain successor, in a loop with a tail (a case may say otherwise);
    `fields`: the keys of an answer to keep (the reciprocal's cases, magic_period=, are kept whole)."""
    run = form_probe(tmp_path_factory)

    def steps(*cases):
        res = run(*["form loop=1 graph_step=0 g1_loop=1 next_plain=1 " + c for c in cases])
        return [r if fields is None or "magic" in r else {k: r[k] for k in fields} for r in res]
    return steps


def state_dict_np():
    if "sd" not in _cache:
        _cache["sd"] = synthetic_state_dict(DenoiserConfig(), seed=0)
    return _cache["sd"]


def oracle_params(dtype=torch.float32):
    key = ("p", dtype)
    if key not in _cache:
        _cache[key] = O.to_torch_params(state_dict_np(), dtype)
    return _cache[key]


def xf_pair(B, T, first=0):
    """(xf_proj, xf_out) as encode_music would return them, from seeded stand-in features."""
    p = oracle_params()
    xf = torch.from_numpy(batch_music_features(B, T, first=first))
    return torch.nn.functional.linear(xf, p["proj.weight"], p["proj.bias"]), xf


def make_model(precision="fp16", device="cuda", no_eff=False):
    from diffusion_conductor_amd import MotionTransformer
    m = MotionTransformer(input_feats=26, num_frames=1800, num_layers=8, latent_dim=128, device=device,
                          no_clip=True, precision=precision, no_eff=no_eff)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state_dict_np().items()}, strict=True)
    return m.to(device).eval()


def make_diffusion(S):
    from diffusion_conductor_amd.sampler import (GaussianDiffusion, LossType, ModelMeanType, ModelVarType,
                                                 get_named_beta_schedule)
    return GaussianDiffusion(betas=get_named_beta_schedule("linear", S), model_mean_type=ModelMeanType.START_X,
                             model_var_type=ModelVarType.FIXED_SMALL, loss_type=LossType.MSE)


# ---- the conditioning pre-pass (dc_sampler_set_conditioning): reference and decoders of its buffers ----------------------------
def cond_reference(p, xf, emu=O.FP32, num_layers=8, num_heads=8, stats=None):
    """What the sampling loop reads of `xf_out` [B, N, 64], in the dtype of the parameters `p` and with `emu`'s operand rounding:
    y = linear(xf) [B, N, 512] and, per layer, the cross-attention matrix of linear_cross_attention (transformer.py:149-155):
    text_norm, key / value, softmax of the keys over ALL N music frames (the reference never masks them), einsum('bnhd,bnhl->bhdl')
    -> A [L, B, H, 16 d, 16 l].  p = oracle_params(torch.float64), emu = FP32: the fp64 reference.  `stats`, a dict, receives the
    largest softmax weight."""
    F = torch.nn.functional
    dt = p["linear.weight"].dtype
    with torch.no_grad():
        y = emu.linear(xf.to(dt), p["linear.weight"], p["linear.bias"])
        B, N, _ = y.shape
        A, peak = [], 0.0
        for i in range(num_layers):
            pre = f"temporal_decoder_blocks.{i}.ca_block"
            tn = O._ln(y, p, pre + ".text_norm")
            key = emu.linear(tn, p[pre + ".key.weight"], p[pre + ".key.bias"], big=True)
            key = F.softmax(key.view(B, N, num_heads, -1), dim=1)
            value = emu.linear(tn, p[pre + ".value.weight"], p[pre + ".value.bias"], big=True).view(B, N, num_heads, -1)
            A.append(emu.einsum('bnhd,bnhl->bhdl', key, value))
            peak = max(peak, float(key.max()))
        if stats is not None:
            stats["peak"] = peak
    return y.double().numpy(), (torch.stack(A).double().numpy() if A else None)


def f16_bits_to_f64(u16, fmt):
    """uint16 bit patterns of fp16 (fmt "f16") or bfloat16 ("bf16") values -> float64."""
    u16 = np.ascontiguousarray(u16, np.uint16)
    if fmt == "f16":
        return u16.view(np.float16).astype(np.float64)
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def round_to_16(a, fmt):
    """float64 array rounded to nearest fp16 / bfloat16, as float64."""
    t = torch.from_numpy(np.array(a, np.float64))
    return t.to(torch.float16 if fmt == "f16" else torch.bfloat16).double().numpy()


def decode_pp(raw, B, Tp):
    """"pp" = linear(xf_proj) as the FiLM GEMM's B operand, [G][32 ks][2 halves][64 lanes][4] fp32 (ld_pp, k_cond_pp64): lane
    (c = lane & 31, hh = lane >> 5) of fragment (g, ks) holds features 16 ks + 8 hh + 4 half + i of token 32 g + c
    -> [B, Tp, 512] (token b * Tp + n, Tp = the clip stride) and the rows past B * Tp."""
    G = (B * Tp + 31) // 32
    r = np.asarray(raw, np.float32).reshape(G, 32, 2, 2, 32, 4)              # [g, ks, half, hh, c, i]
    rows = r.transpose(0, 4, 1, 3, 2, 5).reshape(G * 32, 512)                # [g, c | ks, hh, half, i]
    return rows[:B * Tp].reshape(B, Tp, 512), rows[B * Tp:]


def decode_a_ca(raw, L, B):
    """"a_ca", [layer][clip][8 hi + 8 lo frags][64 lanes][8] 16-bit (k_attn_combine's epilogue): fragment 2 oc + s is head
    h = 2 oc + s (feature tile oc, k-step s); lane (c = lane & 31, hh = lane >> 5), element j of it holds
    A[h][d = 8 (j >> 2) + 4 hh + (j & 3)][l = c & 15] where c >> 4 == s - the other half of the lanes are the cross-head entries of
    the 32 x 32 tile, stored as zeros.  -> (hi, lo, off): uint16 [L, B, 8, 16 d, 16 l] twice and the cross-head entries."""
    r = np.asarray(raw, np.uint16).reshape(L, B, 2, 8, 2, 2, 16, 2, 4)       # [L, B, hi|lo, h, hh, c >> 4, l, j >> 2, j & 3]
    out, off = [], []
    for part in range(2):
        heads, others = [], []
        for h in range(8):
            s = h & 1
            blk = r[:, :, part, h, :, s]                                     # [L, B, hh, l, jh, jl]
            heads.append(blk.transpose(0, 1, 4, 2, 5, 3).reshape(L, B, 16, 16))      # d = 8 jh + 4 hh + jl
            others.append(r[:, :, part, h, :, s ^ 1])
        out.append(np.stack(heads, 2))
        off.append(np.stack(others, 2))
    return out[0], out[1], np.stack(off)


def decode_a_ca16(raw, L, B):
    """"a_ca16", [layer][clip][8 heads][64 lanes][8] 16-bit (k_cond_af16): lane (l = lane & 15, q4 = lane >> 4) of head h = 2 oc + s
    holds A[h][d = 4 q4 + i][l] in elements 4 s + i and zeros in the other four.  -> (values uint16 [L, B, 8, 16, 16], the zeros)."""
    r = np.asarray(raw, np.uint16).reshape(L, B, 8, 4, 16, 2, 4)             # [L, B, h, q4, l, j >> 2, i]
    heads, others = [], []
    for h in range(8):
        s = h & 1
        heads.append(r[:, :, h, :, :, s].transpose(0, 1, 2, 4, 3).reshape(L, B, 16, 16))    # d = 4 q4 + i
        others.append(r[:, :, h, :, :, s ^ 1])
    return np.stack(heads, 2), np.stack(others, 2)


def colspace_state_dict(seed=11):
    """The seeded checkpoint with `linear.bias` moved into the column space of `linear.weight` (bias = W u): features near -u make
    linear(x) nearly constant over its 512 outputs, where text_norm's variance meets its eps (tests/study_cond_rstd.py).  -> (sd, u)"""
    sd = {k: np.asarray(v) for k, v in state_dict_np().items()}
    u = np.random.default_rng(seed).standard_normal(64).astype(np.float32)
    sd["linear.bias"] = (sd["linear.weight"].astype(np.float64) @ u.astype(np.float64)).astype(np.float32)
    return sd, u


def rankdef_state_dict():
    """The seeded checkpoint with column 1 of `linear.weight` a copy of column 0: no full column rank, so the least-squares shift of
    the pre-pass has no unique solution and the library keeps the unshifted form (centre_linear, dc_api.hip)."""
    sd = {k: np.asarray(v) for k, v in state_dict_np().items()}
    w = sd["linear.weight"].copy()
    w[:, 1] = w[:, 0]
    sd["linear.weight"] = w
    return sd


def peaky_state_dict(factor=8.0, seed=12):
    """The seeded checkpoint with every ca_block.key.weight times `factor` and log-normal text_norm gains: the key softmax over the
    music frames then puts most of a column's weight on one frame, and most record units combine with weights that underflow."""
    sd = {k: np.asarray(v) for k, v in state_dict_np().items()}
    rng = np.random.default_rng(seed)
    for i in range(8):
        pre = f"temporal_decoder_blocks.{i}.ca_block"
        sd[pre + ".key.weight"] = (sd[pre + ".key.weight"] * np.float32(factor)).astype(np.float32)
        sd[pre + ".text_norm.weight"] = (sd[pre + ".text_norm.weight"] * np.exp(0.5 * rng.standard_normal(512))).astype(np.float32)
    return sd
