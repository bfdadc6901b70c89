"""ctypes binding of libdc_ddim.so (include/dc_ddim.h).

There is deliberately no fallback: if the shared library is missing or no gfx950 device
is visible, construction raises.  PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdc_ddim.so")
CSRC = os.path.join(_HERE, "csrc")

DC_PREC = {"bf16": 0, "mixed": 1, "bf16x3": 2, "fp16": 3}

EXPORTS = [
    "dc_last_error", "dc_version", "dc_linear_beta_schedule", "dc_ddim_coefficients", "dc_pack_weight",
    "dc_sampler_create", "dc_sampler_destroy", "dc_sampler_set_param", "dc_sampler_finalize_params",
    "dc_sampler_set_conditioning", "dc_sampler_encode_music", "dc_sampler_set_encoder_format", "dc_sampler_set_precise_tail", "dc_precise_tail_default", "dc_sampler_set_precise_forward", "dc_sampler_set_combine_exchange", "dc_sampler_set_clip_aligned", "dc_sampler_set_idle_wave_path", "dc_sampler_denoise", "dc_sampler_ddim_loop", "dc_sampler_profile_loop",
    "dc_kernel_name", "dc_kernel_count", "dc_sampler_workspace_bytes", "dc_sampler_clip_stride", "dc_sampler_debug_denoise",
    "dc_sampler_debug_read", "dc_sampler_debug_layer", "dc_savgol_coefficients", "dc_savgol_filter",
    "dc_ddim_coefficients_ex", "dc_sampler_ddim_loop_ex", "dc_sampler_status", "dc_sampler_set_smoothing",
    "dc_sampler_set_step_noise_seed", "dc_sampler_set_step_noise_seed_at", "dc_step_noise_fill",
    "dc_motion_encoder_create", "dc_motion_encoder_destroy", "dc_motion_encoder_set_param", "dc_motion_encoder_finalize",
    "dc_motion_encoder_encode",
    "dc_ddim_coefficients_known", "dc_sampler_set_known",
    "dc_sampler_set_conditioning_guided", "dc_sampler_set_guidance_scale",
    "dc_m2snet_create", "dc_m2snet_destroy", "dc_m2snet_set_param", "dc_m2snet_finalize", "dc_m2snet_encode_music", "dc_m2snet_fuse",
    "dc_m2snet_score", "dc_m2snet_fuse_pairs", "dc_m2snet_pairs_share",
    "dc_solver_table", "dc_sampler_solver_loop", "dc_sampler_solver_profile_loop",
    "dc_sampler_set_conditioning_takes",
    "dc_sampler_set_conditioning_windows", "dc_windows_check",
    "dc_q_sample_coefficients", "dc_q_sample", "dc_motion_loss_terms", "dc_latent_l1",
    "dc_vb_coefficients", "dc_vb_workspace_floats", "dc_vb_terms", "dc_prior_kl",
    "dc_m2sgan_create", "dc_m2sgan_destroy", "dc_m2sgan_set_param", "dc_m2sgan_finalize", "dc_m2sgan_features", "dc_m2sgan_decode",
    "dc_m2sgan_generate", "dc_m2sgan_debug_blocks", "dc_m2sgan_fold_conv", "dc_m2sgan_set_decoder",
    "dc_bilstm_create", "dc_bilstm_destroy", "dc_bilstm_set_param", "dc_bilstm_finalize", "dc_bilstm_input_size", "dc_bilstm_decode",
    "dc_bilstm_hidden", "dc_bilstm_pass_clips",
    "dc_rhythm_create", "dc_rhythm_destroy", "dc_rhythm_psd", "dc_rhythm_contour", "dc_rhythm_motion_beats", "dc_rhythm_beat_scores",
    "dc_discriminator_create", "dc_discriminator_destroy", "dc_discriminator_set_param", "dc_discriminator_finalize",
    "dc_discriminator_features", "dc_discriminator_score",
    "dc_mel_create", "dc_mel_destroy", "dc_mel_tables", "dc_mel_out_frames", "dc_mel_pass_clips", "dc_mel_power", "dc_mel_features",
]

UPDATE_CLIP_DENOISED, UPDATE_EPSILON = 1, 2          # flags of dc_sampler_ddim_loop_ex
STATUS_NONFINITE, STATUS_F16_SATURATED, STATUS_TIMEOUT = 1, 2, 4        # bits of dc_sampler_status
SOLVER_ROW = 12                                       # DC_SOLVER_ROW: floats per row of dc_solver_table
SOLVER_ORDER = {"ddim": 1, "dpmpp2m": 2}              # solver= of the Python surfaces -> order of dc_solver_table
LOSS_TERMS = 8                                        # DC_LOSS_TERMS: floats per clip of dc_motion_loss_terms
VB_TERMS = 8                                          # DC_VB_TERMS: floats per clip of dc_vb_terms
VB_COEF = 12                                          # DC_VB_COEF: floats per clip of dc_vb_coefficients
VB_MEAN = {"PREVIOUS_X": 1, "START_X": 2, "EPSILON": 3}                                  # DC_VB_MEAN_*
VB_VAR = {"LEARNED": 1, "FIXED_SMALL": 2, "FIXED_LARGE": 3, "LEARNED_RANGE": 4}          # DC_VB_VAR_*


class DcConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("input_feats", "num_frames", "latent_dim", "ff_size", "num_layers",
                                         "num_heads", "no_eff", "precision", "max_timesteps", "device")]


class DcError(RuntimeError):
    pass


SOURCES = ("dc_kernels.hip", "dc_api.hip", "dc_music.hip", "dc_layer16.hip", "dc_stgcn.hip", "dc_m2snet.hip", "dc_loss.hip", "dc_m2sgan.hip",
           "dc_rhythm.hip", "dc_bilstm.hip", "dc_mel.hip")
HEADERS = ("dc_common.h", "dc_dev.h", "dc_form.h", "dc_handle.h", "dc_launch.h", "dc_mfma_f32.h", "dc_music.h", "dc_pack.h")
EXTRA_FLAGS = {}      # per-source compiler flags


def build_library(force: bool = False, verbose: bool = False, out: str = None, objdir: str = None, extra_flags=()) -> str:
    """Compile csrc/*.hip for gfx950 into libdc_ddim.so (hipcc cross-compiles without a GPU).  Each source becomes an
    object under build/ (compiled in parallel, rebuilt only when it or a header changed), then one link.  A/B variants
    (tools/ab.sh): `out` names another library, `objdir` its own object directory (objects built with other flags must
    not mix), `extra_flags` go to every compile."""
    out = out or LIB_PATH
    srcs = [os.path.join(CSRC, f) for f in SOURCES if os.path.exists(os.path.join(CSRC, f))]
    hdrs = [os.path.join(CSRC, f) for f in HEADERS if os.path.exists(os.path.join(CSRC, f))] + \
        [os.path.join(os.path.dirname(_HERE), "include", "dc_ddim.h")]
    hmax = max(os.path.getmtime(h) for h in hdrs)
    bdir = objdir or os.path.join(_HERE, "build")
    os.makedirs(bdir, exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wno-unused-value", *extra_flags]
    objs, jobs = [], []
    for src in srcs:
        obj = os.path.join(bdir, os.path.basename(src).replace(".hip", ".o"))
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(os.path.getmtime(src), hmax):
            cmd = [hipcc, *flags, *EXTRA_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            jobs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in jobs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    if jobs or not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(o) for o in objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", out]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return out


_lib = None


def lib():
    """Load the shared library (never builds implicitly on a GPU box: the prebuilt .so travels)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("DC_DDIM_LIB", LIB_PATH)      # A/B builds of the same ABI side by side (tools/ab.sh); default in-tree
    if not os.path.exists(path):
        raise DcError(f"{path} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback for the sampler)")
    # PyTorch-ROCm ships its own libamdhip64: it must be the copy this process binds (the tensors, streams and the library's
    # kernels have to live in ONE HIP runtime).  Loaded after ours, it becomes a second runtime and the library's own one
    # (/opt/rocm's) sees no device - so torch goes first, also when a caller only wants build() + version().
    import torch  # noqa: F401
    L = C.CDLL(path)
    L.dc_last_error.restype = C.c_char_p
    L.dc_version.restype = C.c_char_p
    L.dc_kernel_name.restype = C.c_char_p
    L.dc_kernel_name.argtypes = [C.c_int32]
    L.dc_kernel_count.restype = C.c_int32
    L.dc_sampler_workspace_bytes.restype = C.c_int64
    L.dc_sampler_workspace_bytes.argtypes = [C.c_void_p]
    L.dc_sampler_clip_stride.restype = C.c_int32
    L.dc_sampler_clip_stride.argtypes = [C.c_void_p]
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    L.dc_linear_beta_schedule.argtypes = [C.c_int32, dp, dp, dp, dp, dp]
    L.dc_ddim_coefficients.argtypes = [C.c_int32, dp, fp]
    L.dc_pack_weight.argtypes = [fp, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]
    L.dc_sampler_create.argtypes = [C.POINTER(DcConfig), C.POINTER(C.c_void_p)]
    L.dc_sampler_destroy.argtypes = [C.c_void_p]
    L.dc_sampler_destroy.restype = None
    L.dc_sampler_set_param.argtypes = [C.c_void_p, C.c_char_p, fp, C.c_int64]
    L.dc_sampler_finalize_params.argtypes = [C.c_void_p]
    L.dc_sampler_set_conditioning.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, ip, C.c_int32, C.c_int32, C.c_void_p]
    L.dc_sampler_encode_music.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    L.dc_sampler_set_encoder_format.argtypes = [C.c_void_p, C.c_int32]
    L.dc_sampler_set_precise_tail.argtypes = [C.c_void_p, C.c_int32]
    L.dc_sampler_set_combine_exchange.argtypes = [C.c_void_p, C.c_int32]
    L.dc_sampler_set_clip_aligned.argtypes = [C.c_void_p, C.c_int32]
    L.dc_sampler_set_idle_wave_path.argtypes = [C.c_void_p, C.c_int32]
    L.dc_precise_tail_default.argtypes = [C.c_int32]
    L.dc_precise_tail_default.restype = C.c_int32
    L.dc_sampler_set_precise_forward.argtypes = [C.c_void_p, C.c_int32]
    L.dc_sampler_denoise.argtypes = [C.c_void_p, C.c_void_p, ip, C.c_void_p, C.c_void_p]
    L.dc_savgol_coefficients.argtypes = [C.c_int32, C.c_int32, fp]
    L.dc_savgol_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.dc_sampler_ddim_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, fp, ip, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_ddim_coefficients_ex.argtypes = [C.c_int32, dp, C.c_float, fp]
    L.dc_sampler_ddim_loop_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, fp, C.c_int32, C.c_void_p, ip, C.c_int32,
                                          C.c_void_p, C.c_void_p]
    L.dc_ddim_coefficients_known.argtypes = [C.c_int32, dp, C.c_float, fp, fp]
    L.dc_solver_table.argtypes = [C.c_int32, dp, ip, C.c_int32, C.c_float, C.c_int32, fp, fp]
    L.dc_sampler_solver_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, ip, fp, C.c_int32, C.c_void_p, ip, C.c_int32,
                                         C.c_void_p, C.c_void_p]
    L.dc_sampler_solver_profile_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, ip, fp, C.c_int32, fp, ip, C.c_int32,
                                                 C.c_void_p]
    L.dc_sampler_set_known.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dc_sampler_set_conditioning_guided.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, ip, C.c_int32, C.c_int32, fp, fp, C.c_void_p]
    L.dc_sampler_set_guidance_scale.argtypes = [C.c_void_p, C.c_float]
    L.dc_sampler_set_conditioning_takes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, ip, C.c_int32, C.c_int32, C.c_int32, fp, fp, C.c_void_p]
    L.dc_sampler_set_conditioning_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, ip, ip, fp, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                                      fp, fp, C.c_void_p]
    L.dc_windows_check.argtypes = [ip, fp, C.c_int32, C.c_int32, C.c_int32, ip]
    L.dc_sampler_set_step_noise_seed.argtypes = [C.c_void_p, C.c_uint64]
    L.dc_sampler_set_step_noise_seed_at.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.dc_step_noise_fill.argtypes = [C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_void_p]
    L.dc_sampler_status.argtypes = [C.c_void_p, ip, C.c_int32]
    L.dc_sampler_set_smoothing.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.dc_sampler_debug_denoise.argtypes = [C.c_void_p, C.c_void_p, ip, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    L.dc_sampler_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]
    L.dc_sampler_debug_layer.argtypes = [C.c_void_p, fp, ip, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    L.dc_sampler_profile_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, fp, fp, ip, C.c_int32, C.c_void_p]
    L.dc_motion_encoder_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.dc_motion_encoder_destroy.argtypes = [C.c_void_p]
    L.dc_motion_encoder_destroy.restype = None
    L.dc_motion_encoder_set_param.argtypes = [C.c_void_p, C.c_char_p, fp, C.c_int64]
    L.dc_motion_encoder_finalize.argtypes = [C.c_void_p]
    L.dc_motion_encoder_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_m2snet_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.dc_m2snet_destroy.argtypes = [C.c_void_p]
    L.dc_m2snet_destroy.restype = None
    L.dc_m2snet_set_param.argtypes = [C.c_void_p, C.c_char_p, fp, C.c_int64]
    L.dc_m2snet_finalize.argtypes = [C.c_void_p]
    L.dc_m2snet_encode_music.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_m2snet_fuse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dc_m2snet_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                  C.c_void_p]
    L.dc_m2snet_fuse_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, ip, ip, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
    L.dc_m2snet_pairs_share.restype = C.c_int32
    L.dc_m2snet_pairs_share.argtypes = []
    L.dc_q_sample_coefficients.argtypes = [C.c_int32, dp, ip, C.c_int32, fp, fp]
    L.dc_q_sample.argtypes = [C.c_void_p, C.c_void_p, fp, fp, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_uint64,
                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.dc_motion_loss_terms.argtypes = [C.c_void_p, C.c_void_p, ip, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_latent_l1.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_vb_coefficients.argtypes = [C.c_int32, dp, C.c_int32, ip, C.c_int32, fp]
    L.dc_vb_workspace_floats.restype = C.c_int64
    L.dc_vb_workspace_floats.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    L.dc_vb_terms.argtypes = [C.c_void_p] * 5 + [fp] + [C.c_int32] * 6 + [C.c_void_p, C.c_void_p, C.c_void_p]
    L.dc_prior_kl.argtypes = [C.c_void_p, fp, fp, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_m2sgan_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.dc_m2sgan_destroy.argtypes = [C.c_void_p]
    L.dc_m2sgan_destroy.restype = None
    L.dc_m2sgan_set_param.argtypes = [C.c_void_p, C.c_char_p, fp, C.c_int64]
    L.dc_m2sgan_finalize.argtypes = [C.c_void_p]
    L.dc_m2sgan_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_m2sgan_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_m2sgan_generate.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_m2sgan_debug_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_m2sgan_fold_conv.argtypes = [fp] * 7 + [C.c_int32] * 3 + [fp, fp]
    L.dc_m2sgan_set_decoder.argtypes = [C.c_void_p, C.c_int32]
    L.dc_bilstm_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.dc_bilstm_destroy.argtypes = [C.c_void_p]
    L.dc_bilstm_destroy.restype = None
    L.dc_bilstm_set_param.argtypes = [C.c_void_p, C.c_char_p, fp, C.c_int64]
    L.dc_bilstm_finalize.argtypes = [C.c_void_p]
    L.dc_bilstm_input_size.argtypes = [C.c_void_p]
    L.dc_bilstm_input_size.restype = C.c_int32
    L.dc_bilstm_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_bilstm_hidden.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_bilstm_pass_clips.argtypes = [C.c_int32, C.c_int32]
    L.dc_bilstm_pass_clips.restype = C.c_int32
    L.dc_rhythm_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.dc_rhythm_destroy.argtypes = [C.c_void_p]
    L.dc_rhythm_destroy.restype = None
    L.dc_rhythm_psd.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_rhythm_contour.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dc_rhythm_motion_beats.argtypes = [C.c_void_p, C.c_void_p, ip, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.dc_rhythm_beat_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.dc_discriminator_create.argtypes = [C.c_int32, C.POINTER(C.c_void_p)]
    L.dc_discriminator_destroy.argtypes = [C.c_void_p]
    L.dc_discriminator_destroy.restype = None
    L.dc_discriminator_set_param.argtypes = [C.c_void_p, C.c_char_p, fp, C.c_int64]
    L.dc_discriminator_finalize.argtypes = [C.c_void_p]
    L.dc_discriminator_features.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_discriminator_score.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_mel_create.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.dc_mel_destroy.argtypes = [C.c_void_p]
    L.dc_mel_destroy.restype = None
    L.dc_mel_tables.argtypes = [C.c_int32, fp, fp, ip, ip, fp, C.c_int32, ip]
    L.dc_mel_out_frames.argtypes = [C.c_int64, C.c_int32]
    L.dc_mel_out_frames.restype = C.c_int32
    L.dc_mel_pass_clips.argtypes = [C.c_int32]
    L.dc_mel_pass_clips.restype = C.c_int32
    L.dc_mel_power.argtypes = [C.c_void_p, C.c_void_p, ip, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.dc_mel_features.argtypes = [C.c_void_p, C.c_void_p, ip, C.c_int32, C.c_int32, ip, C.c_int32, C.c_void_p, C.c_void_p]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise DcError(f"libdc_ddim error {rc}: {lib().dc_last_error().decode()}")


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _iptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


# ---------------------------------------------------------------------------------------
# host-only helpers (work without a GPU)
# ---------------------------------------------------------------------------------------
def linear_beta_schedule(num_steps: int) -> dict:
    """dc_linear_beta_schedule: the fp64 tables of GaussianDiffusion.__init__."""
    n = int(num_steps)
    arrs = [np.empty(n, np.float64) for _ in range(5)]
    dp = C.POINTER(C.c_double)
    _check(lib().dc_linear_beta_schedule(n, *[a.ctypes.data_as(dp) for a in arrs]))
    keys = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")
    return dict(zip(keys, arrs))


def ddim_coefficients(alphas_cumprod: np.ndarray, eta=None) -> np.ndarray:
    """eta None: dc_ddim_coefficients, [S, 4] (eta = 0).  eta a float: dc_ddim_coefficients_ex, [S, 8] with sigma folded in."""
    ac = np.ascontiguousarray(alphas_cumprod, np.float64)
    dp = ac.ctypes.data_as(C.POINTER(C.c_double))
    if eta is None:
        out = np.empty((ac.shape[0], 4), np.float32)
        _check(lib().dc_ddim_coefficients(ac.shape[0], dp, _fptr(out)))
    else:
        out = np.empty((ac.shape[0], 8), np.float32)
        _check(lib().dc_ddim_coefficients_ex(ac.shape[0], dp, C.c_float(float(eta)), _fptr(out)))
    return out


def ddim_coefficients_known(alphas_cumprod: np.ndarray, eta=0.0):
    """dc_ddim_coefficients_known: ([S, 8] table of a loop around known values - dc_ddim_coefficients_ex's plus slot 5 =
    sqrt(1 - abar_prev) and slots 6, 7 = sqrt(abar), sqrt(1 - abar) -, the loop's starting pair [2])."""
    ac = np.ascontiguousarray(alphas_cumprod, np.float64)
    out, start = np.empty((ac.shape[0], 8), np.float32), np.empty(2, np.float32)
    _check(lib().dc_ddim_coefficients_known(ac.shape[0], ac.ctypes.data_as(C.POINTER(C.c_double)), C.c_float(float(eta)), _fptr(out),
                                            _fptr(start)))
    return out, start


def solver_table(alphas_cumprod: np.ndarray, timesteps, eta=0.0, order=1):
    """dc_solver_table: ([n, SOLVER_ROW] rows of a loop over `timesteps` - a strictly decreasing sub-sequence of the training
    schedule `alphas_cumprod` -, the loop's starting pair [2]).  Slots 0..7 are ddim_coefficients_known's on the sub-schedule, slot 8
    the history coefficient of the second-order multistep update (order 2; 0 at order 1).  DcError for a bad list, order or eta."""
    ac = np.ascontiguousarray(alphas_cumprod, np.float64)
    ts = np.ascontiguousarray(np.asarray(timesteps).reshape(-1), np.int32)
    rows, start = np.zeros((max(ts.shape[0], 1), SOLVER_ROW), np.float32), np.empty(2, np.float32)
    _check(lib().dc_solver_table(ac.shape[0], ac.ctypes.data_as(C.POINTER(C.c_double)), _iptr(ts), ts.shape[0], C.c_float(float(eta)),
                                 int(order), _fptr(rows), _fptr(start)))
    return rows, start


def savgol_coefficients(window: int, order: int) -> np.ndarray:
    """dc_savgol_coefficients: the [window, window] hat matrix (host only)."""
    out = np.empty((window, window), np.float32)
    _check(lib().dc_savgol_coefficients(int(window), int(order), _fptr(out)))
    return out


def windows_check(starts, weights, T: int, L: int, length=None):
    """dc_windows_check: the host's check of a plan of overlapping windows (starts [W], weights fp32 [W, T], pieces of L frames);
    ValueError with the library's reason for a plan dc_sampler_set_conditioning_windows refuses (DC_ERR_INVALID)."""
    st = np.ascontiguousarray(np.asarray(starts).reshape(-1), np.int32)
    wt = np.ascontiguousarray(np.asarray(weights), np.float32).reshape(-1)
    if wt.shape[0] != st.shape[0] * int(T):
        raise ValueError(f"weights must be {(st.shape[0], int(T))}")
    ln = None if length is None else np.ascontiguousarray(np.asarray(length).reshape(-1), np.int32)
    rc = lib().dc_windows_check(_iptr(st), _fptr(wt), st.shape[0], int(T), int(L), None if ln is None else _iptr(ln))
    if rc != 0:
        raise ValueError(lib().dc_last_error().decode())


def savgol_filter(poses, window: int = 19, order: int = 5):
    """dc_savgol_filter on a CUDA(ROCm) fp32 tensor [B, T, P] (or [B, T, J, 2]); returns a new tensor."""
    import torch
    assert poses.is_cuda and poses.dtype == torch.float32
    x = poses.contiguous()
    B, T = x.shape[0], x.shape[1]
    P = x.numel() // (B * T)
    out = torch.empty_like(x)
    _check(lib().dc_savgol_filter(x.data_ptr(), out.data_ptr(), B, T, P, int(window), int(order),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def step_noise(shape, seed: int, iteration: int, device):
    """dc_step_noise_fill: the library's N(0, 1) draws of one DDIM iteration for `seed` as a new fp32 tensor of `shape` on `device`
    (what a seeded eta > 0 loop adds at that iteration)."""
    import torch
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _check(lib().dc_step_noise_fill(out.data_ptr(), out.numel(), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(iteration),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def q_sample_coefficients(alphas_cumprod: np.ndarray, timesteps):
    """dc_q_sample_coefficients: (a [B], s [B]) = (float)sqrt(abar[t]), (float)sqrt(1 - abar[t]) per clip (host only).  DcError for a
    timestep outside the schedule."""
    ac = np.ascontiguousarray(alphas_cumprod, np.float64)
    ts = np.ascontiguousarray(np.asarray(timesteps.cpu() if hasattr(timesteps, "cpu") else timesteps).reshape(-1), np.int32)
    a, s = np.empty(max(ts.shape[0], 1), np.float32), np.empty(max(ts.shape[0], 1), np.float32)
    _check(lib().dc_q_sample_coefficients(ac.shape[0], ac.ctypes.data_as(C.POINTER(C.c_double)), _iptr(ts), ts.shape[0], _fptr(a), _fptr(s)))
    return a, s


def _loss_tensor(t, name, shape=None):
    import torch
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), f"{name} must be a contiguous fp32 device tensor"
    assert shape is None or tuple(t.shape) == tuple(shape), f"{name} must be {tuple(shape)}, got {tuple(t.shape)}"
    return t


def q_sample(x_start, a, s, noise=None, noise_seed=None, return_noise=False):
    """dc_q_sample on fp32 device tensors: x_t = a_b x_start + s_b noise over [B, T, ...] with the host arrays (a, s) of
    q_sample_coefficients.  `noise`: the tensor to use; else `noise_seed` = seed or (seed, iteration, first_element): the library's
    draws (step_noise's for (seed, iteration), starting at first_element).  return_noise: (x_t, the draws) - seeded path only."""
    import torch
    x = _loss_tensor(x_start, "x_start")
    B, T = int(x.shape[0]), int(x.shape[1])
    P = x.numel() // max(B * T, 1)
    a, s = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(s, np.float32)
    assert a.shape == (B,) and s.shape == (B,), "one (a, s) pair per clip"
    xt = torch.empty_like(x)
    seed = it = first = 0
    zout = None
    if noise is not None:
        assert noise_seed is None and not return_noise, "noise= and noise_seed= exclude each other"
        _loss_tensor(noise, "noise", x.shape)
    else:
        assert noise_seed is not None, "q_sample needs noise= or noise_seed="
        seed, it, first = noise_seed if isinstance(noise_seed, (tuple, list)) else (noise_seed, 0, 0)
        zout = torch.empty_like(x) if return_noise else None
    with torch.cuda.device(x.device):
        _check(lib().dc_q_sample(x.data_ptr(), None if noise is None else noise.data_ptr(), _fptr(a), _fptr(s), B, T, P,
                                 C.c_uint64(int(seed) & (2 ** 64 - 1)), int(it), C.c_uint64(int(first)),
                                 None if zout is None else zout.data_ptr(), xt.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return (xt, zout) if return_noise else xt


def motion_loss_terms(pred, target, length=None):
    """dc_motion_loss_terms: pred, target fp32 [B, T, 26] on the device, length [B] (None: all T) -> terms fp32 [B, LOSS_TERMS] per
    clip: mse, masked reconstruction sum, velocity body / elbow / head, velocity, 0, 0 (include/dc_ddim.h)."""
    import torch
    p = _loss_tensor(pred, "pred")
    B, T = int(p.shape[0]), int(p.shape[1])
    P = p.numel() // max(B * T, 1)
    g = _loss_tensor(target, "target", p.shape)
    lp = None
    if length is not None:
        la = np.ascontiguousarray(np.asarray(length.cpu() if hasattr(length, "cpu") else length).reshape(-1), np.int32)
        assert la.shape == (B,), "one length per clip"
        lp = _iptr(la)
    out = torch.empty((B, LOSS_TERMS), dtype=torch.float32, device=p.device)
    with torch.cuda.device(p.device):
        _check(lib().dc_motion_loss_terms(p.data_ptr(), g.data_ptr(), lp, B, T, P, out.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def latent_l1(a, b):
    """dc_latent_l1: latents fp32 [B, 64, T] on the device -> the per-clip mean |a - b|, fp32 [B]."""
    import torch
    a = _loss_tensor(a, "a")
    assert a.dim() == 3 and a.shape[1] == 64, f"latents are [B, 64, T], got {tuple(a.shape)}"
    b = _loss_tensor(b, "b", a.shape)
    out = torch.empty((int(a.shape[0]),), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _check(lib().dc_latent_l1(a.data_ptr(), b.data_ptr(), int(a.shape[0]), int(a.shape[2]), out.data_ptr(),
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def _vb_type(table, v, what):
    """A DC_VB_MEAN_* / DC_VB_VAR_* number from an enum member (by name), a name or the number itself."""
    name = getattr(v, "name", v)
    if isinstance(name, str):
        if name not in table:
            raise ValueError(f"{what} must be one of {sorted(table)}, got {name!r}")
        return table[name]
    return int(name)


def vb_coefficients(betas: np.ndarray, var_type, timesteps):
    """dc_vb_coefficients: fp32 [B, VB_COEF] per clip - posterior_mean_coef1 / coef2, posterior_log_variance_clipped, the model's fixed
    log-variance (LEARNED_RANGE: max_log), sqrt_recip / sqrt_recipm1_alphas_cumprod, the t == 0 flag, 1 / coef1, coef2 / coef1 - each
    (float) of the float64 table entry (host only).  DcError for a timestep outside the schedule."""
    be = np.ascontiguousarray(betas, np.float64).reshape(-1)
    ts = np.ascontiguousarray(np.asarray(timesteps.cpu() if hasattr(timesteps, "cpu") else timesteps).reshape(-1), np.int32)
    out = np.zeros((max(ts.shape[0], 1), VB_COEF), np.float32)
    _check(lib().dc_vb_coefficients(be.shape[0], be.ctypes.data_as(C.POINTER(C.c_double)), _vb_type(VB_VAR, var_type, "var_type"),
                                    _iptr(ts), ts.shape[0], _fptr(out)))
    return out


def vb_terms(x_start, x_t, model_out, coef, mean_type, var_type, clip_denoised=True, var_values=None, noise=None):
    """dc_vb_terms on fp32 device tensors [B, T, ...]: per clip [B, VB_TERMS] - output (t == 0 ? decoder_nll : kl), kl, decoder_nll (bits),
    xstart_mse, mse ((eps - noise)^2; 0 without `noise`), 0, 0, 0 - from `coef` of vb_coefficients.  `var_values`: the variance half of a
    LEARNED / LEARNED_RANGE model's output."""
    import torch
    x = _loss_tensor(x_start, "x_start")
    B, T = int(x.shape[0]), int(x.shape[1])
    P = x.numel() // max(B * T, 1)
    xt, mo = _loss_tensor(x_t, "x_t", x.shape), _loss_tensor(model_out, "model_out", x.shape)
    vv = None if var_values is None else _loss_tensor(var_values, "var_values", x.shape)
    nz = None if noise is None else _loss_tensor(noise, "noise", x.shape)
    cf = np.ascontiguousarray(coef, np.float32)
    assert cf.shape == (B, VB_COEF), "one row of vb_coefficients per clip"
    L = lib()
    work = torch.empty((max(int(L.dc_vb_workspace_floats(B, T, P)), 1),), dtype=torch.float32, device=x.device)
    out = torch.empty((B, VB_TERMS), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(L.dc_vb_terms(x.data_ptr(), xt.data_ptr(), mo.data_ptr(), None if vv is None else vv.data_ptr(),
                             None if nz is None else nz.data_ptr(), _fptr(cf), _vb_type(VB_MEAN, mean_type, "mean_type"),
                             _vb_type(VB_VAR, var_type, "var_type"), int(bool(clip_denoised)), B, T, P, work.data_ptr(), out.data_ptr(),
                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def prior_kl(x_start, a, logvar):
    """dc_prior_kl: x_start fp32 [B, T, ...] on the device, host arrays a, logvar [B] -> the prior term of the bound per clip, bits, [B]."""
    import torch
    x = _loss_tensor(x_start, "x_start")
    B, T = int(x.shape[0]), int(x.shape[1])
    P = x.numel() // max(B * T, 1)
    a, lv = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(logvar, np.float32)
    assert a.shape == (B,) and lv.shape == (B,), "one (a, logvar) pair per clip"
    out = torch.empty((B,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib().dc_prior_kl(x.data_ptr(), _fptr(a), _fptr(lv), B, T, P, out.data_ptr(),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def m2sgan_fold_conv(weight_g, weight_v, conv_bias, bn_weight, bn_bias, bn_mean, bn_var):
    """dc_m2sgan_fold_conv: one weight-normed Conv1d (weight_g [cout, 1, 1], weight_v [cout, cin, k], bias) and the eval-mode BatchNorm
    behind it as the generator's finalize folds them -> (W fp32 [cout, k * cin], column tap * cin + ci; b fp32 [cout]).  Host only."""
    v = np.ascontiguousarray(weight_v, np.float32)
    cout, cin, k = v.shape
    vecs = [np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)) for a in (weight_g, conv_bias, bn_weight, bn_bias, bn_mean, bn_var)]
    assert all(a.shape == (cout,) for a in vecs), "one value per output channel"
    W, b = np.empty((cout, k * cin), np.float32), np.empty(cout, np.float32)
    _check(lib().dc_m2sgan_fold_conv(_fptr(vecs[0]), _fptr(v), *[_fptr(a) for a in vecs[1:]], cout, cin, k, _fptr(W), _fptr(b)))
    return W, b


def describe_status(st: int, precision: str) -> str:
    msg = []
    if st & STATUS_NONFINITE:
        msg.append(f"the denoiser produced a non-finite x0 in precision '{precision}' (fp16 operands overflow beyond +-65504): "
                   "use precision='mixed' (bf16-range operands) or precision='auto'")
    if st & STATUS_F16_SATURATED:
        msg.append("a FiLM modulation value left the fp16 range in which every precision mode stores it: this checkpoint is "
                   "outside what the library supports")
    if st & STATUS_TIMEOUT:
        msg.append("a workgroup of the small-batch layer kernel gave up waiting for its clip's combine slices (is the GPU shared with other "
                   "work?): the loop's results are invalid; DC_L16_OWN_COMBINE=1 selects the form without the in-launch exchange")
    return "; ".join(msg) or "ok"


def precise_tail_default(precision: str) -> int:
    """The number of split-operand evaluations at the end of a sampling loop a precision runs unless told otherwise (dc_ddim.h)."""
    return int(lib().dc_precise_tail_default(DC_PREC[precision])) if precision in DC_PREC else 0


def algorithmic_work(n_tokens: int) -> dict:
    """Algorithmic work per launch of the loop's two big kernels at `n_tokens` = B*T, the numerators of
    bench.py's roofline objects.  Both are priced against the MFMA roof, the path's primary bound:
    k_film_gemm is the [6144 x 512] x [512 x tokens] FiLM GEMM; k_layer (one decoder layer for all tokens) carries an eighth of
    the step's remaining algorithmic FLOPs.  `design_bytes`: what THIS decomposition moves through HBM per k_layer launch - per token
    the fp32 residual stream 512 B in + 512 B out, its 24 FiLM tiles x 64 B (written by the GEMM one launch earlier) and the
    workgroup records 72 B out + 36 B in - a property of the design, not SURVEY section 8d's compulsory bytes (2.3 MB per clip-step)."""
    # k_layer's FLOPs: the step's algorithmic 2 * 4 250 112 per token minus the FiLM GEMM's, over 8 layers
    return {"k_layer": {"bound": "mfma", "flops": (2 * 4250112 - 2 * 512 * 6144) // 8 * n_tokens,
                        "design_bytes": (512 + 512 + 24 * 64 + 72 + 36) * n_tokens},
            "k_film_gemm": {"bound": "mfma", "flops": 2 * 512 * 6144 * n_tokens}}


def pack_weight(w: np.ndarray, chained: bool):
    w = np.ascontiguousarray(w, np.float32)
    n_out, k_in = w.shape
    ne = ((n_out + 31) // 32) * ((k_in + 31) // 32) * 2 * 64 * 8
    hi, lo = np.empty(ne, np.uint16), np.empty(ne, np.uint16)
    u16 = C.POINTER(C.c_uint16)
    _check(lib().dc_pack_weight(_fptr(w), n_out, k_in, int(chained), hi.ctypes.data_as(u16), lo.ctypes.data_as(u16)))
    return hi, lo


def tile_row(r, hh):
    return (r & 3) + 8 * (r >> 2) + 4 * hh


def unpack_ft(raw):
    """[G][NT][64 lanes][16 regs] FT tiles -> row-major [32*G tokens][32*NT features]."""
    G, NT = raw.shape[0], raw.shape[1]
    out = np.empty((G, 32, NT, 32), raw.dtype)
    lane = np.arange(64)
    for r in range(16):
        feat = tile_row(r, lane >> 5)
        out[:, lane & 31, :, feat] = raw[:, :, lane, r].transpose(2, 0, 1)
    return out.reshape(G * 32, NT * 32)


# ---------------------------------------------------------------------------------------
# the sampler object
# ---------------------------------------------------------------------------------------
class NativeSampler:
    """Owns one dc_sampler.  Tensors are torch CUDA(ROCm) tensors; only their data_ptr()
    crosses the ABI."""

    def __init__(self, cfg, precision="fp16", max_timesteps=1000, device=0):
        self._h = C.c_void_p()
        c = DcConfig(cfg.input_feats, cfg.num_frames, cfg.latent_dim, cfg.ff_size, cfg.num_layers, cfg.num_heads,
                     int(bool(cfg.no_eff)), DC_PREC[precision], int(max_timesteps), int(device))
        _check(lib().dc_sampler_create(C.byref(c), C.byref(self._h)))
        self.cfg, self.precision, self.device, self.max_timesteps = cfg, precision, int(device), int(max_timesteps)
        self.B = self.T = 0
        self.guided = False
        self.takes = 1
        self.windows = None      # (W, T) while the conditioning holds the windows of longer pieces (set_conditioning_windows)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().dc_sampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, state_dict):
        """state_dict: name -> torch tensor / ndarray, with the reference's keys."""
        for k, v in state_dict.items():
            a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
            if a.dtype.kind != "f":
                continue   # BatchNorm.num_batches_tracked
            a = np.ascontiguousarray(a, np.float32)
            _check(lib().dc_sampler_set_param(self._h, k.encode(), _fptr(a), a.size))
        _check(lib().dc_sampler_finalize_params(self._h))

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def set_conditioning(self, xf_proj, xf_out, length=None, null=None, takes=1):
        """dc_sampler_set_conditioning, or - `null` = the pair (null_proj[64], null_out[64]) - dc_sampler_set_conditioning_guided: the
        loops then run with classifier-free guidance at the scale of set_guidance_scale (1 after this call); every tensor handed to
        them stays [B, T, P].
        `takes` > 1: dc_sampler_set_conditioning_takes - `takes` samples of each of the B musics.  The loops then run takes * B clips,
        take-major (clip j * B + b is take j of music b), and every tensor handed to them is [takes * B, T, P]; self.B is that count."""
        import torch
        assert xf_proj.is_cuda and xf_proj.dtype == torch.float32 and xf_proj.is_contiguous()
        assert xf_out.is_cuda and xf_out.dtype == torch.float32 and xf_out.is_contiguous()
        B, T, Cc = xf_proj.shape
        assert Cc == 64 and tuple(xf_out.shape) == (B, T, 64)
        lp = None
        if length is not None:
            la = np.ascontiguousarray(np.asarray(length.cpu() if hasattr(length, "cpu") else length), np.int32)
            assert la.shape == (B,)
            lp = _iptr(la)
        nv = [None, None]
        if null is not None:
            nv = [None if v is None else
                  np.ascontiguousarray(np.asarray(v.detach().cpu() if hasattr(v, "detach") else v), np.float32).reshape(-1) for v in null]
            assert len(nv) == 2 and all(v is None or v.shape == (64,) for v in nv), "null = (null_proj[64], null_out[64])"
        if int(takes) != 1:
            _check(lib().dc_sampler_set_conditioning_takes(self._h, xf_proj.data_ptr(), xf_out.data_ptr(), lp, B, T, int(takes),
                                                           *[None if v is None else _fptr(v) for v in nv], self._stream()))
        elif null is None:
            _check(lib().dc_sampler_set_conditioning(self._h, xf_proj.data_ptr(), xf_out.data_ptr(), lp, B, T, self._stream()))
        else:
            _check(lib().dc_sampler_set_conditioning_guided(self._h, xf_proj.data_ptr(), xf_out.data_ptr(), lp, B, T,
                                                            *[None if v is None else _fptr(v) for v in nv], self._stream()))
        self.takes = int(takes)
        self.B, self.T = B * self.takes, T
        self.guided = null is not None
        self.windows = None

    def set_conditioning_windows(self, xf_proj, xf_out, starts, weights, L, null=None):
        """dc_sampler_set_conditioning_windows: xf_proj, xf_out [W * B, T, 64], window-major (row k * B + b: window k of piece b),
        `starts` [W], `weights` fp32 [W, T] (harness.window_weights), pieces of L frames; `null`: the pair that makes the loops guided.
        Every tensor handed to the loops and to set_known is then [B, L, P]: self.B is the pieces, self.T is L.  A bad plan raises
        ValueError here, before the library is called (windows_check)."""
        import torch
        assert xf_proj.is_cuda and xf_proj.dtype == torch.float32 and xf_proj.is_contiguous()
        assert xf_out.is_cuda and xf_out.dtype == torch.float32 and xf_out.is_contiguous()
        st = np.ascontiguousarray(np.asarray(starts).reshape(-1), np.int32)
        W = int(st.shape[0])
        WB, T, Cc = xf_proj.shape
        if W < 1 or WB % W:
            raise ValueError(f"{WB} feature rows are not {W} windows of whole pieces")
        assert Cc == 64 and tuple(xf_out.shape) == (WB, T, 64)
        wt = np.ascontiguousarray(np.asarray(weights), np.float32)
        if wt.shape != (W, T):
            raise ValueError(f"weights must be {(W, T)}, got {wt.shape}")
        windows_check(st, wt, T, int(L))
        nv = [None, None]
        if null is not None:
            nv = [np.ascontiguousarray(np.asarray(v.detach().cpu() if hasattr(v, "detach") else v), np.float32).reshape(-1) for v in null]
            assert len(nv) == 2 and all(v.shape == (64,) for v in nv), "null = (null_proj[64], null_out[64])"
        _check(lib().dc_sampler_set_conditioning_windows(self._h, xf_proj.data_ptr(), xf_out.data_ptr(), None, _iptr(st), _fptr(wt), WB // W, W,
                                                         T, int(L), *[None if v is None else _fptr(v) for v in nv], self._stream()))
        self.takes, self.guided = 1, null is not None
        self.B, self.T = WB // W, int(L)
        self.windows = (W, T)

    def set_guidance_scale(self, w):
        """dc_sampler_set_guidance_scale: out = c + (w - 1)(c - u) in the loops of a guided conditioning; another scale replays the same
        graph.  Must be finite."""
        _check(lib().dc_sampler_set_guidance_scale(self._h, C.c_float(float(w))))

    def set_precise_tail(self, steps):
        """The loop's last `steps` model evaluations on split operands (fp16: golden DDIM-50 5.0e-4 -> 2.3e-4 / 1.6e-4 with 1 / 2 steps at
        +0.45 % of the loop each, default 1; bf16: see DESIGN.md section 5; -1: the precision's default).  DC_PRECISE_TAIL=k in the environment overrides it."""
        _check(lib().dc_sampler_set_precise_tail(self._h, int(steps)))

    def set_clip_aligned(self, mode):
        """Units of the wide launch form: True clip-aligned (batch-invariant results), False flat (throughput), None the library's rule -
        aligned whenever that costs no extra round of workgroups (dc_ddim.h, dc_sampler_set_clip_aligned)."""
        _check(lib().dc_sampler_set_clip_aligned(self._h, -1 if mode is None else (1 if mode else 0)))

    def set_idle_wave_path(self, on):
        """Padding waves of a clip's last workgroup in the wide plain layer kernel: True (default) barrier-only, False the whole layer
        as before - bit-identical results, the comparison form (dc_ddim.h, dc_sampler_set_idle_wave_path)."""
        _check(lib().dc_sampler_set_idle_wave_path(self._h, 1 if on else 0))

    def set_precise_forward(self, on):
        """denoise() on split operands (the precise tail's evaluation form; dc_ddim.h, dc_sampler_set_precise_forward)."""
        _check(lib().dc_sampler_set_precise_forward(self._h, 1 if on else 0))

    def set_combine_exchange(self, on):
        """Small batches: whether a clip's workgroups exchange their combine slices inside a layer launch (default) or every workgroup
        combines alone (no in-launch wait; dc_ddim.h, dc_sampler_set_combine_exchange).  dc_sampler_status latches `off` after a timeout."""
        _check(lib().dc_sampler_set_combine_exchange(self._h, 1 if on else 0))

    def set_encoder_format(self, fmt):
        """MusicEncoder activation format: "split" (two bf16 planes, 6e-6 at the encoder's output) or "f16" (one fp16 plane, 3.7e-4, half
        the time; the default beside an fp16 / bf16 denoiser).  DC_ME_PREC=f16|split in the environment overrides it per call."""
        _check(lib().dc_sampler_set_encoder_format(self._h, {"split": 0, "f16": 1, "fp16": 1}[fmt]))

    def encode_music(self, mel, out=None):
        """mel fp32 [B, Tm, 128] on the device -> (xf_proj, xf_out), each [B, (Tm-1)//3+1, 64] (`out`: the pair to fill, e.g.
        batch slices of larger tensors)."""
        import torch
        assert mel.is_cuda and mel.dtype == torch.float32 and mel.is_contiguous() and mel.dim() == 3
        B, Tm, nm = mel.shape
        T = (Tm - 1) // 3 + 1
        if out is None:
            xf_proj = torch.empty((B, T, 64), dtype=torch.float32, device=mel.device)
            xf_out = torch.empty_like(xf_proj)
        else:
            xf_proj, xf_out = out
            for t in out:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, T, 64)
        _check(lib().dc_sampler_encode_music(self._h, mel.data_ptr(), B, Tm, nm, xf_proj.data_ptr(), xf_out.data_ptr(),
                                             self._stream()))
        return xf_proj, xf_out

    def denoise(self, x, timesteps):
        import torch
        if self.windows is not None:
            raise ValueError("the conditioning holds the windows of longer pieces: a single evaluation has no piece to blend into")
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        assert tuple(x.shape) == (self.B, self.T, self.cfg.input_feats)
        ta = np.ascontiguousarray(np.asarray(timesteps.cpu() if hasattr(timesteps, "cpu") else timesteps), np.int32)
        assert ta.shape == (self.B,)
        out = torch.empty_like(x)
        _check(lib().dc_sampler_denoise(self._h, x.data_ptr(), _iptr(ta), out.data_ptr(), self._stream()))
        return out

    def ddim_loop(self, noise, coef, snap_iters=(), flags=0, step_noise=None, noise_seed=None):
        """coef [S, 4] (dc_sampler_ddim_loop: START_X, no clipping, eta = 0) or [S, 8] (dc_sampler_ddim_loop_ex with `flags` =
        UPDATE_* and, when any sigma != 0, either step_noise [S, B, T, P] on the device or noise_seed: the library then generates
        each iteration's draws at the head of its step, dc_sampler_set_step_noise_seed; a pair (seed, first_element) places this
        sampler's clips inside a larger batch's draw, dc_sampler_set_step_noise_seed_at).  A seed serves one loop."""
        import torch
        assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()
        assert tuple(noise.shape) == (self.B, self.T, self.cfg.input_feats)
        coef = np.ascontiguousarray(coef, np.float32)
        S = coef.shape[0]
        out = torch.empty_like(noise)
        si = np.ascontiguousarray(np.asarray(list(snap_iters), np.int32))
        snaps = torch.empty((len(si),) + tuple(noise.shape), dtype=torch.float32, device=noise.device) if len(si) else None
        sip, snp = (_iptr(si) if len(si) else None), (snaps.data_ptr() if snaps is not None else None)
        if coef.shape[1] == 4:
            assert flags == 0 and step_noise is None, "clip / epsilon / eta > 0 need the [S, 8] table of ddim_coefficients(.., eta)"
            _check(lib().dc_sampler_ddim_loop(self._h, noise.data_ptr(), out.data_ptr(), S, _fptr(coef), sip, len(si), snp, self._stream()))
        else:
            assert coef.shape[1] == 8
            zp = None
            if step_noise is not None:
                assert step_noise.is_cuda and step_noise.dtype == torch.float32 and step_noise.is_contiguous()
                assert tuple(step_noise.shape) == (S,) + tuple(noise.shape)
                zp = step_noise.data_ptr()
            elif noise_seed is not None:
                seed, first = noise_seed if isinstance(noise_seed, (tuple, list)) else (noise_seed, 0)
                _check(lib().dc_sampler_set_step_noise_seed_at(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(int(first))))
            _check(lib().dc_sampler_ddim_loop_ex(self._h, noise.data_ptr(), out.data_ptr(), S, _fptr(coef), int(flags), zp, sip,
                                                 len(si), snp, self._stream()))
        return out, snaps

    def solver_loop(self, noise, timesteps, rows, snap_iters=(), flags=0, step_noise=None, noise_seed=None):
        """dc_sampler_solver_loop: ddim_loop on the caller's `timesteps` [n] (strictly decreasing, < max_timesteps) and `rows`
        [n, SOLVER_ROW] of solver_table; step_noise is [n, B, T, P] and snap_iters count this loop's iterations."""
        import torch
        assert noise.is_cuda and noise.dtype == torch.float32 and noise.is_contiguous()
        assert tuple(noise.shape) == (self.B, self.T, self.cfg.input_feats)
        ts, rows, si, n = self._solver_args(timesteps, rows, snap_iters)
        out = torch.empty_like(noise)
        snaps = torch.empty((len(si),) + tuple(noise.shape), dtype=torch.float32, device=noise.device) if len(si) else None
        zp = None
        if step_noise is not None:
            assert step_noise.is_cuda and step_noise.dtype == torch.float32 and step_noise.is_contiguous()
            assert tuple(step_noise.shape) == (n,) + tuple(noise.shape)
            zp = step_noise.data_ptr()
        elif noise_seed is not None:
            seed, first = noise_seed if isinstance(noise_seed, (tuple, list)) else (noise_seed, 0)
            _check(lib().dc_sampler_set_step_noise_seed_at(self._h, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(int(first))))
        _check(lib().dc_sampler_solver_loop(self._h, noise.data_ptr(), out.data_ptr(), n, _iptr(ts), _fptr(rows), int(flags), zp,
                                            _iptr(si) if len(si) else None, len(si), snaps.data_ptr() if snaps is not None else None,
                                            self._stream()))
        return out, snaps

    @staticmethod
    def _solver_args(timesteps, rows, snap_iters=()):
        ts = np.ascontiguousarray(np.asarray(timesteps).reshape(-1), np.int32)
        rows = np.ascontiguousarray(rows, np.float32)
        assert rows.shape == (ts.shape[0], SOLVER_ROW), f"rows must be {(ts.shape[0], SOLVER_ROW)}: native.solver_table"
        return ts, rows, np.ascontiguousarray(np.asarray(list(snap_iters), np.int32)), int(ts.shape[0])

    def solver_profile_loop(self, noise, timesteps, rows, flags=0):
        """profile_loop for a loop over `timesteps` / `rows` (dc_sampler_solver_profile_loop)."""
        import torch
        ts, rows, _, n = self._solver_args(timesteps, rows)
        nk = lib().dc_kernel_count()
        ms, cnt = np.zeros(nk, np.float32), np.zeros(nk, np.int32)
        out = torch.empty_like(noise)
        _check(lib().dc_sampler_solver_profile_loop(self._h, noise.data_ptr(), out.data_ptr(), n, _iptr(ts), _fptr(rows), int(flags),
                                                    _fptr(ms), _iptr(cnt), nk, self._stream()))
        names = [lib().dc_kernel_name(i).decode() for i in range(nk)]
        return {names[i]: (float(ms[i]), int(cnt[i])) for i in range(nk)}, out

    def set_known(self, known=None, mask=None, noise=None):
        """dc_sampler_set_known: the following loops hold the elements whose `mask` is nonzero at sqrt(abar) known + sqrt(1 - abar) noise
        at every noise level (the final sample equals `known` there); fp32 device tensors [B, T, P] each, for the conditioning set
        last.  The loops then take the table of ddim_coefficients_known.  All None: cleared.  The sampler keeps the tensors alive."""
        import torch
        ts = (known, mask, noise)
        for t in ts:
            if t is not None:
                assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
                if tuple(t.shape) != (self.B, self.T, self.cfg.input_feats):
                    raise ValueError(f"known values must be {(self.B, self.T, self.cfg.input_feats)}, got {tuple(t.shape)}")
        _check(lib().dc_sampler_set_known(self._h, *[None if t is None else t.data_ptr() for t in ts]))
        self._known = ts if mask is not None else None

    def set_smoothing(self, window=19, order=5):
        """dc_sampler_set_smoothing: the loops write Savitzky-Golay-smoothed poses from now on (window 0: off)."""
        _check(lib().dc_sampler_set_smoothing(self._h, int(window), int(order)))

    def status(self, clear=True):
        """dc_sampler_status: waits for the sampler's work; OR of STATUS_NONFINITE / STATUS_F16_SATURATED."""
        v = C.c_int32(0)
        _check(lib().dc_sampler_status(self._h, C.byref(v), int(bool(clear))))
        return int(v.value)

    def profile_loop(self, noise, coef):
        import torch
        coef = np.ascontiguousarray(coef, np.float32)
        n = lib().dc_kernel_count()
        ms, cnt = np.zeros(n, np.float32), np.zeros(n, np.int32)
        out = torch.empty_like(noise)
        _check(lib().dc_sampler_profile_loop(self._h, noise.data_ptr(), out.data_ptr(), coef.shape[0], _fptr(coef),
                                             _fptr(ms), _iptr(cnt), n, self._stream()))
        names = [lib().dc_kernel_name(i).decode() for i in range(n)]
        return {names[i]: (float(ms[i]), int(cnt[i])) for i in range(n)}, out

    # ---- test hooks ---------------------------------------------------------------------
    def debug_denoise(self, x, timesteps, n_layers, stage):
        import torch
        ta = np.ascontiguousarray(np.asarray(timesteps), np.int32)
        out = torch.zeros_like(x)
        _check(lib().dc_sampler_debug_denoise(self._h, x.data_ptr(), _iptr(ta), out.data_ptr(), n_layers, stage,
                                              self._stream()))
        return out

    def debug_layer(self, h, timesteps, layer, first_stage, last_stage):
        """Blocks first_stage..last_stage (1 = SA, 2 = CA, 3 = FFN) of decoder layer `layer` alone on the residual stream
        h [B,T,128] (host array); returns h' [B,T,128]."""
        ha = np.ascontiguousarray(np.asarray(h, np.float32).reshape(self.B * self.T, 128))
        ta = np.ascontiguousarray(np.asarray(timesteps), np.int32)
        _check(lib().dc_sampler_debug_layer(self._h, _fptr(ha), _iptr(ta), int(layer), int(first_stage), int(last_stage),
                                            self._stream()))
        return self.read_h()[:self.B * self.T].reshape(self.B, self.T, 128)

    def debug_read(self, what, dtype, count):
        a = np.empty(count, dtype)
        _check(lib().dc_sampler_debug_read(self._h, what.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes))
        return a

    def clip_stride(self):
        """Frames per clip of the internal token space (T, padded to whole 32-frame groups where the clip-aligned kernels run)."""
        return int(lib().dc_sampler_clip_stride(self._h))

    def read_h(self):
        """Residual stream [>= B*T, 128] (rows b*T + n) unpacked from the FT-tile image [G][4][64][16]."""
        Tp = self.clip_stride()
        G = (self.B * Tp + 31) // 32
        # device order [G][tile][quarter][lane][4] -> [G][tile][lane][16 regs]
        raw = self.debug_read("h", np.float32, G * 4 * 64 * 16).reshape(G, 4, 4, 64, 4)
        rows = unpack_ft(raw.transpose(0, 1, 3, 2, 4).reshape(G, 4, 64, 16))
        if Tp != self.T:       # drop the padding frames of every clip
            rows = rows[:self.B * Tp].reshape(self.B, Tp, 128)[:, :self.T].reshape(self.B * self.T, 128)
        return rows

    def workspace_bytes(self):
        return int(lib().dc_sampler_workspace_bytes(self._h))


# ---------------------------------------------------------------------------------------
# the evaluation networks' handles
# ---------------------------------------------------------------------------------------
class _NativeHandle:
    """Owns one C handle of dc_ddim.h with PREFIX_create(device, &h) / _destroy / _set_param / _finalize.  Tensors are torch
    CUDA(ROCm) tensors; only their data_ptr() crosses the ABI."""
    _prefix = None

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _check(self._fn("create")(int(device), C.byref(self._h)))
        self.device = int(device)

    def _fn(self, name):
        return getattr(lib(), f"{self._prefix}_{name}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._fn("destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_param(self, name, a):
        a = np.ascontiguousarray(np.asarray(a), np.float32)
        _check(self._fn("set_param")(self._h, name.encode(), _fptr(a), a.size))

    def finalize(self):
        _check(self._fn("finalize")(self._h))

    @staticmethod
    def _ok(t, shape=None):
        import torch
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
        assert shape is None or tuple(t.shape) == tuple(shape), (tuple(t.shape), shape)

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------
# the motion encoder (M2SNet's ST-GCN, the evaluation metrics' latent space)
# ---------------------------------------------------------------------------------------
class NativeMotionEncoder(_NativeHandle):
    """Owns one dc_motion_encoder."""
    _prefix = "dc_motion_encoder"

    def encode(self, motion, out=None):
        """motion fp32 [B, T, 13, 2] (or [B, T, 26]) on the device -> latent fp32 [B, 64, T] (`out`: a tensor to fill)."""
        import torch
        assert motion.is_cuda and motion.dtype == torch.float32 and motion.is_contiguous()
        B, T = int(motion.shape[0]), int(motion.shape[1])
        assert motion.numel() == B * T * 26, tuple(motion.shape)
        if out is None:
            out = torch.empty((B, 64, T), dtype=torch.float32, device=motion.device)
        assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, 64, T)
        with torch.cuda.device(motion.device):
            _check(lib().dc_motion_encoder_encode(self._h, motion.data_ptr(), B, T, out.data_ptr(), self._stream()))
        return out


# ---------------------------------------------------------------------------------------
# M2SNet (the learned music-motion synchronisation score)
# ---------------------------------------------------------------------------------------
class NativeM2SNet(_NativeHandle):
    """Owns one dc_m2snet."""
    _prefix = "dc_m2snet"

    def encode_music(self, mel, out=None):
        """mel fp32 [B, Tm, 128] on the device -> music latent fp32 [B, (Tm-1)//3+1, 64] (`out`: a tensor to fill)."""
        import torch
        self._ok(mel)
        assert mel.dim() == 3 and mel.shape[2] == 128, tuple(mel.shape)
        B, Tm = int(mel.shape[0]), int(mel.shape[1])
        T = (Tm - 1) // 3 + 1
        if out is None:
            out = torch.empty((B, T, 64), dtype=torch.float32, device=mel.device)
        self._ok(out, (B, T, 64))
        with torch.cuda.device(mel.device):
            _check(lib().dc_m2snet_encode_music(self._h, mel.data_ptr(), B, Tm, out.data_ptr(), self._stream()))
        return out

    def fuse(self, music_latent, motion_latent, logits=False):
        """music latent [B, T, 64] and motion latent [B, 64, T] (fp32, on the device) -> probability [B, T], or the pair
        (probability, logit) with `logits`."""
        import torch
        self._ok(music_latent)
        B, T = int(music_latent.shape[0]), int(music_latent.shape[1])
        self._ok(music_latent, (B, T, 64))
        self._ok(motion_latent, (B, 64, T))
        prob = torch.empty((B, T), dtype=torch.float32, device=music_latent.device)
        logit = torch.empty_like(prob) if logits else None
        with torch.cuda.device(prob.device):
            _check(lib().dc_m2snet_fuse(self._h, music_latent.data_ptr(), motion_latent.data_ptr(), B, T, prob.data_ptr(),
                                        logit.data_ptr() if logits else None, self._stream()))
        return (prob, logit) if logits else prob

    @staticmethod
    def pairs_share():
        """The number of motions one wave of `fuse_pairs` walks per launch."""
        return int(lib().dc_m2snet_pairs_share())

    def fuse_pairs(self, music_latent, motion_latent, len_music=None, len_motion=None, frames=False):
        """Every music [Bm, T, 64] against every motion [Bn, 64, T] (fp32, on the device) -> (sum fp32 [Bm, Bn], above int32 [Bm, Bn],
        below int32 [Bm, Bn], prob fp32 [Bm, Bn, T] | None) over the frames t < min(len_music[i], len_motion[j]) (int arrays on the
        host, None = T)."""
        import torch
        self._ok(music_latent)
        self._ok(motion_latent)
        assert music_latent.dim() == 3 and motion_latent.dim() == 3, (tuple(music_latent.shape), tuple(motion_latent.shape))
        Bm, T, Bn = int(music_latent.shape[0]), int(music_latent.shape[1]), int(motion_latent.shape[0])
        self._ok(music_latent, (Bm, T, 64))
        self._ok(motion_latent, (Bn, 64, T))
        lens = []
        for a, n, what in ((len_music, Bm, "len_music"), (len_motion, Bn, "len_motion")):
            if a is not None:
                a = np.ascontiguousarray(np.asarray(a).astype(np.int32, casting="same_kind"))
                if a.shape != (n,):
                    raise ValueError(f"{what} must have shape ({n},), got {a.shape}")
            lens.append(a)
        dev = music_latent.device
        total = torch.empty((Bm, Bn), dtype=torch.float32, device=dev)
        above = torch.empty((Bm, Bn), dtype=torch.int32, device=dev)
        below = torch.empty((Bm, Bn), dtype=torch.int32, device=dev)
        prob = torch.empty((Bm, Bn, T), dtype=torch.float32, device=dev) if frames else None
        with torch.cuda.device(dev):
            _check(lib().dc_m2snet_fuse_pairs(self._h, music_latent.data_ptr(), motion_latent.data_ptr(), Bm, Bn, T,
                                              None if lens[0] is None else _iptr(lens[0]), None if lens[1] is None else _iptr(lens[1]),
                                              total.data_ptr(), above.data_ptr(), below.data_ptr(), prob.data_ptr() if frames else None,
                                              self._stream()))
        return total, above, below, prob

    def score(self, mel, motion, logits=False):
        """mel [B, Tm, 128] and motion [B, T, 13, 2] (or [B, T, 26]) -> probability [B, T] (or (probability, logit))."""
        import torch
        self._ok(mel)
        self._ok(motion)
        assert mel.dim() == 3 and mel.shape[2] == 128, tuple(mel.shape)
        B, Tm, T = int(mel.shape[0]), int(mel.shape[1]), int(motion.shape[1])
        assert motion.shape[0] == B and motion.numel() == B * T * 26, (tuple(mel.shape), tuple(motion.shape))
        prob = torch.empty((B, T), dtype=torch.float32, device=mel.device)
        logit = torch.empty_like(prob) if logits else None
        with torch.cuda.device(prob.device):
            _check(lib().dc_m2snet_score(self._h, mel.data_ptr(), motion.data_ptr(), B, Tm, T, prob.data_ptr(),
                                         logit.data_ptr() if logits else None, self._stream()))
        return (prob, logit) if logits else prob


# ---------------------------------------------------------------------------------------
# the M2S-GAN generator (the baseline of the evaluation table)
# ---------------------------------------------------------------------------------------
class NativeM2SGAN(_NativeHandle):
    """Owns one dc_m2sgan.  Shapes the library refuses (T <= 128, T != 30 Ln, T != (Tm-1)//3+1) raise ValueError before the call.
    `decoder`: "tcn" (the reference's default), or "none" for a features-only generator whose poses come from a NativeBiLSTM."""
    _prefix = "dc_m2sgan"
    DECODERS = {"tcn": 0, "none": 1}      # DC_M2SGAN_DECODER_*

    def __init__(self, device=0, decoder="tcn"):
        if decoder not in self.DECODERS:
            raise ValueError(f"decoder must be one of {sorted(self.DECODERS)}, got {decoder!r}")
        super().__init__(device)
        self.decoder = decoder
        if decoder != "tcn":
            _check(lib().dc_m2sgan_set_decoder(self._h, self.DECODERS[decoder]))

    @staticmethod
    def check_frames(T, Tm=None, Ln=None, decoder="tcn"):
        """The library's shape rules (dc_ddim.h) as ValueErrors."""
        if Tm is not None and (Tm < 4 or T != (Tm - 1) // 3 + 1):
            raise ValueError(f"{Tm} mel frames make {(Tm - 1) // 3 + 1 if Tm >= 4 else 0} frames, not {T} (and at least 4 are needed)")
        if Ln is not None and T != 30 * Ln:
            raise ValueError(f"a latent of {Ln} steps makes {30 * Ln} frames, the music has {T}")
        if T <= 128 and decoder == "tcn":
            raise ValueError(f"{T} frames: the generator's last temporal block reflects 128 frames and needs T > 128 (T >= 150)")

    def _inputs(self, mel, noise):
        self._ok(mel)
        self._ok(noise)
        assert mel.dim() == 3 and mel.shape[2] == 128, tuple(mel.shape)
        B, Tm, Ln = int(mel.shape[0]), int(mel.shape[1]), int(noise.shape[1])
        self._ok(noise, (B, Ln, 8))
        T = (Tm - 1) // 3 + 1 if Tm >= 4 else 0
        self.check_frames(T, Tm, Ln, self.decoder)
        return B, Tm, Ln, T

    def features(self, mel, noise):
        """mel fp32 [B, Tm, 128], noise fp32 [B, Ln, 8] on the device -> Generator.features fp32 [B, T, 128]."""
        import torch
        B, Tm, Ln, T = self._inputs(mel, noise)
        out = torch.empty((B, T, 128), dtype=torch.float32, device=mel.device)
        with torch.cuda.device(mel.device):
            _check(lib().dc_m2sgan_features(self._h, mel.data_ptr(), B, Tm, noise.data_ptr(), Ln, out.data_ptr(), self._stream()))
        return out

    def generate(self, mel, noise):
        """mel fp32 [B, Tm, 128], noise fp32 [B, Ln, 8] on the device -> poses fp32 [B, T, 26]."""
        import torch
        if self.decoder != "tcn":
            raise ValueError("this generator was built without a decoder (decoder='none'): it computes features only")
        B, Tm, Ln, T = self._inputs(mel, noise)
        out = torch.empty((B, T, 26), dtype=torch.float32, device=mel.device)
        with torch.cuda.device(mel.device):
            _check(lib().dc_m2sgan_generate(self._h, mel.data_ptr(), B, Tm, noise.data_ptr(), Ln, out.data_ptr(), self._stream()))
        return out

    def decode(self, feat, n_blocks=None):
        """features fp32 [B, T, 128] on the device -> poses fp32 [B, T, 26]; `n_blocks` in 1 .. 6 (test hook): the residual stream
        [B, T, 64] after that many temporal blocks instead."""
        import torch
        self._ok(feat)
        assert feat.dim() == 3 and feat.shape[2] == 128, tuple(feat.shape)
        B, T = int(feat.shape[0]), int(feat.shape[1])
        if self.decoder != "tcn":
            raise ValueError("this generator was built without a decoder (decoder='none'): it computes features only")
        self.check_frames(T)
        out = torch.empty((B, T, 26 if n_blocks is None else 64), dtype=torch.float32, device=feat.device)
        with torch.cuda.device(feat.device):
            if n_blocks is None:
                _check(lib().dc_m2sgan_decode(self._h, feat.data_ptr(), B, T, out.data_ptr(), self._stream()))
            else:
                _check(lib().dc_m2sgan_debug_blocks(self._h, feat.data_ptr(), B, T, int(n_blocks), out.data_ptr(), self._stream()))
        return out


# ---------------------------------------------------------------------------------------
# the BiLSTM pose decoder (the CNN-LSTM baselines of the evaluation table)
# ---------------------------------------------------------------------------------------
def bilstm_pass_clips(B, T):
    """dc_bilstm_pass_clips: clips per pass of the BiLSTM decoder, min(B, 128, 2^28 // (1536 T)) and at least 1."""
    return int(lib().dc_bilstm_pass_clips(int(B), int(T)))


class NativeBiLSTM(_NativeHandle):
    """Owns one dc_bilstm."""
    _prefix = "dc_bilstm"

    @property
    def input_size(self):
        return int(lib().dc_bilstm_input_size(self._h))

    def _run(self, feat, layers):
        import torch
        self._ok(feat)
        assert feat.dim() == 3, tuple(feat.shape)
        B, T, In = (int(n) for n in feat.shape)
        if In != self.input_size:
            raise ValueError(f"features of {In} values per frame, the decoder was loaded for {self.input_size}")
        out = torch.empty((B, T, 26 if layers is None else 256), dtype=torch.float32, device=feat.device)
        with torch.cuda.device(feat.device):
            if layers is None:
                _check(lib().dc_bilstm_decode(self._h, feat.data_ptr(), B, T, out.data_ptr(), self._stream()))
            else:
                _check(lib().dc_bilstm_hidden(self._h, feat.data_ptr(), B, T, int(layers), out.data_ptr(), self._stream()))
        return out

    def decode(self, feat):
        """features fp32 [B, T, In] on the device -> poses fp32 [B, T, 26]."""
        return self._run(feat, None)

    def hidden(self, feat, layers=2):
        """Test hook: the LSTM's output fp32 [B, T, 256] after `layers` (1 or 2) layers."""
        return self._run(feat, layers)


# ---------------------------------------------------------------------------------------
# realism and rhythm: the Welch spectrum, the speed contour, the standard deviation; the M2S-GAN critic
# ---------------------------------------------------------------------------------------
def _motion26(handle, motion):
    """(B, T) of a motion tensor fp32 [B, T, 26] (or [B, T, 13, 2]) on the device."""
    handle._ok(motion)
    B, T = int(motion.shape[0]), int(motion.shape[1])
    assert motion.dim() in (3, 4) and motion.numel() == B * T * 26, tuple(motion.shape)
    return B, T


class NativeRhythm(_NativeHandle):
    """Owns one dc_rhythm (no parameters: the handle is ready after create).  Shapes the library refuses raise ValueError before
    the call."""
    _prefix = "dc_rhythm"
    PSD_BINS, MIN_PSD_T, MIN_CONTOUR_T, MAX_ORDER = 32, 256, 60, 64

    @staticmethod
    def windows(T):
        """W of the contour: AvgPool1d(60, 30) over T frames."""
        return (T - 60) // 30 + 1

    def psd(self, motion):
        """motion fp32 [B, T, 26] on the device -> bins 0 .. 31 of the channel-averaged Welch PSD, fp32 [B, 32]."""
        import torch
        B, T = _motion26(self, motion)
        if T < self.MIN_PSD_T:
            raise ValueError(f"{T} frames: Welch's 256-frame segment needs T >= 256")
        out = torch.empty((B, self.PSD_BINS), dtype=torch.float32, device=motion.device)
        with torch.cuda.device(motion.device):
            _check(lib().dc_rhythm_psd(self._h, motion.data_ptr(), B, T, out.data_ptr(), self._stream()))
        return out

    def contour(self, motion, contour=True, sd=True):
        """motion fp32 [B, T, 26] on the device -> (speed contour fp32 [B, W] | None, standard deviation fp32 [B] | None)."""
        import torch
        B, T = _motion26(self, motion)
        if T < self.MIN_CONTOUR_T:
            raise ValueError(f"{T} frames: the contour's 60-frame window needs T >= 60")
        c = torch.empty((B, self.windows(T)), dtype=torch.float32, device=motion.device) if contour else None
        s = torch.empty((B,), dtype=torch.float32, device=motion.device) if sd else None
        with torch.cuda.device(motion.device):
            _check(lib().dc_rhythm_contour(self._h, motion.data_ptr(), B, T, c.data_ptr() if contour else None,
                                           s.data_ptr() if sd else None, self._stream()))
        return c, s

    def motion_beats(self, motion, length=None, order=10, envelope=False):
        """motion fp32 [B, T, 26] on the device, `length` None or B host ints -> (beats uint8 [B, T], envelope fp32 [B, T] | None):
        dc_rhythm_motion_beats, the strict minima over +-`order` frames of the summed joint speed."""
        import torch
        B, T = _motion26(self, motion)
        if not 1 <= int(order) <= self.MAX_ORDER:
            raise ValueError(f"order {order} is outside 1 .. {self.MAX_ORDER}")
        lp = None
        if length is not None:
            ln = np.ascontiguousarray(np.asarray(length).reshape(-1), np.int32)
            if ln.shape != (B,) or ln.min() < 1 or ln.max() > T:
                raise ValueError(f"length must hold {B} values in [1, {T}], got {ln.tolist()}")
            lp = _iptr(ln)
        beats = torch.empty((B, T), dtype=torch.uint8, device=motion.device)
        env = torch.empty((B, T), dtype=torch.float32, device=motion.device) if envelope else None
        with torch.cuda.device(motion.device):
            _check(lib().dc_rhythm_motion_beats(self._h, motion.data_ptr(), lp, B, T, int(order), env.data_ptr() if envelope else None,
                                                beats.data_ptr(), self._stream()))
        return beats, env

    def beat_scores(self, motion_beats, music_beats, music_stride=1, sigma=3.0):
        """one-hots uint8 [B, T] and [B, Lm] on the device (nonzero = a beat) -> (scores fp32 [B, 2]: BC and Beat Align, counts int32
        [B, 2]: music beats and motion beats): dc_rhythm_beat_scores."""
        import torch
        for t in (motion_beats, music_beats):
            assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == 2, (t.dtype, tuple(t.shape))
        B, T, Lm = int(motion_beats.shape[0]), int(motion_beats.shape[1]), int(music_beats.shape[1])
        if int(music_beats.shape[0]) != B or B < 1 or T < 1 or Lm < 1:
            raise ValueError(f"motion beats {tuple(motion_beats.shape)} and music beats {tuple(music_beats.shape)}: one non-empty row per clip each")
        if int(music_stride) < 1 or not (np.isfinite(sigma) and sigma > 0):
            raise ValueError(f"music_stride {music_stride} must be >= 1 and sigma {sigma} finite and > 0")
        scores = torch.empty((B, 2), dtype=torch.float32, device=motion_beats.device)
        counts = torch.empty((B, 2), dtype=torch.int32, device=motion_beats.device)
        with torch.cuda.device(motion_beats.device):
            _check(lib().dc_rhythm_beat_scores(self._h, motion_beats.data_ptr(), B, T, music_beats.data_ptr(), Lm, int(music_stride),
                                               C.c_float(float(sigma)), scores.data_ptr(), counts.data_ptr(), self._stream()))
        return scores, counts


class NativeDiscriminator(_NativeHandle):
    """Owns one dc_discriminator.  T < 41 (no pooled frame behind the third stage) raises ValueError before the call."""
    _prefix = "dc_discriminator"
    MIN_T = 41

    @staticmethod
    def pooled_frames(T):
        """(L1, L2, L3) behind the three Conv1d + MaxPool1d(5, stride 3 / 2 / 2) stages."""
        L1 = (T - 5) // 3 + 1
        L2 = (L1 - 5) // 2 + 1
        return L1, L2, (L2 - 5) // 2 + 1

    def _frames(self, motion):
        B, T = _motion26(self, motion)
        if T < self.MIN_T:
            raise ValueError(f"{T} frames leave no pooled frame behind the critic's third stage (T >= 41)")
        return B, T

    def features(self, motion):
        """motion fp32 [B, T, 26] on the device -> Discriminator_1DCNN.features' tensor fp32 [B, 64, L3]."""
        import torch
        B, T = self._frames(motion)
        out = torch.empty((B, 64, self.pooled_frames(T)[2]), dtype=torch.float32, device=motion.device)
        with torch.cuda.device(motion.device):
            _check(lib().dc_discriminator_features(self._h, motion.data_ptr(), B, T, out.data_ptr(), self._stream()))
        return out

    def score(self, motion):
        """motion fp32 [B, T, 26] on the device -> D(x) fp32 [B]."""
        import torch
        B, T = self._frames(motion)
        out = torch.empty((B,), dtype=torch.float32, device=motion.device)
        with torch.cuda.device(motion.device):
            _check(lib().dc_discriminator_score(self._h, motion.data_ptr(), B, T, out.data_ptr(), self._stream()))
        return out


# ---------------------------------------------------------------------------------------
# the mel spectrogram of a waveform (extract_mel_feature)
# ---------------------------------------------------------------------------------------
MEL_FFT, MEL_HOP, MEL_BANDS, MEL_BINS = 2048, 256, 128, 1025
MEL_PAD = {"constant": 0, "reflect": 1}             # DC_MEL_PAD_*


def mel_tables(sr=22050):
    """dc_mel_tables (host only): what a dc_mel of `sr` uploads - {"window" fp32 [2048], "twiddle" fp32 [2048, 2], "first" / "count"
    int32 [128], "weights" fp32 [sum(count)]}: filter m covers bins first[m] .. first[m] + count[m] - 1 with the next count[m] weights."""
    win, tw = np.empty(MEL_FFT, np.float32), np.empty((MEL_FFT, 2), np.float32)
    first, count, total = np.empty(MEL_BANDS, np.int32), np.empty(MEL_BANDS, np.int32), np.zeros(1, np.int32)
    _check(lib().dc_mel_tables(int(sr), _fptr(win), _fptr(tw), _iptr(first), _iptr(count), None, 0, _iptr(total)))
    wts = np.empty(int(total[0]), np.float32)
    _check(lib().dc_mel_tables(int(sr), None, None, None, None, _fptr(wts), wts.size, None))
    return {"window": win, "twiddle": tw, "first": first, "count": count, "weights": wts}


def mel_out_frames(n, sr=22050):
    """dc_mel_out_frames (host only): the reference's int(n / sr * 90)."""
    return int(lib().dc_mel_out_frames(int(n), int(sr)))


def mel_pass_clips(N):
    """dc_mel_pass_clips (host only): clips per pass of NativeMel.features at N samples."""
    return int(lib().dc_mel_pass_clips(int(N)))


class NativeMel(_NativeHandle):
    """Owns one dc_mel (no parameters: ready after create).  Shapes the library refuses raise ValueError before the call."""
    _prefix = "dc_mel"

    def __init__(self, device=0, sr=22050, pad_mode="constant"):
        if pad_mode not in MEL_PAD:
            raise ValueError(f"pad_mode must be one of {sorted(MEL_PAD)}, got {pad_mode!r}")
        if int(sr) < 1:
            raise ValueError(f"sr must be >= 1, got {sr}")
        self._h = C.c_void_p()
        _check(lib().dc_mel_create(int(device), int(sr), MEL_PAD[pad_mode], C.byref(self._h)))
        self.device, self.sr, self.pad_mode = int(device), int(sr), pad_mode

    def _wave(self, wave, lengths):
        self._ok(wave)
        assert wave.dim() == 2, tuple(wave.shape)
        B, N = int(wave.shape[0]), int(wave.shape[1])
        if B < 1 or N < MEL_FFT:
            raise ValueError(f"waveforms {tuple(wave.shape)}: at least one clip of at least {MEL_FFT} samples")
        ln = None
        if lengths is not None:
            ln = np.ascontiguousarray(np.asarray(lengths).reshape(-1), np.int32)
            if ln.shape != (B,) or ln.min() < MEL_FFT or ln.max() > N:
                raise ValueError(f"lengths must hold {B} values in [{MEL_FFT}, {N}], got {ln.tolist()}")
        return B, N, ln

    def power(self, wave, lengths=None):
        """wave fp32 [B, N] on the device, `lengths` None or B host ints -> the mel power fp32 [B, 1 + N // 256, 128]: dc_mel_power."""
        import torch
        B, N, ln = self._wave(wave, lengths)
        out = torch.empty((B, 1 + N // MEL_HOP, MEL_BANDS), dtype=torch.float32, device=wave.device)
        with torch.cuda.device(wave.device):
            _check(lib().dc_mel_power(self._h, wave.data_ptr(), None if ln is None else _iptr(ln), B, N, out.data_ptr(), self._stream()))
        return out

    def features(self, wave, lengths=None, out_frames=None):
        """wave fp32 [B, N] on the device, `lengths` and `out_frames` None or B host ints -> fp32 [B, Tm, 128], Tm the largest output
        length (default per clip: mel_out_frames of its length): dc_mel_features."""
        import torch
        B, N, ln = self._wave(wave, lengths)
        if out_frames is None:
            tm = np.array([mel_out_frames(n, self.sr) for n in (ln if ln is not None else [N] * B)], np.int32)
        else:
            tm = np.ascontiguousarray(np.asarray(out_frames).reshape(-1), np.int32)
        if tm.shape != (B,) or tm.min() < 1:
            raise ValueError(f"out_frames must hold {B} values >= 1, got {tm.tolist()}")
        Tm = int(tm.max())
        out = torch.empty((B, Tm, MEL_BANDS), dtype=torch.float32, device=wave.device)
        with torch.cuda.device(wave.device):
            _check(lib().dc_mel_features(self._h, wave.data_ptr(), None if ln is None else _iptr(ln), B, N, _iptr(tm), Tm, out.data_ptr(),
                                         self._stream()))
        return out
