// dc_music.h - internal interface of the MusicEncoder / encode_music kernels (dc_music.hip).
// Reference: Diffusion_Stage/models/transformer.py:289-340 (Conv2dResLayer, MusicEncoder), :447-459 (encode_music).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "dc_pack.h"   // DcParams; music_pack: the encoder's folding and packing, host only

struct dc_music;   // device-resident folded weights + ping-pong activation planes

// names/sizes of the reference state_dict entries the encoder consumes (`music_encoder.*`, `proj.*`).  with_proj = false here and
// below: an encoder of the `music_encoder.*` entries alone (Contrastive_Stage/models/MusicEncoder.py:30-53, the same layers without
// the denoiser's proj), whose dc_music_encode takes d_xf_proj = nullptr
std::vector<std::pair<std::string, size_t>> dc_music_required(int music_dim, bool with_proj = true);
// false, with *err set, when one of them is missing or has the wrong size
bool dc_music_check(const DcParams& params, int music_dim, std::string* err, bool with_proj = true);
// Builds the encoder on the current device: dc_music_check, music_pack (BatchNorm in eval mode, running statistics, is folded
// into the convolution in front of it), upload.  Returns nullptr and sets *err on failure.
dc_music* dc_music_build(const DcParams& params, int music_dim, std::string* err, bool with_proj = true);
void dc_music_destroy(dc_music* m);

// mel [B][Tm][128] fp32 (device) -> xf_out [B][T][64], xf_proj [B][T][64] fp32 (device), T = (Tm - 1) / 3 + 1.
// Work is enqueued on `st`; clips are processed in chunks so the activation planes stay bounded.  d_xf_proj == nullptr: xf_out
// alone (the proj kernel is not launched); an encoder built without proj accepts nothing else (hipErrorInvalidValue).
hipError_t dc_music_encode(dc_music* m, const float* d_mel, int B, int Tm, float* d_xf_proj, float* d_xf_out, hipStream_t st,
                           std::string* err);
// plane format of this encoder's activations: 0 = two bf16 planes (hi + lo, three MFMAs per product: ~6e-6 at the output), 1 = one
// fp16 plane (one MFMA per product, half the bytes: ~4e-4 at the output, 1.3e-4 of x0 after DDIM-50).  DC_ME_PREC=f16|split overrides.
void dc_music_set_format(dc_music* m, int single_fp16);
// ... for good: DC_ME_PREC no longer applies to this encoder (a metric's encoder must not change with the sampler's switch)
void dc_music_pin_format(dc_music* m, int single_fp16);
int dc_music_format(const dc_music* m);
int dc_music_frames(int Tm);
long long dc_music_workspace_bytes(const dc_music* m);
