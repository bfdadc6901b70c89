#!/bin/bash
# Build libdc_ddim.so for gfx950 (native.build_library, every object compiled again) and print register/spill usage of the kernels
# matching $1 (default: k_layer).
set -e
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R"
PAT="${1:-k_layerIDF16_Lb0ELb0ELb0ELb1ELb0}"
python -c "import diffusion_conductor_amd; from diffusion_conductor_amd import native; native.build_library(force=True, extra_flags=['-Rpass-analysis=kernel-resource-usage'])" 2>&1 \
  | grep -E "error|Function Name|VGPRs:|AGPRs:|ScratchSize|VGPRs Spill|Occupancy" \
  | grep -A5 -E "error|Name: _Z[0-9]+($PAT)" | grep -E "error|Name|VGPRs:|AGPRs|Scratch|VGPRs Spill" | sed 's/.*remark: *//' | cut -c1-100
