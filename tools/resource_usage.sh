#!/bin/bash
# Register and scratch use of every kernel, from the compiler's own remarks (-Rpass-analysis=kernel-resource-usage) on the
# kernel files that carry the sweep step, the input gradients, the core gradients, the optimiser step, the orthogonal form, the scaled prediction, the MPS algebra, the two samplers, the likelihood gradients, the per-pixel conditionals, the pair marginals and the likelihood sweep: one line per kernel.  Device pass only, nothing is linked or written.
# Usage: tools/resource_usage.sh [substring of file:kernel ...]     (no argument: every kernel)
set -e -o pipefail
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
ARCH=${ARCH:-gfx950}
cd "$(dirname "$0")/../tensornetworkforml_amd/csrc"
printf '%-44s %6s %6s %6s %11s %11s %9s %6s\n' kernel SGPRs VGPRs AGPRs SGPR-spill VGPR-spill scratch-B LDS-B
for f in kernels_narrow kernels_wide kernels_big kernels_anyd kernels_inputgrad kernels_coregrad kernels_optim kernels_orth kernels_scaled kernels_algebra kernels_sample kernels_sample_masked kernels_nll kernels_site_cond kernels_pair kernels_nll_sweep kernels_nll_masked; do
  $HIPCC -O3 -std=c++17 -fPIC --offload-arch=$ARCH -I/opt/rocm/include --cuda-device-only -Rpass-analysis=kernel-resource-usage \
      -c $f.hip -o /dev/null 2>&1 | ${CXXFILT:-c++filt} |
  awk -v file=$f -v want="$*" '
    function val(s) { sub(/ \[-Rpass.*/, "", s); sub(/.*: /, "", s); return s }
    /Function Name:/            { name = val($0); sub(/ \[-Rpass.*/, "", name); gsub(/\(anonymous namespace\)::/, "", name); sub(/\(.*/, "", name); sub(/^void /, "", name); gsub(/tnml::/, "", name) }
    /TotalSGPRs:/               { sg = val($0) }
    / VGPRs:/ && !/Spill/       { vg = val($0) }
    / AGPRs:/                   { ag = val($0) }
    /SGPRs Spill:/              { ss = val($0) }
    /VGPRs Spill:/              { vs = val($0) }
    /ScratchSize \[bytes\/lane\]:/ { sc = val($0) }
    /LDS Size \[bytes\/block\]:/ {
      lds = val($0); show = (want == "")
      n = split(want, w, " "); for (i = 1; i <= n; ++i) if (index(file ":" name, w[i])) show = 1
      if (show) printf "%-44s %6s %6s %6s %11s %11s %9s %6s\n", file ":" name, sg, vg, ag, ss, vs, sc, lds
    }'
done
