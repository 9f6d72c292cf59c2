#!/bin/bash
export TRK_LAB=1   # tools are lab runs: lab knobs are honoured (trtools_amd/_knobs.py)
# Kernels of libtrk.so that use scratch memory, per translation unit, from the compiler's own resource remarks
# (`-Rpass-analysis=kernel-resource-usage`): name, VGPRs, scratch bytes per lane.  Run from anywhere; no GPU needed.
# The multi-outcome regression and every form of the Gram correction are listed whether they spill or not (their
# register counts are quoted in profiles/assoc_multi_probe_notes.md), and so is the logistic Newton kernel (k_assoc_logit).
cd "$(dirname "$0")/../trtools_amd/csrc" || exit 1
for f in trk_kernels trk_hwe trk_assoc trk_assoc_logit trk_qc trk_compare trk_mosaic trk_parse trk_reads trk_api; do
    [ -f $f.hip ] || continue
    extra=""; [ $f = trk_hwe ] && extra="-mllvm -disable-machine-licm"
    [ $f = trk_compare ] && extra="-Xclang -target-feature -Xclang -packed-fp32-ops"
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off $extra --cuda-device-only -c $f.hip -o /dev/null \
        -Rpass-analysis=kernel-resource-usage 2>&1 | grep -E "Function Name|  VGPRs:|ScratchSize" |
        sed 's/.*remark: *//; s/ \[-Rpass.*//' | paste - - - |
        awk -v f=$f '{n++} $NF>0 || /k_assoc_regress_multi|k_assoc_gram_miss|k_assoc_logit/{print f".hip\t"$3"\tVGPRs "$5"\tscratch "$NF} END{print f".hip: "n" kernels"}'
done | c++filt | cut -c1-170
