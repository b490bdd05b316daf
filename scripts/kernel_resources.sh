#!/bin/bash
# Per-kernel registers / scratch / occupancy / LDS of one kernel unit (a device-only compile
# with the kernel-resource-usage remarks):
#   bash scripts/kernel_resources.sh [unit.hip (default td_step.hip)] [extra hipcc flags]
cd "$(dirname "$0")/../gym-td_amd/csrc"
unit=td_step.hip
case "$1" in *.hip) unit=$1; shift ;; esac
obj=$(mktemp /tmp/tdres_XXXXXX.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -w --cuda-device-only "$@" \
  -c "$unit" -o "$obj" -Rpass-analysis=kernel-resource-usage 2>&1 |
  grep -E "Function Name|SGPRs:|VGPRs:|ScratchSize|Occupancy|LDS Size" | paste - - - - - - |
  sed -E 's/[A-Za-z0-9_.\/]+\.(hip|inc|h):[0-9]*:[0-9]*: remark: //g; s/ \[-Rpass-analysis=kernel-resource-usage\]//g; s/Function Name: _ZN2td[0-9]+//; s/EEEvNS_8StepArgsE//; s/ScratchSize \[bytes\/lane\]/scratch/; s/Occupancy \[waves\/SIMD\]/occ/; s/LDS Size \[bytes\/block\]/lds/; s/TotalSGPRs/sgpr/; s/VGPRs/vgpr/' |
  awk '{$1=$1};1'
rm -f "$obj"
