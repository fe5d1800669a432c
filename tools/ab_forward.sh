#!/bin/bash
# dev tool: bf16 forward time of several library variants (tools/build_variant.sh), both cfg4 shapes
R=$(cd "$(dirname "$0")/.." && pwd)
for v in "$@"; do
  lib=$R/shallow_wavenet_amd/libswn_hip_$v.so; [ "$v" = main ] && lib=$R/shallow_wavenet_amd/libswn_hip.so
  for shape in "8 150" "64 150"; do
    echo -n "$v $shape: "; SWN_HIP_LIB=$lib python3 $R/tools/time_forward.py $shape 2>&1 | grep "^bf16:"
  done
done
