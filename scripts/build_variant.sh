#!/bin/bash
# Build a variant of libnmf_hip.so with extra -D flags for kernel A/B experiments (loaded with NMF_HIP_LIB=<path>).
# usage: scripts/build_variant.sh <name> [-DFLAG ...]   -> build/libnmf_<name>.so
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
mkdir -p "$ROOT/build"
# (the flags are flygym_amd/_native.py::compile_command's; the -D options go in front of the include paths)
cd "$ROOT"
python -c 'import subprocess, sys; from flygym_amd import _native; subprocess.run(_native.compile_command(sys.argv[1], sys.argv[2:]))' \
  "$ROOT/build/libnmf_$NAME.so" "$@" 2>&1 | grep -v "occupancy target\|nmf_step_kernel(const\|\^\|warnings generated" || true
python "$ROOT/scripts/kernel_stats.py" "$ROOT/build/libnmf_$NAME.so" | grep "step_kernel" | head -4
