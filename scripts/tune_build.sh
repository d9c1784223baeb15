#!/bin/bash
# Kernel tuning builds: scripts/tune_build.sh NAME [extra hipcc flags...]  ->  build/tune/liblk_NAME.so
# (affine + reference bicubic solve kernels only; select with LK_ENGINE_LIB=build/tune/liblk_NAME.so)
# The source list is correlation_amd/build.py's: a library of every unit the package's own build links.
set -e
cd "$(dirname "$0")/../correlation_amd/csrc"
name=$1; shift
mkdir -p ../../build/tune
sources=$(python3 -c 'import sys; sys.path.insert(0, ".."); import build; print(" ".join(build.SOURCES))')
/opt/rocm/bin/hipcc -O3 --offload-arch=gfx950 -fPIC -shared -std=c++17 -ffp-contract=off \
  -fhip-fp32-correctly-rounded-divide-sqrt -fno-slp-vectorize -DLK_TUNE_ONLY_AFFINE_BICUBIC "$@" \
  -o ../../build/tune/liblk_$name.so $sources -lrocprofiler-sdk-roctx -lrccl -lz
echo build/tune/liblk_$name.so
