#!/bin/bash
# Build an experimental variant of liblfbm5d_hip.so with extra compiler flags (kernel A/B tests, -DLFBM5D_PHASE_TIMING=1|2):
#   tools/build_variant.sh <name> "<extra hipcc flags>"   ->  lfbm5d_amd/variants/lib_<name>.so
# Select it at run time with LFBM5D_HIP_LIB=lfbm5d_amd/variants/lib_<name>.so.
# The sources and their flags are the Makefile's; the objects go to lfbm5d_amd/variants/obj_<name>/.
set -e
cd "$(dirname "$0")/../lfbm5d_amd/csrc"
name=$1; extra=$2
mkdir -p ../variants/obj_$name
make -j"${JOBS:-8}" OBJDIR=../variants/obj_$name/ EXTRA_HIPFLAGS="$extra" LIB=../variants/lib_$name.so ../variants/lib_$name.so
echo built ../variants/lib_$name.so
