#!/bin/bash
# Faster form of tools/build_variant.sh for A/B runs that touch few files: only the named sources are recompiled with the extra
# flags, every other object is the product build's (lfbm5d_amd/csrc/*.o, brought up to date first).
#   tools/build_variant_files.sh <name> "<extra hipcc flags>" group_ht aggregate ...   ->  lfbm5d_amd/variants/lib_<name>.so
set -e
cd "$(dirname "$0")/../lfbm5d_amd/csrc"
name=$1; extra=$2; shift 2
mkdir -p ../variants/obj_$name
make -j"${JOBS:-8}" ../liblfbm5d_hip.so
make -j"${JOBS:-8}" OBJDIR=../variants/obj_$name/ EXTRA_HIPFLAGS="$extra" VARIANT_SRCS="${*/#/lfbm5d_}" LIB=../variants/lib_$name.so ../variants/lib_$name.so
echo built ../variants/lib_$name.so
