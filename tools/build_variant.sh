#!/bin/bash
# tools/build_variant.sh NAME "-DFLAG ..." — development build of the library with extra flags: zlib.es_amd/libzes_NAME.so
# (use with ZES_LIB=zlib.es_amd/libzes_NAME.so; *.so is git-ignored)
# Built by csrc/Makefile itself (its sources, its flags), run in a fresh object directory so that the product build's
# objects stay as they are; the extra flags ride on the compiler command.
set -e
root="$(cd "$(dirname "$0")/.." && pwd)"
src=$root/zlib.es_amd/csrc
name=$1; shift
obj=$(mktemp -d)
trap 'rm -rf "$obj"' EXIT
# (vpath by pattern, sources and headers only: a plain VPATH would also find the product build's objects in csrc/,
# newer than their sources, and link those without compiling anything)
make -s -j8 -C "$obj" -f "$src/Makefile" --eval "vpath %.hip $src" --eval "vpath %.c $src" --eval "vpath %.h $src" \
  HIPCC="/opt/rocm/bin/hipcc $*" OUT="$root/zlib.es_amd/libzes_$name.so"
echo built zlib.es_amd/libzes_$name.so
