#!/bin/bash
# usage: build_variant.sh tag "flags"  -> espflix_amd/libefx_<tag>.so
# The Makefile's own commands for libefx.so (its OBJS, its flags, k_recon.o's extra one), with the given flags added to every
# compile, the objects in build/variant_<tag>/ and the library under the variant's name.  The product's objects are left alone.
set -e -o pipefail
tag=$1; flags=$2
[ -n "$tag" ] || { echo "usage: $0 tag \"flags\"" >&2; exit 2; }
cd "$(dirname "$0")/../.."
d=build/variant_$tag; mkdir -p $d
make -n -B lib | sed -e "s#espflix_amd/csrc/\([A-Za-z0-9_]*\)\.o#$d/\1.o#g" -e "s#-o espflix_amd/libefx\.so#-o espflix_amd/libefx_$tag.so#" > $d/commands
grep -e ' -c ' $d/commands | sed -e "s# -c # $flags -c #" | xargs -d '\n' -P "${MAX_JOBS:-8}" -n 1 sh -c
grep -e ' -shared ' $d/commands | sh -e
echo built $tag
