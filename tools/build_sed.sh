#!/bin/bash
# Build libdpt.so of the working tree's csrc with one sed expression applied to the text of the tokenize unit:
# dpt_kernels.hip, dpt_long.hip, every dpt_tok_*.h, and dpt_wave.h, where the unit's own wave primitives live beside
# the ones every kernel file shares (A/Bs of a constant without a compile-time knob in the source):
#   bash tools/build_sed.sh <tag> '<sed expression>'  ->  dp-tokenization_amd/csrc/build/var_<tag>/libdpt.so
set -e
cd "$(dirname "$0")/.."
tag=$1; expr=$2
tmp=$(mktemp -d /tmp/dpt_sed_XXXX)
mkdir -p "$tmp/dp-tokenization_amd" && cp -r dp-tokenization_amd/csrc "$tmp/dp-tokenization_amd/" && cp -r include "$tmp/"
rm -rf "$tmp/dp-tokenization_amd/csrc/build"
changed=0
for p in dp-tokenization_amd/csrc/dpt_kernels.hip dp-tokenization_amd/csrc/dpt_long.hip dp-tokenization_amd/csrc/dpt_wave.h \
         dp-tokenization_amd/csrc/dpt_tok_*.h; do
    sed -i -e "$expr" "$tmp/$p"
    diff -q "$p" "$tmp/$p" > /dev/null || changed=1
done
[ $changed = 1 ] || { echo "sed changed nothing"; exit 1; }
out=$PWD/dp-tokenization_amd/csrc/build/var_$tag
mkdir -p "$out"
make -s -C "$tmp/dp-tokenization_amd/csrc" -j8 OUT="$out/libdpt.so" "$out/libdpt.so"
rm -rf "$tmp"
ls -la "$out/libdpt.so"
