#!/bin/bash
# usage: tools/build_variant.sh <name> [-DFOO=1 ...] -- compiles gpurun_variants/lib_<name>.so with extra flags (dev helper; A/B runs via tools/ab_variants.sh)
set -e
name=$1; shift
cd "$(dirname "$0")/.."
mkdir -p gpurun_variants
lib() {      # the variant's path; sources and flags are those of saro-gs_amd/build.py
echo gpurun_variants/lib_$name.so
}
python3 saro-gs_amd/build.py --force --out "$(lib)" "$@" > /dev/null
lib
