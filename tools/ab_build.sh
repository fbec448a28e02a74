#!/bin/bash
# Build library variants of ONE kernel file under tools/ab/ (timed by tools/ab_bench.sh): the other objects come from the
# product build.  A spec holds every flag the variant needs beyond the common ones, the file's own flags of
# cuttlefish_amd/build.py (PER_FILE_FLAGS) included.
# usage: bash tools/ab_build.sh <file.hip> name1="-DFOO=1" name2="-DBAR=2" ...
# BC7: the remaining ablations are -DCF_BC7_ABLATE=n with n a sum of 1, 2, 4, 8, 16, 32 (csrc/bc7_encode.hip); their payloads differ.
set -e
src=$1; shift
base=$(basename $src .hip)
mkdir -p tools/ab
others=$(ls cuttlefish_amd/build/*.o | grep -v "/$base.o")
for spec in "$@"; do
  name=${spec%%=*}; flags=${spec#*=}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -Wno-unused-function $flags -c -o /tmp/ab_$name.o $src &
done
wait
for spec in "$@"; do
  name=${spec%%=*}
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o tools/ab/$name.so /tmp/ab_$name.o $others
done
ls -la tools/ab
