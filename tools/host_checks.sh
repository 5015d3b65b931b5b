#!/usr/bin/env bash
# host_checks.sh -- builds and runs every tools/*_host_check.c* under the host sanitizers (address + undefined).
#
# The library is compiled once with the sanitizers on its host code (the device code is built as always, and never runs),
# every check is linked against that object, and the checks run one after the other; the first failure -- a failed check,
# a sanitizer report, a leak -- ends the script with a non-zero status.  No device is needed or touched: every check
# works without a context.  A CPU tool: it takes a few minutes, almost all of them in the compile of the library.
#
#   tools/host_checks.sh                  every check
#   tools/host_checks.sh tbe treedist     only tools/tbe_host_check.c and tools/treedist_host_check.c
#   HOST_CHECKS_DIR=dir                   where the objects and programs go (default: build/host_checks; the library
#                                         object is rebuilt only when a source under tetrad_amd/csrc or include/ is newer)
set -euo pipefail

repo=$(cd "$(dirname "$0")/.." && pwd)
out=${HOST_CHECKS_DIR:-$repo/build/host_checks}
hipcc=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
clang=${CLANG:-$(command -v clang || echo /opt/rocm/llvm/bin/clang)}
san=-fsanitize=address,undefined
mkdir -p "$out"

lib=$out/tetrad_hip_san.o
if [ ! -e "$lib" ] || [ -n "$(find "$repo/tetrad_amd/csrc" "$repo/include" \( -name '*.hip' -o -name '*.hpp' -o -name '*.h' \) -newer "$lib")" ]; then
    echo "host_checks: compiling the library with $san (host code only)"
    "$hipcc" -O1 -g -std=c++17 --offload-arch=gfx950 -Wno-inline-asm -Xarch_host $san \
        -c "$repo/tetrad_amd/csrc/tetrad_hip.hip" -o "$lib"
fi

if [ $# -gt 0 ]; then
    sources=()
    for name in "$@"; do sources+=("$repo"/tools/"$name"_host_check.c*); done
else
    sources=("$repo"/tools/*_host_check.c*)
fi

for src in "${sources[@]}"; do
    name=$(basename "$src")
    name=${name%%.*}
    case $src in
    *.c) "$clang" -O1 -g $san -I"$repo/include" -c "$src" -o "$out/$name.o" ;;
    *) "$clang" -x c++ -std=c++17 -O1 -g $san -I"$repo/include" -c "$src" -o "$out/$name.o" ;;
    esac
    "$hipcc" $san "$lib" "$out/$name.o" -o "$out/$name"
    "$out/$name"
done
echo "host_checks: all ok"
