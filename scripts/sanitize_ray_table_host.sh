#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host code of the per-view ray table (csrc/vp_tables.cpp ensure_ray_table) in a
# stand-alone program with stand-ins for the HIP runtime and the launches (scripts/sanitize_ray_table_host.cpp).  Host code only: needs
# no GPU, loads nothing into Python, leaves the regular build alone.
set -e
cd "$(dirname "$0")/.."
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
T=$(mktemp -d)
trap 'rm -rf $T' EXIT
FLAGS="-O1 -g -std=c++17 -x hip --cuda-host-only -ffp-contract=off -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wall -Wno-unused-function"
$HIPCC $FLAGS -c cuda-volpath_amd/csrc/vp_tables.cpp -o $T/vp_tables.o
$HIPCC $FLAGS -c scripts/sanitize_ray_table_host.cpp -o $T/main.o
$HIPCC -fsanitize=address,undefined $T/main.o $T/vp_tables.o -o $T/ray_table_host
ASAN_OPTIONS=halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $T/ray_table_host
