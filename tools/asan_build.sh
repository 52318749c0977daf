#!/bin/bash
# Host-side AddressSanitizer build of libpskv.so and the C++ boundary programs
# (tests/cpp), into scratch/asan/ (git-ignored).  Only host code is
# instrumented (-Xarch_host); device code is unchanged.  Run the programs on
# the GPU box with ASAN_OPTIONS=detect_leaks=0 (the HIP runtime's own
# allocations are not ours to report), e.g.
#   bash tools/asan_build.sh && ASAN_OPTIONS=detect_leaks=0 scratch/asan/hip_storage_test
# The host planner's test (tests/cpp/host_plan_test.cpp) needs no GPU: it is
# built with the same sanitizers and run by this script.
# UBSan (SAN=address,undefined) is built with -fno-sanitize-recover=all, so any
# report ends the program with a non-zero status instead of only being logged.
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
SAN=${SAN:-address}  # e.g. SAN=address,undefined
NORECOVER=-fno-sanitize-recover=all
O=$R/scratch/asan
mkdir -p "$O"
CXX=/opt/rocm/llvm/bin/clang++
# the library's sources and the test programs: parameter_server_amd/build.py's
# LIB_SOURCES and CPP_TESTS are the only lists
from_build() {
  python3 -c "import runpy; m = runpy.run_path('$R/parameter_server_amd/build.py'); print(' '.join($1))"
}
srcs=()
for f in $(from_build "m['LIB_SOURCES']"); do srcs+=("$R/parameter_server_amd/csrc/$f"); done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -shared \
  -Xarch_host -fsanitize=$SAN -Xarch_host $NORECOVER -Xarch_host -fno-omit-frame-pointer \
  -I "$R/include" -I "$R/parameter_server_amd/csrc" "${srcs[@]}" \
  -o "$O/libpskv.so"
# program:source:links-the-oracle-checker
for t in $(from_build "['%s:%s:%d' % (p, s, o) for p, (s, o) in m['CPP_TESTS'].items()]"); do
  IFS=: read -r p src with_oracle <<<"$t"
  oracle_link=""
  if [ "$with_oracle" = 1 ]; then
    oracle_link="-L $R/oracle -loracle -Wl,-rpath,$R/oracle"
  fi
  # shellcheck disable=SC2086  # oracle_link is a word list on purpose
  $CXX -O1 -g -std=c++11 -pthread -fsanitize=$SAN $NORECOVER -fno-omit-frame-pointer \
    -I "$R/include" "$R/tests/cpp/$src" -o "$O/$p" \
    -L "$O" -lpskv '-Wl,-rpath,$ORIGIN' $oracle_link
done
# the host planner's CPU test (tests/cpp/host_plan_test.cpp): host-only, so it
# is built and run here, no GPU needed
$CXX -O1 -g -std=c++17 -Wall -Werror -fsanitize=$SAN $NORECOVER -fno-omit-frame-pointer \
  -I "$R/include" -I "$R/parameter_server_amd/csrc" "$R/tests/cpp/host_plan_test.cpp" -o "$O/host_plan_test"
"$O/host_plan_test"
# the grouped pooled push's planner (tests/cpp/pooled_push_group_plan_test.cpp): host-only too; the
# loop above built it as build.py does, this is the strict stand-alone form, run here
$CXX -O1 -g -std=c++17 -Wall -Werror -fsanitize=$SAN $NORECOVER -fno-omit-frame-pointer \
  -I "$R/include" -I "$R/parameter_server_amd/csrc" "$R/tests/cpp/pooled_push_group_plan_test.cpp" \
  -o "$O/pooled_push_group_plan_test_alone"
"$O/pooled_push_group_plan_test_alone"
echo "asan build: $O"
