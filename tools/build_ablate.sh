#!/bin/bash
# builds tools/libfanlin_gpu_ablate_<name>.so for each "name[:mask[:extra compiler flags]]" given: experiment variants of
# one kernel file (ABL_FILE, default fl_stream.hip, whose FL_ABLATE masks are documented at the head of resample_stream_kernel;
# fl_wtile.hip has its own).  The other sources are the Makefile's SRCS (`make print-srcs`), compiled once and shared.
set -e
cd "$(dirname "$0")/../fanlin-rs_amd/csrc"
mkdir -p /tmp/abl
KFILE=${ABL_FILE:-fl_stream.hip}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math"
ALL=$(make -s print-srcs)
case " $ALL " in *" $KFILE "*) ;; *) echo "$KFILE is not among the library's sources: $ALL" >&2; exit 1 ;; esac
OTHERS=""; for f in $ALL; do [ "$f" = "$KFILE" ] || OTHERS="$OTHERS $f"; done
make -s fl_buildinfo.o >/dev/null # (writes fl_buildinfo.gen.cpp)
for f in $OTHERS fl_buildinfo.gen.cpp; do /opt/rocm/bin/hipcc $FLAGS -x hip -c $f -o /tmp/abl/$f.o & done
for v in "$@"; do
  IFS=: read -r name mask extra <<< "$v"
  /opt/rocm/bin/hipcc $FLAGS -DFL_ABLATE=${mask:-0} ${extra} ${EXTRA} -x hip -c $KFILE -o /tmp/abl/k_$name.o &
done
wait
true
for v in "$@"; do
  name=${v%%:*}
  objs=""; for f in $OTHERS fl_buildinfo.gen.cpp; do objs="$objs /tmp/abl/$f.o"; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../../tools/libfanlin_gpu_ablate_$name.so /tmp/abl/k_$name.o $objs -ldl
done
ls -la ../../tools/*.so
