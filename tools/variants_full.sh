#!/usr/bin/env bash
# tools/variants_full.sh name:"-Dflags" … — like variants.sh, but EVERY object that sees the device data layout (rt_device_types.h) is rebuilt
# with the flags: the kernels, the host and device tree builders and the rt_*.cpp host files. For layout experiments (record sizes, alignment).
set -e
cd "$(dirname "$0")/../raytracing-course-hw-public_amd/csrc"
mkdir -p variants
# the Makefile's own lists: every device object, and the host sources split into those that see rt_device_types.h and the rest (host/*)
DEV_OBJS=$(make -s print-dev-objs)
HOST_SRCS=$(make -s print-host-srcs)
LAYOUT_SRCS=$(echo $HOST_SRCS | tr ' ' '\n' | grep -v '^host/')
OTHER_OBJS=$(echo $HOST_SRCS | tr ' ' '\n' | grep '^host/' | sed 's/\.cpp$/.o/' | tr '\n' ' ')
DEV="/opt/rocm/bin/hipcc -std=c++20 -O3 -ffp-contract=off -fPIC -Wall -Wno-unused-function -Wno-unused-result --offload-arch=gfx950 -fno-slp-vectorize"
HOST="/opt/rocm/bin/hipcc -std=c++20 -O3 -ffp-contract=off -fPIC -Wall -Wno-unused-function -Wno-unused-result -x c++ -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include"
for spec in "$@"; do
  name="${spec%%:*}"; flags="${spec#*:}"
  d=variants/$name.d; mkdir -p $d
  for o in $DEV_OBJS; do $DEV $flags -c ${o%.o}.hip -o $d/$o & done
  for f in $LAYOUT_SRCS; do $HOST $flags -c $f -o $d/${f%.cpp}.o & done
  wait
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o variants/$name.so $OTHER_OBJS $d/*.o -lz -ldl
  rm -rf $d
  echo "built $name ($flags)"
done
