#!/usr/bin/env bash
# tools/variants.sh — build tuning variants of librt_amd.so into csrc/variants/<name>.so:  name:"-Dflags"
# (development aid for kernel tuning; the shipped library is csrc/librt_amd.so; select one with RT_AMD_LIB=<path>)
set -e
cd "$(dirname "$0")/../raytracing-course-hw-public_amd/csrc"
mkdir -p variants
# the objects of the shipped build, from the Makefile's own lists; the three kernel objects are replaced by the variant's
HOST_OBJS=$(make -s print-host-srcs | sed 's/\.cpp/.o/g')
OTHER_DEV_OBJS=$(make -s print-dev-objs | tr ' ' '\n' | grep -vx -e rt_kernels.o -e rt_wavefront.o -e rt_wide.o | tr '\n' ' ')
CC="/opt/rocm/bin/hipcc -std=c++20 -O3 -ffp-contract=off -fPIC -Wall -Wno-unused-function --offload-arch=gfx950 -fno-slp-vectorize"
for spec in "$@"; do
  name="${spec%%:*}"; flags="${spec#*:}"
  $CC $flags -c rt_kernels.hip -o variants/$name.k.o &
  $CC $flags -c rt_wavefront.hip -o variants/$name.w.o &
  $CC $flags -c rt_wide.hip -o variants/$name.x.o &
  wait
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o variants/$name.so $HOST_OBJS $OTHER_DEV_OBJS variants/$name.k.o variants/$name.w.o variants/$name.x.o -lz -ldl
  rm -f variants/$name.k.o variants/$name.w.o variants/$name.x.o
  echo "built $name ($flags)"
done
