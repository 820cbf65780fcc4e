#!/usr/bin/env bash
# tools/variants.sh — build tuning variants of librt_amd.so into csrc/variants/<name>.so:  name:"-Dflags"
# (development aid for kernel tuning; the shipped library is csrc/librt_amd.so; select one with RT_AMD_LIB=<path>)
set -e
cd "$(dirname "$0")/../raytracing-course-hw-public_amd/csrc"
mkdir -p variants
# the objects of the shipped build, from the Makefile's own lists; the kernel objects are replaced by the variant's
KERNEL_FILES="rt_kernels rt_wavefront rt_wf_extend rt_wf_shade rt_wide"
HOST_OBJS=$(make -s print-host-srcs | sed 's/\.cpp/.o/g')
OTHER_DEV_OBJS=$(make -s print-dev-objs | tr ' ' '\n' | grep -vx $(printf -- '-e %s.o ' $KERNEL_FILES) | tr '\n' ' ')
CC="/opt/rocm/bin/hipcc -std=c++20 -O3 -ffp-contract=off -fPIC -Wall -Wno-unused-function --offload-arch=gfx950 -fno-slp-vectorize"
for spec in "$@"; do
  name="${spec%%:*}"; flags="${spec#*:}"
  objs=""
  for f in $KERNEL_FILES; do
    $CC $flags -c $f.hip -o variants/$name.$f.o &
    objs="$objs variants/$name.$f.o"
  done
  wait
  /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o variants/$name.so $HOST_OBJS $OTHER_DEV_OBJS $objs -lz -ldl
  rm -f $objs
  echo "built $name ($flags)"
done
