#!/bin/bash
# Experiment builds: tools/build_variant.sh NAME [-DMACRO=..]...  ->  sea-current_amd/variants/NAME.so (astar.hip rebuilt
# with the given macros, the other objects as they are); select with SC_LIB_PATH.  ASTAR_SRC=file: another astar.hip
# (e.g. `git show HEAD:sea-current_amd/csrc/astar.hip > sea-current_amd/csrc/astar_prev.hip`), for A/B runs on one box.
set -e
cd "$(dirname "$0")/../sea-current_amd"
name=$1; shift
mkdir -p variants
make -s all
unit=${VARIANT_UNIT:-astar}     # which source is rebuilt with the macros (astar, edt, bezier, ...)
src=csrc/$unit.hip
[ $unit = astar ] && src=${ASTAR_SRC:-csrc/astar.hip}
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-function "$@" -c $src -o variants/$name.$unit.o
# the Makefile's object list, with the rebuilt unit swapped in
objs=$(make -s print-objs | sed "s#csrc/$unit\.o#variants/$name.$unit.o#")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o variants/$name.so $objs -ldl
rm -f variants/$name.$unit.o
echo built variants/$name.so
