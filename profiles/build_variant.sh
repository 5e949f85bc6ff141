#!/bin/bash
# Build an A/B variant of libspindyn.so with extra -D flags for kernels_apply.hip and basis.cpp (each source reads the flags it
# knows: SD_PACK_* the kernel, SD_ORBIT_* the planner):  bash profiles/build_variant.sh <name> -DFOO=1 ...
# -> spindynamics.jl_amd/csrc/_var/libspindyn_<name>.so (git-ignored; travels to the GPU box); compare with profiles/ab_lib.py
# -DSD_PACK_TRACE=1 (per-block time stamps of the packed launch, profiles/pack_trace.py) adds a field to sd_dev_model, which
# every source sees: with it ALL sources are compiled with the flags.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../spindynamics.jl_amd/csrc"
make -s -j8
mkdir -p _var
FLAGS="-O3 -std=c++17 -fPIC -ffp-contract=off --offload-arch=gfx950 -Wno-unused-function"
case " $* " in
  *" -DSD_PACK_TRACE="[1-9]*)
    mkdir -p _var/obj_$NAME
    for s in *.cpp *.hip; do
      case $s in *.cpp) X="-x hip";; *) X="";; esac
      /opt/rocm/bin/hipcc $FLAGS "$@" $X -c $s -o _var/obj_$NAME/$s.o &
    done
    wait
    for s in *.cpp *.hip; do test -s _var/obj_$NAME/$s.o; done
    /opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 _var/obj_$NAME/*.o -o _var/libspindyn_$NAME.so
    echo built _var/libspindyn_$NAME.so "(all sources)"
    exit 0;;
esac
/opt/rocm/bin/hipcc $FLAGS "$@" -c kernels_apply.hip -o _var/kernels_apply_$NAME.o
/opt/rocm/bin/hipcc $FLAGS "$@" -x hip -c basis.cpp -o _var/basis_$NAME.o
OBJS=$(ls _obj/*.o | grep -v -e kernels_apply -e basis.cpp)
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 $OBJS _var/kernels_apply_$NAME.o _var/basis_$NAME.o -o _var/libspindyn_$NAME.so
echo built _var/libspindyn_$NAME.so
