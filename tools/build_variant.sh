#!/bin/bash
# build_variant.sh NAME SOURCE.hip -DFLAG...: compile one source with extra flags, link it with the regular objects of the other
# sources (tntorch_amd/csrc/build/*.o from `python __graft_entry__.py` or `make -C tntorch_amd/csrc`) into
# tntorch_amd/libttround_NAME.so; use it with TTR_LIB_PATH=tntorch_amd/libttround_NAME.so.
# The object list and the source's regular flags come from tntorch_amd/csrc/Makefile (`print-objs`, FLAGS_<file>).
set -e
cd "$(dirname "$0")/../tntorch_amd/csrc"
name=$1; src=$2; shift 2
flags=$(make -s --eval "print-flags: ; @echo \$(FLAGS_$src)" print-flags)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC $flags "$@" -c "$src" -o "build/${src%.hip}_$name.o"
objs=$(make -s print-objs | sed "s|build/${src%.hip}\.o|build/${src%.hip}_$name.o|")
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC $objs -o "../libttround_$name.so"
echo "built tntorch_amd/libttround_$name.so"
