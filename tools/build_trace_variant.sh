# usage: tools/build_trace_variant.sh NAME "FLAGS"  -> epsm_mitsuba3_amd/libepsm_NAME.so with epsm_trace.hip rebuilt with extra FLAGS
# (linked with every other unit of the library: the objects `make` leaves in build/, epsm_trace.o aside)
set -e
cd "$(dirname "$0")/../epsm_mitsuba3_amd/csrc"
make -s
F="-O3 -std=c++17 --offload-arch=gfx950 -fPIC -ffp-contract=fast -fno-slp-vectorize -Wall -Wno-unused-function -DEPSM_TRACE_NT_STORES"
/opt/rocm/bin/hipcc $F $2 -c -o build/tr_$1.o epsm_trace.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ../libepsm_$1.so $(ls build/epsm_*.o | grep -v '/epsm_trace\.o$') build/tr_$1.o
