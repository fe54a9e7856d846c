#!/bin/bash
# usage: tools/mkvar.sh <name> [extra hipcc flags...]  -> ab/lib_<name>.so (kernels + host rebuilt with the flags, other objects reused)
# KSRC=<file> compiles that copy of the walk kernels instead (e.g. the parent commit's, from `git show`); headers come from csrc/.
# A/B variants of the walk kernel for same-box comparisons (tools/ab.sh); ab/ is git-ignored (*.so) but travels to the GPU box.
set -e
NAME=$1; shift
ROOT=$(cd "$(dirname "$0")/.." && pwd)
HERE=$ROOT/ss-gnn_amd/csrc
W=/tmp/vb/$NAME; mkdir -p $W $ROOT/ab; rm -f $W/*.o
FL="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -x hip"
HOST="ugs_host ugs_jobs ugs_side_eps ugs_side_uniform ugs_side_rwr ugs_cache_common ugs_rwr_cache ugs_graph_cache ugs_eps_cache"     # the host translation units (ugs_host_internal.h)
/opt/rocm/bin/hipcc $FL -mllvm -amdgpu-sched-strategy=${SCHED:-max-ilp} "$@" -I$HERE -c ${KSRC:-$HERE/ugs_kernels.hip} -o $W/ugs_kernels.o &
for f in $HOST; do /opt/rocm/bin/hipcc $FL "$@" -c $HERE/$f.cpp -o $W/$f.o & done
wait
for f in ugs_kernels $HOST; do [ -f $W/$f.o ] || { echo "$f did not compile"; exit 1; }; done
for f in ugs_eps ugs_uniform ugs_rwr ugs_preproc ugs_apx ugs_apx_gpu ugs_collate ugs_batch ugs_wl ugs_store; do [ -f $HERE/$f.o ] || { echo "missing $HERE/$f.o (run build.py)"; exit 1; }; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o $ROOT/ab/lib_$NAME.so $W/ugs_kernels.o $(for f in $HOST; do echo $W/$f.o; done) $HERE/ugs_eps.o $HERE/ugs_uniform.o $HERE/ugs_rwr.o $HERE/ugs_preproc.o $HERE/ugs_apx.o $HERE/ugs_apx_gpu.o $HERE/ugs_collate.o $HERE/ugs_batch.o $HERE/ugs_wl.o $HERE/ugs_store.o
echo built ab/lib_$NAME.so
