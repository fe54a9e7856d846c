#!/bin/bash
# usage: tools/ab.sh [-w workload] A B C ...   -> bench with ab/lib_<X>.so alternately, $AB_ROUNDS rounds (default 2) on the same box (the first round
# also checks 20000 rows against the oracle); prints k-subgraphs/s, ms per step, walk / fill kernel ms and the parity row count per run.
# The bench lines go to $AB_OUT (default ab/runs).  A failed run ends the comparison: nothing is started after it.
WL=c5_er_1m
if [ "$1" = "-w" ]; then WL=$2; shift 2; fi
O=${AB_OUT:-ab/runs}; mkdir -p $O
for round in $(seq 1 ${AB_ROUNDS:-2}); do for v in "$@"; do
  if [ $round = 1 ]; then EXTRA="--cpu-sample 20000 --no-cpu-reference"; else EXTRA="--no-cpu-baseline"; fi
  UGS_MI355_LIB=$PWD/ab/lib_$v.so timeout -k 10 300 python bench.py --workload $WL --steps 6 --warmup 2 --full --no-extras $EXTRA > $O/$v.$WL.json 2> $O/$v.$WL.err || { echo "$v FAILED"; tail -3 $O/$v.$WL.err; exit 1; }
  python -c "import json; d=json.load(open('$O/$v.$WL.json')); print('$v', '$WL', round(d['value']/1e6,2), 'M/s  ms/step', d['ms_per_step'], ' walk', d['roofline']['kernel_ms'], 'ms fill', d['roofline']['path']['fill_kernel_ms'], 'parity rows', d.get('parity_checked_rows'))"
done; done
