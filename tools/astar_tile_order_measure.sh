#!/bin/bash
# Run on a box with one MI355X, from the repository root, with this tree built:
#   bash tools/astar_tile_order_measure.sh <library built from the parent commit> <output directory>
# then: python tools/astar_tile_order_collect.py <output directory>
# Parent and this tree take turns, a fresh process per run: bench.py (six runs each), --map salt05 and --map blocks
# (three each), bench.py --full (one each), and tools/astar_saturation.py salt20 6144 under rocprofv3 --pmc, one pass per
# counter group.  Every step runs under a time limit of its own and the script ends at the first step that fails.
set -u
R=$PWD
PARENT=$(readlink -f "$1")
O=$(readlink -f "$2")
mkdir -p $O
step() {   # step <seconds> <log> <command ...>
    local lim=$1 log=$2; shift 2
    timeout -k 10 $lim "$@" > $log 2> $log.err
    local rc=$?
    if [ $rc -ne 0 ]; then echo "FAILED rc=$rc: $* (see $log)"; tail -5 $log $log.err; exit $rc; fi
}
uselib() { if [ $1 = parent ]; then export SC_LIB_PATH=$PARENT; else unset SC_LIB_PATH; fi; }
value() { python -c "import json; print(json.load(open('$1'))['value'])"; }

for i in 1 2 3 4 5 6; do for lib in parent new; do uselib $lib
    step 200 $O/bench_salt20_${lib}_$i.json python bench.py
    echo "salt20 $lib $i $(value $O/bench_salt20_${lib}_$i.json)"
done; done
for map in salt05 blocks; do for i in 1 2 3; do for lib in parent new; do uselib $lib
    step 200 $O/bench_${map}_${lib}_$i.json python bench.py --map $map
    echo "$map $lib $i $(value $O/bench_${map}_${lib}_$i.json)"
done; done; done
for lib in parent new; do uselib $lib
    step 500 $O/bench_full_$lib.json python bench.py --full
    echo "full $lib done"
done
cd /tmp && export TMPDIR=/tmp
for lib in parent new; do uselib $lib
    for grp in "TCC_HIT_sum TCC_MISS_sum" "TCC_ATOMIC_sum" "FETCH_SIZE" "WRITE_SIZE"; do
        tag=$(echo $grp | tr ' ' '_')
        step 200 $O/pmc_${lib}_$tag.log rocprofv3 --kernel-trace --pmc $grp --output-format csv -d $O/pmc_${lib}_$tag -o a -- python3 $R/tools/astar_saturation.py salt20 6144
        echo "pmc $lib $grp done: $(tail -1 $O/pmc_${lib}_$tag.log)"
    done
done
echo all done
