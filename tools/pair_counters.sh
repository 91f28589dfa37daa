#!/bin/bash
# tools/pair_counters.sh [LIBDIR] [NAME] [OUTDIR] : SQ counters of the pair kernel in the bench's production step (grav_pair_kernel_live beside the main
# walk; a profiler that collects counters runs the two one after the other, so the pair kernel finds every flag up and its figures are its
# own), with the in-tree libraries or with the build in LIBDIR.  Every counter group is a rocprofv3 run of its own (--pmc alone, no
# tracing), each under its own time limit; the first failure ends the script.  Writes OUTDIR/NAME.json (OUTDIR: build/pair_counters unless given): per dispatch
# and per task (262144 tasks at 256^3).  GPU box, repo root.
set -e -o pipefail
ROOT=$(pwd); OUT=$ROOT/${3:-build/pair_counters}; mkdir -p $OUT; export TMPDIR=/tmp
[ -n "$1" ] && export SHQ_LIBDIR=$ROOT/$1
NAME=${2:-tree}
cd /tmp
B="python3 $ROOT/bench.py --steps 2 --warmup 1 --no-cpu-baseline --no-sph"
one() { find "$1" -name "*$2" | head -1; }
i=0
for grp in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_SMEM SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY" \
           "SQ_ACTIVE_INST_SCA SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_BRANCH SQ_ACTIVE_INST_LDS SQ_WAIT_ANY SQ_ACTIVE_INST_VMEM"; do
  i=$((i+1))
  rm -rf $OUT/p$i
  timeout -k 10 240 rocprofv3 --pmc $grp --output-format csv -d $OUT/p$i -o q -- $B > $OUT/$NAME.p$i.log 2>&1 || { echo "pass $i failed"; tail -5 $OUT/$NAME.p$i.log; exit 1; }
  python3 $ROOT/tools/pmc_summary.py pmc "$(one $OUT/p$i counter_collection.csv)" > $OUT/$NAME.c$i.json
  rm -rf $OUT/p$i
done
python3 - $OUT $NAME <<PY
import json, sys
out, name = sys.argv[1], sys.argv[2]
res = {}
for i in (1, 2):
    for k, v in json.load(open("%s/%s.c%d.json" % (out, name, i))).items():
        if k.startswith("grav_pair_kernel"):
            res.setdefault(k, {}).update(v)
res = {k: v for k, v in res.items() if v.get("SQ_INSTS_VALU", 0) > 1e6}   # not the mop-up pass that returns at once
per_task = {k: {c: x / 262144.0 for c, x in v.items() if c.startswith("SQ_") and c != "SQ_WAVES"} for k, v in res.items()}
json.dump({"per_dispatch": res, "per_task": per_task}, open("%s/%s.json" % (out, name), "w"), indent=1, sort_keys=True)
for k, v in per_task.items():
    print(name, k, {c: round(x, 1) for c, x in sorted(v.items())})
PY
