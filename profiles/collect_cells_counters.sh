#!/bin/bash
# Where the cycles of the classifier's two set-abstraction cell launches go (both are sa_cell_kernel instantiations):
#   bash profiles/collect_cells_counters.sh <tag> [library.so] [outdir]   -> <outdir>/<tag>_cls_b64_kernel_stats.csv, <outdir>/<tag>.json
# (outdir: bench_out by default)
# One kernel-trace pass of the replayed graph for the per-kernel times, then counter passes of their own (--pmc alone, no tracing
# next to it; eager launches so that every kernel is a dispatch the profiler sees; only the cell kernels are collected).  A pass
# that ends with ANY non-zero status ends the script: nothing else is started on that GPU.
TAG=${1:-cells}
LIB=${2:-}
export TMPDIR=/tmp
O=${3:-bench_out}
mkdir -p $O
if [ -n "$LIB" ]; then RUN="python tools/bench_with_lib.py $LIB"; else RUN="python bench.py"; fi
stop_on_fault() { if [ "$1" -ne 0 ]; then echo "pass ended with status $1: stopping"; exit "$1"; fi; }

rm -rf $O/prof_$TAG
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$TAG -o p -f csv -- $RUN --worker --steps 20 --warmup 5 --full --no-cpu-baseline --no-others > $O/${TAG}_trace.log 2>&1
stop_on_fault $?
cp $O/prof_$TAG/p_kernel_stats.csv $O/${TAG}_cls_b64_kernel_stats.csv 2>/dev/null || find $O/prof_$TAG -name '*kernel_stats.csv' -exec cp {} $O/${TAG}_cls_b64_kernel_stats.csv \;

n=0
for group in "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAVES GRBM_GUI_ACTIVE SQ_INSTS_VALU SQ_INSTS_MFMA" \
             "SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_ANY SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM" \
             "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_VMEM"; do
  n=$((n + 1))
  rm -rf $O/pmc_${TAG}_$n
  timeout -k 10 300 rocprofv3 --pmc $group --kernel-include-regex sa_cell_kernel -d $O/pmc_${TAG}_$n -o c -f csv -- \
    $RUN --worker --steps 3 --warmup 1 --no-cpu-baseline --no-graph --no-others > $O/${TAG}_pmc_$n.log 2>&1
  stop_on_fault $?
done

python - "$TAG" "$O" <<'PY'
import collections, csv, glob, json, sys
tag, O = sys.argv[1], sys.argv[2]
acc = collections.defaultdict(lambda: collections.defaultdict(list))
for f in glob.glob(f"{O}/pmc_{tag}_*/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "sa_cell_kernel" in r["Kernel_Name"]:
            name = r["Kernel_Name"].split("(")[0].replace("void ", "")
            acc[name][r["Counter_Name"]].append(float(r["Counter_Value"]))
            acc[name]["_grid"].append(float(r.get("Grid_Size", 0) or 0))
            acc[name]["_vgpr"].append(float(r.get("VGPR_Count", 0) or 0) + float(r.get("Accum_VGPR_Count", 0) or 0))
out = {}
for k, v in acc.items():
    out[k] = {c: round(sum(x) / len(x), 1) for c, x in sorted(v.items())}
    out[k]["_launches_averaged"] = len(v.get("SQ_WAVES", v.get("SQ_WAIT_ANY", [])))
json.dump(out, open(f"{O}/{tag}.json", "w"), indent=1, sort_keys=True)
print(json.dumps(out, indent=1, sort_keys=True))
PY
