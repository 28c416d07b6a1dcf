#!/bin/bash
# rocprofv3 instruction-cache and instruction-fetch counters of bench.py's headline kernel on the GPU box, beside
# tools/profile.sh: one counter group per run, nothing but the kernel trace with it.  A pass that fails ends the script.
# Usage: tools/profile_icache.sh <output directory>   (from the repository root; the passes are condensed into
# pmc_summary.json there: mean / min / max per counter over the headline kernel's launches)
set -u
R=$(pwd)
O=$(realpath -m "${1:?output directory}")
mkdir -p "$O"
export TMPDIR=/tmp
pass() {   # pass <name> <counters...>
  local name=$1; shift
  timeout -k 10 240 rocprofv3 --kernel-trace --pmc "$@" --output-format csv -d "$O/pmc/$name" -- python3 "$R/bench.py" --steps 3 --warmup 1 --no-cpu-baseline --no-extra > "$O/pmc_$name.log" 2>&1
  local rc=$?
  echo "$name=$rc"
  if [ $rc -ne 0 ]; then tail -20 "$O/pmc_$name.log"; exit $rc; fi
}
pass icache SQC_ICACHE_REQ SQC_ICACHE_HITS SQC_ICACHE_MISSES SQC_ICACHE_MISSES_DUPLICATE
pass ifetch SQ_IFETCH SQ_WAIT_INST_ANY SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY SQ_WAVES SQ_BUSY_CYCLES
pass icache2 SQC_ICACHE_BUSY_CYCLES SQC_ICACHE_INPUT_VALID_READYB SQ_INSTS_SALU SQ_INSTS_VALU SQ_INSTS_BRANCH
pass latency InstrFetchLatency
python3 - "$O" <<'EOF'
import csv, glob, json, os, sys
src = sys.argv[1]
res = {}
for tag in sorted(os.listdir(os.path.join(src, "pmc"))):
    per = {}
    for f in glob.glob(os.path.join(src, "pmc", tag, "**", "*counter_collection.csv"), recursive=True):
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                if "gibbs_sweeps_kernel" in r["Kernel_Name"]:
                    per.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
        with open(f) as fh, open(os.path.join(src, "pmc_%s_counters_head.csv" % tag), "w") as out:
            out.writelines(ln for i, ln in enumerate(fh) if i == 0 or ("gibbs_sweeps_kernel" in ln and i < 400))
    res[tag] = {"launches": {k: len(v) for k, v in per.items()}, "mean": {k: sum(v) / len(v) for k, v in per.items()},
                "min": {k: min(v) for k, v in per.items()}, "max": {k: max(v) for k, v in per.items()}}
json.dump(res, open(os.path.join(src, "pmc_summary.json"), "w"), indent=1)
print(json.dumps({t: v["mean"] for t, v in res.items()}, indent=1))
EOF
