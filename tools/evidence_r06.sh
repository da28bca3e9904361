#!/bin/bash
# Round-6 evidence from ONE build: `gpurun -- bash tools/evidence_r06.sh <part>`; results under gpurun_out/evidence_r06/, copied into profiles/r06_* afterwards
# (profiles/README.md says which file came from which part).
#   bench  : bench.py lines - C3 with the driver's flags (twice: cpu_baseline, parity, tolerance_engine), one context (+ per-op table), int8, C2 / C4 / C5
#   prof   : rocprofv3 --kernel-trace --stats of C3 (three contexts; one context on one lane), of the fp32 engine (one context, one lane) and of C5,
#            and the PMC pass for the conv family's HBM traffic on C3 (its own run: --pmc with --kernel-trace only)
#   suite  : the full `pytest -m gpu` with parity drift as a FAILURE (the default); the parity record of the run is kept
export TMPDIR=/tmp
export TRTX_TACTIC_CACHE=/tmp/trtx_tactics.txt   # one set of tactic timings for every process of this script: the rocprofv3 runs see real launches only
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
E=$R/gpurun_out/evidence_r06
mkdir -p $E
cd $R
PART=${1:-all}
if [ $PART = bench ] || [ $PART = all ]; then
  for i in 1 2; do
    timeout 500 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $E/bench_c3_driverflags_$i.log 2> $E/bench_c3_driverflags_$i.err
  done
  timeout 300 python bench.py --full --steps 20 --warmup 5 --contexts 1 --no-cpu-baseline --no-tolerance-engine --dump-ops $E/ops_c3_1ctx.json > $E/bench_c3_1ctx.log 2>/dev/null
  timeout 500 python bench.py --full --steps 20 --warmup 5 --precision int8 > $E/bench_c3_int8.log 2>/dev/null
  for cfg in resnet50 retinaface_r50 rcnn_r50c4; do
    timeout 600 python bench.py --full --config $cfg --steps 20 --warmup 5 > $E/bench_$cfg.log 2>/dev/null
  done
  python tools/show_bench.py $E/bench_*.log
  timeout 300 python tools/layer_table.py $E/layer_table.json > $E/layer_table.txt 2>&1; tail -5 $E/layer_table.txt
  timeout 300 python tools/f32_engine_probe.py > $E/f32_engine_probe.txt 2>&1; grep -v "^   op\|   tactic" $E/f32_engine_probe.txt | tail -6
fi
if [ $PART = prof ] || [ $PART = all ]; then
  timeout 300 python bench.py --full --steps 5 --warmup 2 --repeats 3 --no-cpu-baseline > /dev/null 2>&1            # fills the tactic cache (3 contexts + 1 context + fp32 engines)
  prof() {  # name, command
    (cd /tmp && timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $E/prof_$1 -o p -- $2 > $E/prof_$1.log 2>&1)
    { echo "# rocprofv3 --kernel-trace --stats -- $2   (round 6; TRTX_TACTIC_CACHE set: no tactic-timing launches inside)"; python tools/rocprof_summary.py $E/prof_$1; } > $E/kernel_stats_$1.txt 2>&1
    head -12 $E/kernel_stats_$1.txt | cut -c1-170
    rm -rf $E/prof_$1
  }
  prof c3 "python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-tolerance-engine"
  TRTX_LANES=1 prof c3_1ctx_lanes1 "python $R/bench.py --full --contexts 1 --steps 20 --warmup 5 --no-cpu-baseline --no-tolerance-engine"
  TRTX_LANES=1 prof c3_fp32_1ctx_lanes1 "python $R/tools/f32_engine_probe.py --contexts 1 --steps 40 --no-oracle"
  timeout 300 python bench.py --full --config rcnn_r50c4 --steps 3 --warmup 1 --repeats 3 --no-cpu-baseline > /dev/null 2>&1
  TRTX_LANES=1 prof c5_1ctx_lanes1 "python $R/bench.py --full --config rcnn_r50c4 --contexts 1 --steps 20 --warmup 5 --no-cpu-baseline"
  # (round 6: the one-context kernel statistics of C2, C4 and the int8 build too - VERDICT r5 Weak 6 / item 8)
  timeout 300 python bench.py --full --config resnet50 --steps 3 --warmup 1 --repeats 3 --no-cpu-baseline > /dev/null 2>&1
  TRTX_LANES=1 prof c2_1ctx_lanes1 "python $R/bench.py --full --config resnet50 --contexts 1 --steps 20 --warmup 5 --no-cpu-baseline"
  timeout 300 python bench.py --full --config retinaface_r50 --steps 3 --warmup 1 --repeats 3 --no-cpu-baseline > /dev/null 2>&1
  TRTX_LANES=1 prof c4_1ctx_lanes1 "python $R/bench.py --full --config retinaface_r50 --contexts 1 --steps 20 --warmup 5 --no-cpu-baseline"
  timeout 400 python bench.py --full --precision int8 --steps 3 --warmup 1 --repeats 3 --no-cpu-baseline > /dev/null 2>&1
  TRTX_LANES=1 prof c3_int8_1ctx_lanes1 "python $R/bench.py --full --precision int8 --contexts 1 --steps 20 --warmup 5 --no-cpu-baseline"
  OUT=$E/pmc_yolov8n
  (cd /tmp && timeout 400 rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum --kernel-trace --output-format csv -d $OUT -o c -- python $R/bench.py --full --config yolov8n --contexts 1 --steps 3 --warmup 1 --repeats 3 --no-cpu-baseline --no-tolerance-engine > $OUT.log 2>&1)
  python - <<PY | tee $E/pmc_conv_traffic.txt
import csv, glob, collections
fs = glob.glob("$E/pmc_yolov8n/**/c_counter_collection.csv", recursive=True)
per = collections.defaultdict(lambda: collections.defaultdict(float)); n = collections.Counter(); seen = set()
for r in csv.DictReader(open(fs[0])):
    k = r["Kernel_Name"]
    fam = "conv" if ("conv_igemm" in k or "conv_ws" in k or "conv_gemm256" in k or "conv_patch" in k or "conv_res" in k) else ("conv_stem" if "conv_stem" in k else ("yolo" if "yolo" in k else "other"))
    per[fam][r["Counter_Name"]] += float(r["Counter_Value"])
    key = (r["Dispatch_Id"], fam)
    if key not in seen:
        seen.add(key); n[fam] += 1
print("# rocprofv3 --pmc TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum --kernel-trace over bench.py --contexts 1 --steps 3 --warmup 1 --repeats 3 (round 6)")
print("# bytes = (2 x RDREQ + WRREQ) x 64 B  (reads doubled: gfx950 counts 128-B read requests at 64 B, MI355X_MICROARCH.md HBM section)")
for fam, d in per.items():
    rd, wr = d.get("TCC_EA0_RDREQ_sum", 0.0), d.get("TCC_EA0_WRREQ_sum", 0.0)
    print(f"yolov8n {fam:12s} launches {n[fam]:6d}  RDREQ {rd:14.0f}  WRREQ {wr:14.0f}  bytes/launch {(2 * rd + wr) * 64 / max(n[fam], 1):14.0f}")
PY
  rm -rf $E/pmc_yolov8n/
fi
if [ $PART = suite ] || [ $PART = all ]; then
  rm -f gpurun_out/parity_metrics.jsonl
  unset TRTX_TACTIC_CACHE
  timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -12 | tee $E/pytest_gpu_$(date +%H%M%S).txt
  cp gpurun_out/parity_metrics.jsonl $E/parity_$(date +%H%M%S).jsonl
fi
if [ $PART = harness ]; then
  timeout 200 tools/hip/bin/mfma_f32_rate 2>&1 | tee $E/mfma_f32_rate.txt
  timeout 200 tools/hip/bin/igemm_f32_anatomy 2>&1 | tee $E/igemm_f32_anatomy.txt
  timeout 100 tools/hip/bin/igemm_f32_residency 2>&1 | tee $E/igemm_f32_residency.txt
  timeout 100 tools/hip/bin/igemm_residency 2>&1 | tee $E/igemm_residency.txt
fi
