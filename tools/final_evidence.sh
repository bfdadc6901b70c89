#!/bin/bash
# GPU box: the round's evidence in one call - full gpu suite, rocprofv3 passes (kernel trace, SQ / issue / LDS / FETCH / WRITE and the
# instruction-class census), stage stamps, the bench lines of every configuration, the batch-size curve, the evaluation driver.
# usage: bash tools/final_evidence.sh r05      (results under gpurun_out/; copy what is to be judged into profiles/)
TAG="${1:-r05}"
cd "$(dirname "$0")/.."
R="$(pwd)"
O=gpurun_out
mkdir -p $O
# the driver's own forms, from the repo root, no file arguments (round 5's suite was never run this way and was refused by the pool's gate)
( time timeout 2400 python -m pytest tests/ -x -q -m gpu --durations=15 ) > $O/${TAG}_pytest_gpu.txt 2>&1; echo "pytest rc=$?" >> $O/${TAG}_pytest_gpu.txt
( time python -c "import __graft_entry__ as g; g.smoke()" ) >> $O/${TAG}_pytest_gpu.txt 2>&1; echo "smoke rc=$?" >> $O/${TAG}_pytest_gpu.txt
timeout 1500 bash tools/collect_profiles.sh $TAG > $O/${TAG}_collect.log 2>&1
( export TMPDIR=/tmp; cd /tmp
  BENCH="python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-extras"
  timeout 600 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VALU_ADD_F32 SQ_INSTS_VALU_MUL_F32 SQ_INSTS_VALU_FMA_F32 SQ_INSTS_VALU_TRANS_F32 SQ_INSTS_VALU_CVT SQ_INSTS_VALU_INT32 SQ_INSTS_SALU \
      --kernel-trace --output-format csv -d "$R/$O/profiles_$TAG/pmc_census" -- $BENCH > "$R/$O/profiles_$TAG/pmc_census.log" 2>&1 )
python3 tools/pmc_summary.py "$O/profiles_$TAG/pmc_census" > "$O/profiles_$TAG/summary_pmc_census.txt" 2>&1; rm -rf "$O/profiles_$TAG/pmc_census"
DC_STAMPS=1 DC_DISABLE_GRAPH=1 timeout 600 python tools/stage_stamps.py > $O/${TAG}_stage_stamps.txt 2>&1
timeout 900 python bench.py --full 2> $O/${TAG}_bench_default.err | tail -1 > $O/${TAG}_bench_default.json
timeout 900 python bench.py --full --ddim 1000 --steps 3 --warmup 1 --no-cpu-baseline --no-extras 2>/dev/null | tail -1 > $O/${TAG}_bench_ddim1000.json
timeout 900 python bench.py --full --bs 128 --frames 900 --no-cpu-baseline --no-extras 2>/dev/null | tail -1 > $O/${TAG}_bench_t900.json
timeout 900 python bench.py --full --no-eff --steps 5 --warmup 1 --no-cpu-baseline --no-extras 2>/dev/null | tail -1 > $O/${TAG}_bench_noeff.json
timeout 900 python bench.py --full --precision mixed --no-cpu-baseline --no-extras 2>/dev/null | tail -1 > $O/${TAG}_bench_mixed.json
timeout 900 python tools/batch_curve.py 2>/dev/null > $O/${TAG}_batch_curve.md
timeout 600 python tools/time_evaluate.py --clips 294 2>/dev/null > $O/${TAG}_time_evaluate_294.json
timeout 600 python tools/time_evaluate.py --clips 96 --ddim 1000 --repeat 1 2>/dev/null > $O/${TAG}_time_evaluate_ddim1000.json
tail -40 $O/${TAG}_pytest_gpu.txt; for f in default ddim1000 t900 noeff mixed; do echo -n "$f: "; grep -o "ms_per_step\": [0-9.]*" $O/${TAG}_bench_$f.json; done
