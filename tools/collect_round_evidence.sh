# usage: tools/collect_round_evidence.sh OUTPUT_DIR   (the output directory of the GPU run)
OUT=${1:?output directory}
set -x
bash tools/collect_profiles.sh r06 > $OUT/r06_collect.log 2>&1
python bench.py --full > $OUT/r06_bench_default.log 2>&1
tail -1 $OUT/r06_bench_default.log > $OUT/r06_bench_bf16.json
cut -c1-300 $OUT/r06_bench_bf16.json
bash tools/collect_config_evidence.sh r06 > $OUT/r06_config_evidence.log 2>&1
tail -9 $OUT/r06_config_evidence.log
python bench.py --frames 8 --steps 3 --warmup 1 2>/dev/null | tail -1 > $OUT/r06_frames8.json
bash tools/collect_train_profiles.sh r06 > $OUT/r06_train_profiles.log 2>&1
python tools/power_trace.py bf16 250 > $OUT/r06_power_trace.txt 2>&1
python tools/soak_determinism.py 12 > $OUT/r06_soak_determinism.txt 2>&1; tail -2 $OUT/r06_soak_determinism.txt
