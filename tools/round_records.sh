# round 6's records that are not part of profile_round.sh (run from the repo root; written under $OUT, copies go to profiles/ by hand)
OUT=${OUT:-bench_out}
mkdir -p $OUT
python bench.py --full > $OUT/r06_bench_default.json 2> $OUT/r06_bench_default.err
python bench.py --driver multi-device --gpus 1 --steps 5 --warmup 2 > $OUT/r06_multi_n1.json 2>> $OUT/r06_bench_default.err
python bench.py --driver multi-device --gpus 2 --devices 0,0 --steps 5 --warmup 2 > $OUT/r06_multi_n2_same_gpu.json 2>> $OUT/r06_bench_default.err
if [ "${1:-}" = "all" ]; then
python tools/concordance.py --samples 1024 --emit-mode tables --margins > $OUT/r06_concordance_tables_200k_x_1024.json 2>> $OUT/r06_bench_default.err
python tools/concordance.py --samples 1024 --emit-mode tables --margins --deep > $OUT/r06_concordance_tables_deep_200k_x_1024.json 2>> $OUT/r06_bench_default.err
python tools/concordance.py --samples 1024 --emit-mode tables --margins --depth 400 > $OUT/r06_concordance_tables_depth400_200k_x_1024.json 2>> $OUT/r06_bench_default.err
python tools/concordance.py --samples 1024 --emit-mode tables --margins --depth 1600 > $OUT/r06_concordance_tables_depth1600_200k_x_1024.json 2>> $OUT/r06_bench_default.err
fi
bash tools/sanitize.sh gpu $OUT/r06_sanitize_asan_ubsan_gpu.log > /dev/null 2>&1
bash tools/sanitize.sh tsan $OUT/r06_sanitize_tsan.log > /dev/null 2>&1
tail -4 $OUT/r06_sanitize_asan_ubsan_gpu.log; tail -4 $OUT/r06_sanitize_tsan.log
python - $OUT <<'PY'
import json, sys
for f in ("r06_multi_n1.json","r06_multi_n2_same_gpu.json"):
    j=json.load(open(sys.argv[1] + "/" + f)); print(f, j["ms_per_step"], j["devices"])
j=json.load(open(sys.argv[1] + "/r06_bench_default.json")); print(j["ms_per_step"], j["roofline"]["frac"], j["h2d"].get("r_entry"), j["h2d"]["pageable"], {k: v for k, v in j["extra"]["workflow"].items() if k.endswith("_ms") or k in ("choice_checksum_rank0", "reference_sets_form")})
PY
