# GPU box: the whole GPU suite, the full bench line, the attack loops and their kernel statistics, into <out>/final_*.
out=${1:?usage: tools/final_refresh.sh <output folder>}
mkdir -p "$out" || exit 1
set -x
python -m pytest tests -m gpu -x -q > "$out/final_tests.log" 2>&1; rc=$?; tail -3 "$out/final_tests.log"
[ $rc -eq 0 ] || exit $rc
python bench.py --full > "$out/final_bench.json" 2> "$out/final_bench.err" || exit 1
tail -c 600 "$out/final_bench.json"
python tools/bench_attacks.py geoa3 knn cw_curvenet geoa3_curvenet > "$out/final_attacks.log" 2>&1 || exit 1
tail -1 "$out/final_attacks.log"
for v in geoa3 knn cw_curvenet; do
  bash tools/prof_attack.sh $v > "$out/final_pa_$v.txt" 2>&1 || exit 1
  head -3 "$out/final_pa_$v.txt"
done
