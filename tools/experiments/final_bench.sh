# usage: tools/experiments/final_bench.sh OUT_DIR   (the -m gpu suite, then the --full bench line -> OUT_DIR/bench_final.json)
O=${1:?usage: tools/experiments/final_bench.sh OUT_DIR}
mkdir -p "$O"
python -m pytest tests -m gpu -x -q 2>&1 | tail -3
python bench.py --full 2>/dev/null | grep "^{" > "$O/bench_final.json"
python - "$O/bench_final.json" <<PY
import json, sys
d=json.load(open(sys.argv[1]))
print(d["value"], d["roofline"]["frac"], d["t100"]["shapes_per_s"], d["t100"]["wall_shapes_per_s"], d["train_iteration"]["ms"], d["train_iteration"]["stage1"]["ms"], d["train_iteration"]["stage1"]["encoder_bf16_ms"])
PY
