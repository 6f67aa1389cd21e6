# Usage: tools/gpu/bench_full.sh [OUT [bench.py args]]  -> OUT.json (the --full line), OUT.err; OUT defaults to build/bench_full
cd "$(dirname "$0")/../.."
out=${1:-build/bench_full}
mkdir -p "$(dirname "$out")"
python bench.py --full ${@:2} > $out.json 2> $out.err; echo "rc $?"; tail -3 $out.err
python - <<P
import json
d=json.load(open("$out.json"))
print("main", d["value"], d["t_primal_ms"], d["t_adjoint_ms"], d["t_grad_reduce_ms"], "frac", d["roofline"]["frac"], "cpu", (d.get("cpu_baseline") or {}).get("value"))
for k,v in (d["other_configs"] or {}).items():
    extra = {kk: vv.get("value") for kk, vv in v.items() if isinstance(vv, dict) and "value" in vv}
    print(k, v.get("value"), v.get("unit"), v.get("t_primal_ms"), v.get("t_adjoint_ms"), v.get("t_grad_reduce_ms"), (v.get("roofline") or {}).get("frac"), v.get("error"), extra)
P
