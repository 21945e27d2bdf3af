#!/bin/bash
# Same-box A/B of the plain bench line: bench.py --gpus 1 --steps 200 --warmup 20
# against a parent build and a new build of libsstgpu.so (SST_LIBRARY),
# alternating parent / new over ROUNDS rounds, then the verdict: the new build
# counts as a gain only if it is below the parent in every round and the
# median difference exceeds the parent's own max - min over its rounds.
# usage: [OUT=dir] tools/ab_plain.sh ROUNDS parent.so new.so [TAG]   (output under $OUT, default bench_out/)
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
R=$1; PARENT=$2; NEW=$3; TAG=${4:-abp}
for r in $(seq 1 $R); do
  for v in parent new; do
    lib=$PARENT; [ $v = new ] && lib=$NEW
    out=$OUT/${TAG}_${v}_$r
    SST_LIBRARY=$PWD/$lib timeout -k 10 240 python3 bench.py --gpus 1 --steps 200 --warmup 20 > $out.json 2> $out.err
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v round $r rc=$rc"; tail -3 $out.err; exit $rc; fi
    python3 -c "import json,sys; d=json.loads(open('$out.json').read().strip().splitlines()[-1]); print('$v', $r, round(d['ms_per_step']*1e3,2), 'us/step')"
  done
done
python3 - $R $TAG $OUT <<'PY'
import json, statistics, sys
R, tag, out = int(sys.argv[1]), sys.argv[2], sys.argv[3]
us = {v: [json.loads(open(f"{out}/{tag}_{v}_{r}.json").read().strip().splitlines()[-1])["ms_per_step"] * 1e3
          for r in range(1, R + 1)] for v in ("parent", "new")}
diff = [p - n for p, n in zip(us["parent"], us["new"])]
spread = max(us["parent"]) - min(us["parent"])
res = {"rounds": R, "parent_us": us["parent"], "new_us": us["new"], "median_parent_us": statistics.median(us["parent"]),
       "median_new_us": statistics.median(us["new"]), "median_diff_us": statistics.median(diff),
       "parent_spread_us": spread, "new_below_parent_every_round": all(d > 0 for d in diff)}
res["gain"] = bool(res["new_below_parent_every_round"] and res["median_diff_us"] > spread)
json.dump(res, open(f"{out}/{tag}_verdict.json", "w"), indent=1)
print(json.dumps(res))
PY
