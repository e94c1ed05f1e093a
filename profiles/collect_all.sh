#!/bin/bash
# One round's profiles of the final build, from any directory:   bash profiles/collect_all.sh <tag>
# The full bench line, collect.sh (kernel stats + PMC traffic) of random64 / text64, PMC traffic of the other workloads,
# collect_sq.sh of random64 / text64 and the two-rank rehearsal; everything lands in $PROFILE_OUT (default:
# profile_out/ in the repository root) — copy the summaries into profiles/.
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd "$ROOT"
TAG=${1:-r04_h}
export PROFILE_OUT=$(realpath -m "${PROFILE_OUT:-profile_out}")
RES=$PROFILE_OUT
mkdir -p "$RES"
python3 bench.py --full > "$RES/${TAG}_bench_default.json" 2> "$RES/${TAG}_bench_default.err"; echo "[all] bench rc=$?"
for wl in random64 text64; do bash profiles/collect.sh $TAG $wl > "$RES/${TAG}_collect_$wl.log" 2>&1; echo "[all] collect $wl rc=$?"; done
for wl in batch1m lowent256 lowent64 zlibtext64; do
  OUT=$RES/prof_${TAG}_$wl; mkdir -p "$OUT"
  ( cd "${TMPDIR:-/tmp}" && rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/fetch" -o fetch -- python3 "$ROOT/bench.py" --full --steps 2 --warmup 0 --no-cpu-baseline --workload $wl > "$OUT/fetch.log" 2>&1 && rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/write" -o write -- python3 "$ROOT/bench.py" --full --steps 2 --warmup 0 --no-cpu-baseline --workload $wl > "$OUT/write.log" 2>&1 )
  python3 profiles/summarize.py "$OUT" $TAG $wl; echo "[all] pmc $wl done"
done
for wl in random64 text64; do bash profiles/collect_sq.sh $TAG $wl > "$RES/${TAG}_sq_$wl.log" 2>&1; echo "[all] sq $wl rc=$?"; done
ZES_BENCH_BACKEND=gloo python3 bench.py --gpus 2 --steps 3 --warmup 1 --full --no-cpu-baseline > "$RES/${TAG}_bench_two_ranks_gloo_rehearsal.json" 2>/dev/null; echo "[all] two ranks rc=$?"
