# A/B of frames in flight for plain C2 frames at 32 hardware queues (headline and its tiled form
# at one rank).  Logs go to $OUT (default build/ab).
set -e
OUT=${OUT:-build/ab}
mkdir -p "$OUT"
: > "$OUT/ab_inflight_q32.log"
for rep in 1 2; do
  for n in 4 6 8; do
    timeout -k 10 200 python bench.py --full --no-cpu --tiled-frames 0 --extra-frames 0 --inflight $n > "$OUT/b_if$n.log" 2>&1
    echo "inflight=$n $(grep '^{' "$OUT/b_if$n.log" | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], d['ms_per_step'], d['tiled_1gpu']['ms_per_step'])")" >> "$OUT/ab_inflight_q32.log"
  done
done
cat "$OUT/ab_inflight_q32.log"
