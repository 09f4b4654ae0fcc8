set -e
export TMPDIR=/tmp
OUT=${OUT:-out/split_prof}
mkdir -p "$OUT"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/dd_split" -o run -- python3 bench.py --full --workload c4 --rows 125000000 --steps 5 --warmup 1 --no-cpu --c4-cols 8,9,13,14 --dict-split > "$OUT/dd_split.json" 2> "$OUT/dd_split.err"
echo "== dd split"; python3 tools/kstats.py "$OUT/dd_split"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/c2_split" -o run -- python3 bench.py --full --no-cpu --steps 10 --dict-split > "$OUT/c2_split.json" 2> "$OUT/c2_split.err"
echo "== c2 split"; python3 tools/kstats.py "$OUT/c2_split"
