# GPU round check: parity tests, smoke, bench, then rocprofv3 kernel traces of the
# bench command per workload (fail-fast).
set -o pipefail
cd "$(dirname "$0")/.."
export OUT_DIR=$(realpath -m "${OUT_DIR:-bench_out}"); mkdir -p $OUT_DIR
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT_DIR/pytest_gpu.log 2>&1 || { tail -30 $OUT_DIR/pytest_gpu.log; exit 1; }
tail -1 $OUT_DIR/pytest_gpu.log; grep -c PASSED $OUT_DIR/pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT_DIR/smoke.log 2>&1 || { cat $OUT_DIR/smoke.log; exit 1; }
echo "smoke ok"
timeout -k 10 600 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT_DIR/bench.json 2> $OUT_DIR/bench.err || { tail $OUT_DIR/bench.err; exit 1; }
cat $OUT_DIR/bench.json
: > $OUT_DIR/ktrace_summary.txt
# same steps / warm-up as the bench line each number is compared with (the frame
# headline: 200 / 20; the extras: bench.py's own counts)
for spec in frame:20:5 batch:256:256 tile8192:512:512 tile8192_random:512:512; do
  IFS=: read wl k w <<< "$spec"
  rm -rf $OUT_DIR/prof_$wl
  timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof_$wl -o run -- python3 bench.py --workload $wl --steps $k --warmup $w --full --no-extras --no-cpu-baseline > $OUT_DIR/bench_prof_$wl.json 2> $OUT_DIR/bench_prof_$wl.err || { tail $OUT_DIR/bench_prof_$wl.err; exit 1; }
  u=$(python3 -c "import json;print(json.load(open('$OUT_DIR/bench_prof_$wl.json'))['roofline'].get('kernel_us_steady_unit') or 1)")
  { echo "== bench.py --workload $wl --steps $k --warmup $w (profiled line: roofline.kernel_us_avg $(python3 -c "import json;print(json.load(open('$OUT_DIR/bench_prof_$wl.json'))['roofline']['kernel_us_avg'])"), steady unit $u)"; python3 scripts/ktrace_summary.py $OUT_DIR/prof_$wl $k $u; } >> $OUT_DIR/ktrace_summary.txt
done
cat $OUT_DIR/ktrace_summary.txt
# producer side: the GPU encoder (async, back to back) and the device-only chain
rm -rf $OUT_DIR/prof_encode
timeout -k 10 120 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof_encode -o run -- python3 scripts/enc_profile.py 64 > $OUT_DIR/enc_profile.log 2>&1 || { tail $OUT_DIR/enc_profile.log; exit 1; }
timeout -k 10 60 ./host/mh_decode_host device 2048 1536 200 > $OUT_DIR/device_chain.log 2>&1 || { cat $OUT_DIR/device_chain.log; exit 1; }
python3 - > $OUT_DIR/encoder_ktrace.txt <<'PY'
import csv, os
O = os.environ["OUT_DIR"]
print([l for l in open(O + "/enc_profile.log") if "async encode" in l][-1].strip())
print(open(O + "/device_chain.log").read().strip())
for r in sorted(csv.DictReader(open(O + "/prof_encode/run_kernel_stats.csv")), key=lambda r: -float(r["AverageNs"])):
    print(f"{float(r['AverageNs']) / 1e3:8.2f} us  x{r['Calls']:>4}  {r['Name'][:80]}")
PY
cat $OUT_DIR/encoder_ktrace.txt
