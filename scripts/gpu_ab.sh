# A/B the experiment builds in ab on the batch + frame workloads.
set -o pipefail
cd "$(dirname "$0")/.."
export OUT_DIR=$(realpath -m "${OUT_DIR:-bench_out}"); mkdir -p $OUT_DIR
OUT=$OUT_DIR/ab.txt
: > $OUT
for v in ${VARIANTS:-default $(ls ab | sed 's/^lib_//; s/\.so$//')}; do
  lib=$v; extra=""
  if [ "$lib" = default ]; then unset MH_LIB; else export MH_LIB=$PWD/ab/lib_$lib.so; fi
  for wl in ${WLS:-batch frame}; do
    r=$(timeout -k 10 300 python bench.py --workload $wl --steps ${STEPS:-50} --warmup 5 --full --no-extras --no-cpu-baseline $extra 2>>$OUT_DIR/ab.err) || { echo "$v $wl FAILED" >> $OUT; exit 1; }
    echo "$v $wl $r" | python -c "import sys,json; l=sys.stdin.read().split(' ',2); d=json.loads(l[2]); print(l[0], l[1], 'value', d['value'], 'kernel_us', d['roofline']['kernel_us_avg'], 'frac', d['roofline']['frac'])" >> $OUT
  done
done
cat $OUT
