# Single-frame kernel A/B: the default library vs ab/lib_$V.so (MH_LIB), interleaved, driver-shaped
# bench (20 steps) -> $OUT_DIR/frame_ab_$V.txt.   V=tlbpf [REPS=3] bash scripts/gpu_frame_ab.sh
# (ab/lib_$V.so from build.build_variant; another commit's kernel: decode_src=<its mh_decode.hip>)
set -o pipefail
cd "$(dirname "$0")/.."
export OUT_DIR=$(realpath -m "${OUT_DIR:-bench_out}"); mkdir -p $OUT_DIR
OUT=$OUT_DIR/frame_ab_$V.txt
: > $OUT
for rep in $(seq 1 ${REPS:-3}); do
  for lib in default $V; do
    E=(X=1); [ $lib != default ] && E=(MH_LIB=$PWD/ab/lib_$lib.so)
    env "${E[@]}" timeout -k 10 120 python bench.py --steps 20 --warmup 5 --full --no-extras --no-cpu-baseline > $OUT_DIR/fab.json 2> $OUT_DIR/fab_err.txt || { tail $OUT_DIR/fab_err.txt; exit 1; }
    python3 -c "import json; d=json.load(open('$OUT_DIR/fab.json')); r=d['roofline']; print('rep $rep $lib', d['value'], 'warm', d.get('warm_value'), 'kernel_us', r['kernel_us_avg'], 'verified', d['frames_verified'])" >> $OUT
  done
done
cat $OUT
