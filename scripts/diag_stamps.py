"""Phase timeline of one decode launch from a MH_DIAG_STAMPS=1 build (GPU, diagnostic).

    MH_LIB=ab/lib_diag.so python scripts/diag_stamps.py [--batch N]

Stamps (s_memrealtime, 100 MHz) per wave: 0 entry, 1 first header resolved,
2 LUT ready, 3 first span staged, 4 first tile decoded (stores issued),
5 loop done, 6 stores drained.

--launches N stamps the last of N back-to-back launches, each on a frame set of its own
(with --cold: all of them never decoded before, the flush in front of the first).
--rows (MH_DIAG_ROWS build, small launches): core clocks of each of the 8 block rows of
the chain, from the s_memtime stamps behind every row store. A single frame with mid-block
marks takes mh_decode_frame_marked_kernel, whose lanes run 4 rows (32 steps) each: the same slots,
rows 0-3 only. --no-marks drops the marks (mh_decode_frame_kernel in the same library).
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import metalhuffman_amd as mh  # noqa: E402
from metalhuffman_amd import _native as N, decoder as D, frames as F  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--tag", default="")
ap.add_argument("--clock", action="store_true",
                help="MH_DIAG_CLOCK build: slot 5 holds the decode's core-clock cycles (s_memtime)")
ap.add_argument("--args", action="store_true",
                help="MH_DIAG_ARGS build (small launches): slot 5 is stamped once the output arguments are in registers")
ap.add_argument("--tile8192", action="store_true", help="config 3: one 8192x8192 BigBridge mirror tile")
ap.add_argument("--random8192", action="store_true",
                help="config 3 stress: one 8192x8192 uniform-random frame (flat 8-bit table: the flat8 loop; "
                     "stamps 2 and 3 = 1, stamp 4 = first tile's codes landed and stores issued)")
ap.add_argument("--cold", action="store_true",
                help="stamp a launch of a second, never-decoded frame set after a 1 GiB cache flush (bench.py's cold rule)")
ap.add_argument("--launches", type=int, default=1,
                help="stamp the last of this many back-to-back launches, each on its own frame set")
ap.add_argument("--rows", action="store_true",
                help="MH_DIAG_ROWS build: core clocks per block row of the single-frame chain")
ap.add_argument("--no-marks", action="store_true", help="decode without the frames' mid-block marks")
args = ap.parse_args()

lib = N.lib()
if not hasattr(lib, "mh_diag_stamps"):
    sys.exit("not a MH_DIAG_STAMPS build (set MH_LIB)")
bb = F.bigbridge()
if args.random8192:
    efs = [mh.encode_frame(F.uniform_random(8192, 8192, 1234))]
    efs2 = [mh.encode_frame(F.block_shuffle(F.uniform_random(8192, 8192, 1234), 100))] if args.cold else efs
elif args.tile8192:
    base = F.mirror_tile(bb, 8192, 8192)
    efs = [mh.encode_frame(base)]
    efs2 = [mh.encode_frame(F.block_shuffle(base, 100))] if args.cold else efs
else:
    efs = [mh.encode_frame(F.block_shuffle(bb, i) if i else bb) for i in range(args.batch)]
    efs2 = ([mh.encode_frame(F.block_shuffle(bb, 1000 + i)) for i in range(args.batch)] if args.cold else efs)
# the frame sets of the launches in front of the stamped one (fresh ones when cold)
sets_before = []
for k in range(1, args.launches):
    if args.cold and not (args.random8192 or args.tile8192):
        sets_before.append([mh.encode_frame(F.block_shuffle(bb, 1000 + 100 * k + i)) for i in range(args.batch)])
    else:
        sets_before.append(efs)
t1, t2 = efs[0].tables()
tabs = D.DeviceTables.upload(t1, t2, "cuda")
def pack(e):
    f = D.DeviceFrames.pack(e, "cuda")
    if args.no_marks:
        f.mid_marks = None
    return f


fr, fr2 = pack(efs), pack(efs2)
frs_before = [pack(e) for e in sets_before]
# a lane's chain: 4 rows from a mark in the marked single-frame kernel, else the block's 8
chain_rows = 4 if (fr2.mid_marks is not None and fr2.n_frames == 1 and N.has_mid_marks()) else 8
out = D.decode(fr, tabs)
out2 = torch.empty_like(out)
outs_before = [torch.empty_like(out) for _ in frs_before]
for _ in range(args.reps):
    D.decode(fr, tabs, out)
if args.cold:  # evict the Infinity Cache and L2s; the stamped launch decodes frames nothing touched yet
    fa = torch.empty(512 << 20, dtype=torch.uint8, device="cuda").fill_(1)
    torch.empty_like(fa).copy_(fa)
    del fa
torch.cuda.synchronize()
s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for f_, o_ in zip(frs_before, outs_before):
    D.decode(f_, tabs, o_)
s0.record()
D.decode(fr2, tabs, out2)
s1.record()
torch.cuda.synchronize()
n = 8192 * 8
buf = (ctypes.c_ulonglong * n)()
assert lib.mh_diag_stamps(buf, ctypes.c_size_t(n)) == n
st = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8)
live = st[:, 0] > 0
st = st[live]
t0 = st[:, 0].min()
print(f"launch event time {s0.elapsed_time(s1) * 1e3:.2f} us; waves {live.sum()}")
if args.clock:  # slot 5 = s_memtime cycles between stamps 3 and 4 (staged tiles only)
    cyc = st[:, 5].astype(np.int64)
    us = (st[:, 4].astype(np.int64) - st[:, 3].astype(np.int64)) * 0.01
    ok = (cyc > 0) & (us > 0)
    mhz = cyc[ok] / us[ok]
    print(f"decode core cycles p50 {np.median(cyc[ok]):.0f} p90 {np.percentile(cyc[ok], 90):.0f}; "
          f"per symbol p50 {np.median(cyc[ok]) / (8 * chain_rows):.1f}; clock MHz p10 {np.percentile(mhz, 10):.0f} "
          f"p50 {np.median(mhz):.0f} p90 {np.percentile(mhz, 90):.0f}")
    st[:, 5] = st[:, 4]
if args.args:  # slot 5 = the small-launch kernels' output arguments in registers (behind stamp 2)
    d = (st[:, 5].astype(np.int64) - st[:, 2].astype(np.int64)) * 0.01
    print(f"lut->out args p50 {np.median(d):7.2f}  p90 {np.percentile(d, 90):7.2f}  max {d.max():7.2f}")
    st[:, 5] = st[:, 4]
if args.rows:  # lanes 0-7: s_memtime (low word) behind each row's store; lane 8: at the chain's entry
    if not hasattr(lib, "mh_diag_rows"):
        sys.exit("not a MH_DIAG_ROWS build")
    rb = (ctypes.c_uint32 * (8192 * 16))()
    assert lib.mh_diag_rows(rb, ctypes.c_size_t(8192 * 16)) == 8192 * 16
    rw = np.frombuffer(rb, dtype=np.uint32).reshape(-1, 16)[live].astype(np.int64)
    rw = rw[rw[:, 8] != 0]
    edges = np.concatenate([rw[:, 8:9], rw[:, :chain_rows]], axis=1)
    per_row = np.diff(edges, axis=1) & 0xFFFFFFFF
    print(f"row clocks ({len(rw)} waves, {chain_rows} rows per lane), cycles per symbol (8 symbols per row):")
    for r in range(chain_rows):
        v = per_row[:, r] / 8.0
        print(f"  row {r}: p10 {np.percentile(v, 10):6.1f}  p50 {np.median(v):6.1f}  p90 {np.percentile(v, 90):6.1f}  "
              f"mean {v.mean():6.1f}")
    tot = per_row.sum(axis=1) / (8.0 * chain_rows)
    print(f"  all rows: p50 {np.median(tot):6.1f}  mean {tot.mean():6.1f} cycles per symbol")
names = ["entry", "hdr", "lut", "staged", "tile0", "loop", "drain"]
for i, nm in enumerate(names):
    v = (st[:, i].astype(np.int64) - int(t0)) * 0.01
    print(f"{nm:7s} us  min {v.min():7.2f}  p50 {np.median(v):7.2f}  p90 {np.percentile(v, 90):7.2f}  max {v.max():7.2f}")
loop_end = (st[:, 5].astype(np.int64) - int(t0)) * 0.01
print("loop end per wave: p10 %.2f p50 %.2f p90 %.2f p99 %.2f max %.2f us" % tuple(np.percentile(loop_end, [10, 50, 90, 99, 100])))
for a, b in [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6)]:
    d = (st[:, b].astype(np.int64) - st[:, a].astype(np.int64)) * 0.01
    print(f"{names[a]}->{names[b]:7s} p50 {np.median(d):7.2f}  p90 {np.percentile(d, 90):7.2f}  max {d.max():7.2f}")
# start / steady / drain: until the median wave has its first span staged; from then
# until the first 10 % of waves have finished their last tile; from then to the last drain
T = lambda i: (st[:, i].astype(np.int64) - int(t0)) * 0.01
start, fin10, end = float(np.median(T(3))), float(np.percentile(T(5), 10)), float(T(6).max())
print(f"decomposition: start {start:.2f} us, steady {fin10 - start:.2f} us, drain {end - fin10:.2f} us "
      f"(end {end:.2f} us)")
if args.launches > 1:
    args.tag += f"_l{args.launches}"
out_npz = os.path.join(ROOT, "gpurun_out", f"stamps_b{args.batch}{args.tag}{'_cold' if args.cold else ''}.npz")
os.makedirs(os.path.dirname(out_npz), exist_ok=True)
np.savez(out_npz, stamps=np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8))
