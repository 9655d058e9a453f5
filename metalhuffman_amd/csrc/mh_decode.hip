// mh_decode.hip -- CDNA4 (gfx950) Huffman block decoder.
//
// Replaces the reference's per-frame GPU work (Shared/AAPLShaders.metal:127-518 driven
// by Shared/AAPLRenderer.m:1178-1678: 4 x huffFragmentShaderB8W12 + 1 x
// huffFragmentShaderB8W16 render passes, a 16-slice blit and the
// cropAndGrayscaleFromTexturesFragmentShader reorder) with ONE kernel launch that
// writes the W x H 8-bit raster directly.
//
// Work decomposition:
//   * a wavefront owns a "tile" = 64 consecutive 8x8 blocks (one lane per block,
//     block order by*bw + bx as in AAPLShaders.metal:309). For a 2048-wide frame a
//     tile is a 512 x 8 pixel strip whose code bits are one contiguous byte span;
//   * the span is staged into the wave's LDS window with coalesced 16-byte buffer
//     loads, byte-swapped once so the bit cursor reads big-endian dwords;
//   * the lookup table lives in LDS, shared by the workgroup: a 2^13-entry first
//     level and a small second level for the (rare) codes of 14-16 bits. For every
//     16-bit window it returns exactly the {symbol, bitWidth} the reference's T1/T2
//     pair returns (AAPLShaders.metal:159-170), invalid windows included;
//   * each lane runs the 64 serial decode steps of its block from a 64-bit bit
//     window (one LDS word read per two symbols), folds the per-block delta
//     (AAPLShaders.metal:260-262) and stores each finished 8-pixel block row as one
//     8-byte store: the 64 lanes of a wave write 512 contiguous bytes per row.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <stdint.h>

#include <atomic>
#include <cmath>
#include <mutex>

#include "../../include/metalhuffman.h"
#include "mh_box.hpp"
#include "mh_lut.hpp"

namespace {

#ifndef MH_DIAG_STAMPS          // diagnostic builds only: per-wave phase timestamps
#define MH_DIAG_STAMPS 0        //    (scripts/diag_stamps.py)
#endif
#ifndef MH_DIAG_CLOCK           // diagnostic builds only: core-clock cycles of the single-frame
#define MH_DIAG_CLOCK 0         //    decode in stamp slot 5 (scripts/diag_stamps.py --clock)
#endif
#ifndef MH_DIAG_ARGS            // diagnostic builds only: small-launch kernels stamp slot 5 once their
#define MH_DIAG_ARGS 0          //    output arguments are in registers (scripts/diag_stamps.py --args)
#endif
#ifndef MH_DIAG_DROP_STORES     // diagnostic builds only: every row store out of range (dropped)
#define MH_DIAG_DROP_STORES 0
#endif
#ifndef MH_DIAG_ROWS            // diagnostic builds only: core-clock stamps at every row boundary of the
#define MH_DIAG_ROWS 0          //    small-launch kernels' staged decode (scripts/diag_stamps.py --rows)
#endif
#if MH_DIAG_ROWS && !MH_DIAG_STAMPS
#error "MH_DIAG_ROWS is a mode of the MH_DIAG_STAMPS build"
#endif
#ifndef MH_LANE_PAIRS           // 1: the lane-pair diagnostic library only (libmh_diag_lanepairs.so,
#define MH_LANE_PAIRS 0         //    metalhuffman_amd/build.py), which exports mh_diag_decode_lanepairs
#endif
#ifndef MH_LAZY_ROWS_PER_ITER   // A/B builds: 1, 2 or 8 (8: the chain fully unrolled, as before the row loop)
#define MH_LAZY_ROWS_PER_ITER 4
#endif
constexpr int kLazyRowsPerIter = MH_LAZY_ROWS_PER_ITER;  // rows per trip of the small-launch chain's row loop
static_assert(kLazyRowsPerIter == 1 || kLazyRowsPerIter == 2 || kLazyRowsPerIter == 4 || kLazyRowsPerIter == 8,
              "a block's 8 rows in whole trips");
constexpr int kStageBytes = 4352;             // per-wave LDS window (max tile span)
constexpr int kMaxWavesPerWG = 8;             // batch kernel workgroup width
constexpr int kMinWavesPerEU = 6;             // register cap: 6 waves/SIMD = what the LDS budget admits
// Row-store cache bits (gfx950 aux field: 1 sc0, 2 nt, 16 sc1). Batch kernel: nt.
// Small-launch kernel: nt sc1, write-through, so nothing dirty is left in the XCDs'
// L2s for the end-of-kernel release to write back (profiles/r03_v5_store_write_through_ab.txt;
// both re-checked cold in round 5: profiles/r05_batch_store_policy_ab.txt, r05_small_store_policy_ab.txt).
constexpr int kBatchStoreAux = 2;
constexpr int kSmallStoreAux = 18;
static_assert(kStageBytes % 16 == 0, "stage uses 16-byte chunks");

typedef unsigned int v4u32 __attribute__((ext_vector_type(4)));

struct DecodeArgs {
  const uint32_t *offsets;     // frame f's block offsets at offsets + f*nb
  const uint8_t *codes;
  const uint64_t *frame_off;   // n_frames+1 entries, or null
  uint64_t codes_bytes;
  const uint16_t *t1;          // HuffLookupSymbol viewed as u16 = symbol | bitWidth << 8
  const uint16_t *t2;
  const uint16_t *lut;         // prepared L1+L2 table or null
  const uint8_t *block_init;
  uint8_t *out;
  uint64_t out_pitch;
  uint64_t out_frame_stride;
  uint64_t out_frame_bytes;    // H * pitch
  uint32_t t2_entries;
  uint32_t w, h, bw, bh, nb;
  uint32_t tiles_per_frame, total_tiles;
  uint32_t n_groups;           // ceil(total_tiles / waves_per_wg)
  uint32_t nwaves, grid;       // batch kernel launch shape as kernel arguments: blockDim / gridDim
                               // read the dispatch packet's implicit arguments, a dependent
                               // global load at the head of the kernel (code object v5)
};

__device__ __forceinline__ uint32_t bswap32(uint32_t x) {
  return __builtin_amdgcn_perm(0u, x, 0x00010203u);
}

// AAPLShaders.metal:159-170 / HuffmanUtil.cpp:961-995 on a 16-bit pattern.
// Out-of-range T2 reads (corrupt tables only) return the all-zero entry.
__device__ __forceinline__ uint32_t split_lookup(const uint16_t *t1, const uint16_t *t2,
                                                 uint32_t t2_entries, uint32_t pat16) {
  uint32_t e = t1[pat16 >> 8];
  if ((e >> 8) == 0) {
    const uint32_t idx = (e & 0xFFu) * 256u + (pat16 & 0xFFu);
    e = idx < t2_entries ? (uint32_t)t2[idx] : 0u;
  }
  return e;
}


// Builds the two-level table into `lut` (LDS or global) with `nthreads`
// cooperating threads; `p0` is a scratch word shared by them.
//   L1[p] (p = 13-bit prefix): step_word(split_lookup(p << 3)) when that code has
//     <= 13 bits or the window is invalid (0 -> no-op, as the reference's dummy
//     T2 subtable, HuffmanUtil.cpp:550-556); otherwise an escape `sub`.
//     Canonical codes are ordered by length, so every code of 14-16 bits lies at
//     or above the first such code's prefix P0 and the long codes (<= 256 codes
//     of >= 4 patterns) occupy at most 128 prefixes from P0.
//   L2[sub*8 + x] = step_word(split_lookup(((P0 + sub - 1) << 3) | x)), sub >= 1;
//   L2 subtable 0 is all zero (escapes beyond the long-code range: invalid windows).
template <class SyncFn>
__device__ void build_lut(const uint16_t *t1, const uint16_t *t2, uint32_t t2_entries,
                          uint16_t *lut, uint32_t *p0, uint32_t tid, uint32_t nthreads,
                          SyncFn sync) {
  if (tid == 0) *p0 = (uint32_t)kL1Entries;
  sync();
  for (uint32_t p = tid; p < (uint32_t)kL1Entries; p += nthreads) {
    const uint32_t e = split_lookup(t1, t2, t2_entries, p << kL2Bits);
    lut[p] = (uint16_t)step_word(e);
    if ((e >> 8) > (uint32_t)kLutBits) atomicMin(p0, p);
  }
  for (uint32_t i = tid; i < (uint32_t)(kLutEntries - kL1Entries); i += nthreads)
    lut[kL1Entries + i] = 0;
  sync();
  const uint32_t P0 = *p0;
  for (uint32_t p = P0 + tid; p < (uint32_t)kL1Entries; p += nthreads) {
    const uint32_t sub = p - P0 + 1;
    lut[p] = (uint16_t)(sub < (uint32_t)kL2Subtables ? sub : 0u);
  }
  const uint32_t nl2 = ((uint32_t)kL1Entries - P0) << kL2Bits;
  for (uint32_t i = tid; i < nl2 && i < (uint32_t)(kL2Entries - (1 << kL2Bits)); i += nthreads)
    lut[kL1Entries + (1 << kL2Bits) + i] =
        (uint16_t)step_word(split_lookup(t1, t2, t2_entries, (P0 << kL2Bits) + i));
  sync();
}


#if !MH_LANE_PAIRS
// mh_prepare_lut: the prepared tables from T1/T2 in device memory, one workgroup
// (build_prepared_lut, mh_lut.hpp).
__global__ void __launch_bounds__(1024) mh_prepare_lut_kernel(const uint16_t *t1, const uint16_t *t2,
                                                              uint32_t t2_entries, uint8_t *buf) {
  __shared__ uint16_t s_t1[256];
  __shared__ uint32_t s_scratch[4];
  if (threadIdx.x < 256) s_t1[threadIdx.x] = t1[threadIdx.x];
  __syncthreads();
  build_prepared_lut(s_t1, t2, t2_entries, buf, s_scratch);
}
#endif

// Word source for the bit cursor: big-endian dwords of the tile's code span.
struct LdsWords {
  const uint8_t *w;
  __device__ __forceinline__ const uint8_t *at(uint32_t byte_off) const { return w + byte_off; }
};
// Stage swizzle (batch kernel, flat tables only): the eight 16-B chunks of every
// 128-B row of a wave's stage are permuted by the row index (XOR), so lanes whose
// blocks start a multiple of 128 B apart -- flat code lengths make every block
// exactly 64 B -- refill from different LDS banks (b32 reads bank on (a/4) mod 32).
// Chunks stay whole (16-B staging stores) and stay inside their row.
__device__ __forceinline__ uint32_t swz_off(uint32_t o) { return o ^ ((o >> 3) & 0x70u); }

// byte 1 (prev) of four successive lane states -> one output word, 3 VALU
__device__ __forceinline__ uint32_t pack_prev4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const uint32_t lo = __builtin_amdgcn_perm(b, a, 0x0C0C0501u);  // [a.1, b.1, 0, 0]
  const uint32_t hi = __builtin_amdgcn_perm(d, c, 0x05010C0Cu);  // [0, 0, c.1, d.1]
  return lo | hi;
}

// byte 0 of four successive sums -> one output word, 3 VALU
__device__ __forceinline__ uint32_t pack_lo4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
  const uint32_t lo = __builtin_amdgcn_perm(b, a, 0x0C0C0400u);  // [a.0, b.0, 0, 0]
  const uint32_t hi = __builtin_amdgcn_perm(d, c, 0x04000C0Cu);  // [0, 0, c.0, d.0]
  return lo | hi;
}

// v_perm_b32 selectors: put S0.byte1 at byte J, keep S1's other bytes
__device__ __forceinline__ constexpr uint32_t ins_sel1(int j) {
  return j == 0 ? 0x03020105u : j == 1 ? 0x03020500u : j == 2 ? 0x03050100u : 0x05020100u;
}

__shared__ __attribute__((aligned(16))) uint16_t s_lut[kLutEntries];
__shared__ __attribute__((aligned(16))) uint8_t s_stage[kMaxWavesPerWG * kStageBytes];
__shared__ uint32_t s_p0;

#if MH_DIAG_STAMPS
constexpr int kDiagWaves = 8192, kDiagSlots = 8;
__device__ unsigned long long g_stamps[kDiagWaves * kDiagSlots];
#if MH_DIAG_ROWS
// per wave: s_memtime (low word) behind each of the 8 row stores of decode_block, then at its entry
constexpr int kDiagRowSlots = 16;
__device__ uint32_t g_rows[kDiagWaves * kDiagRowSlots];
#endif
#define MH_STAMP(i) (ts[i] = __builtin_amdgcn_s_memrealtime())
#else
#define MH_STAMP(i) ((void)0)
#endif

// Wave priority 0..3 (s_setprio takes an immediate). The SIMD arbiter serves the
// oldest wave first among equal priorities, so waves of later workgroups fall
// behind; the batch loop gives waves with more tiles left a higher priority.
__device__ __forceinline__ void set_prio(uint32_t p) {
  switch (__builtin_amdgcn_readfirstlane(p) & 3u) {
    case 0: __builtin_amdgcn_s_setprio(0); break;
    case 1: __builtin_amdgcn_s_setprio(1); break;
    case 2: __builtin_amdgcn_s_setprio(2); break;
    default: __builtin_amdgcn_s_setprio(3); break;
  }
}

// Lookup flavours of the decode step.
//   Lut13: 2^13-entry first level + escapes to the second level (any code <= 16 bits).
//   Lut14: 2^14-entry single level, no escape test at all; valid when no code is
//          longer than 14 bits (the prepared table records the longest code).
// kMasked: only the lanes that consumed a word read the next one (batch kernel);
//   the small-launch kernel's latency-bound chain reads unmasked.
// kLazy: the refill test runs at every step on the cursor the lookup itself uses, in the
//   lookup's LDS shadow, and takes effect at the next step (the small kernel's step since
//   round 5: profiles/r05_lazy_ab.txt) (sh <= 47 still holds at every
//   lookup: sh >= 32 drops a word, sh < 32 advances by <= 16), so the chain from one
//   lookup to the next is add, shift, and -- no compare / select on it.
template <int kBits, bool kMaskedRefill, bool kEscapes = kBits == kLutBits, bool kSwizzle = false,
          int kStoreAux = kBatchStoreAux, bool kLazyRefill = false, bool kFlat8Bytes = false>
struct StepCfg {
  static constexpr bool kLazy = kLazyRefill;
  static constexpr bool kFlat8 = kFlat8Bytes;  // flat 8-bit canonical table: byte arithmetic
  static constexpr int kAux = kStoreAux;  // row-store cache bits
  static constexpr bool kEsc = kEscapes;
  static constexpr bool kSwz = kSwizzle;
  static constexpr bool kMasked = kMaskedRefill;
  static constexpr uint32_t kCur = 127u - (uint32_t)kBits;   // S low byte = kCur - sh
  static constexpr uint32_t kMask = (2u << kBits) - 2u;       // byte address of a u16 entry
  static constexpr uint32_t kRefillAt = kCur - 32u;           // low byte <= this: sh >= 32
};

using Lut13 = StepCfg<kLutBits, true>;  // the batch kernel's step
// ... and its escape-free twin, for tables whose longest code is <= 13 bits (the
// first level then decodes every window; no per-symbol escape test)
using Lut13NoEsc = StepCfg<kLutBits, true, false>;
// ... and for flat tables (every code the same length, e.g. uniform bytes: every
// block the same size, so lanes sit a multiple of 128 B apart): swizzled stage.
// Escape-free like Lut13NoEsc, so only for a length <= 13 bits: the sampled
// longest == shortest also holds for {14: n}, {15: n}, {16: n} and {15: 1, 16: 2},
// whose codes all live in the second level (the general step)
using Lut13Flat = StepCfg<kLutBits, true, false, true>;

#if MH_DIAG_ROWS  // lane r of *rowv: the core clock behind row r's store; lane 8: at the chain's entry
#define MH_ROWS_PARAM , uint32_t *rowv = nullptr
#define MH_ROWS_NONE , nullptr  // a caller that names the output stage behind it
#define MH_ROW_STAMP(r) \
  if (rowv) *rowv = (threadIdx.x & 63u) == (r) ? (uint32_t)__builtin_amdgcn_s_memtime() : *rowv
#else
#define MH_ROWS_PARAM
#define MH_ROWS_NONE
#define MH_ROW_STAMP(r) ((void)0)
#endif

// The output stage of a block row. decode_block and flat8_block finish every row of a block as
// two packed words (byte i of o0 = pixel i, of o1 = pixel 4 + i); what becomes of them is a policy.
//   StoreRows, the default: one 8-byte store per row at `off` -- a frame's or a region's raster.
//   BoxRows<k> (mh_decode_region_scaled, k = 1..3): the block's s x s cells, s = 2^k, averaged
//     over their IN-FRAME pixels, c = 8 >> k bytes per output row in one b32 / b16 / b8 store at
//     rbase + (r >> k) * pitch (the lanes of a wave write 64 c contiguous bytes).
//     Straight-line code, no branch and no select inside the decode chain: the chain leaves no
//     SGPRs for either (every live comparison result is a pair of them; a wave-uniform "edge
//     tile" branch per row or per rounding point cost the kernels 5 to 27 SGPR spills).
//     Columns: each word passes a v_perm_b32 whose per-lane selectors (sel0 / sel1, once per
//       tile) turn the bytes outside the frame into 0 -- all identity but in the frame's
//       right-edge block. Rows: a row at or below the frame's bottom takes the all-zero selector
//       (a scalar select and v_max_u32: identity selectors are below 0x0C0C0C0C as words).
//     Sums: s = 2 keeps SWAR 16-bit pair sums, s = 4 and 8 a byte sum per word (v_sad_u8 against 0).
//     Rounding, s = 2: a cell has 4, 2, 1 or 0 pixels, and the mean of 2 (1) pixels is the mean of
//       the 4 with each counted twice (four times). So the selectors REPLICATE a lone last
//       column into its neighbour, a lone last row is doubled by a scalar shift, and every cell
//       rounds by (sum + 2) >> 2 -- exact, no division.
//     Rounding, s = 4 and 8: a cell has n = nw * nh pixels, any of 0..s^2, and takes
//       mh_box_round (mh_box.hpp; a 24-bit division, 2 and 1 per output row); nw is counted from
//       the selectors, nh is scalar. n = 0 -- a cell wholly outside the frame -- gives byte 0.
//     Dead lanes and rows >= SH store outside the descriptor as everywhere (OutTile).
typedef unsigned int v2u32_t __attribute__((ext_vector_type(2)));
struct StoreRows {
  static constexpr int kLog2 = 0;
  static constexpr bool kCrop = false;
  static constexpr bool kNorm = false;
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t, uint32_t o0, uint32_t o1, uint32_t off,
                                      uint32_t, uint32_t) {
    v2u32_t v;
    v.x = o0;
    v.y = o1;
    __builtin_amdgcn_raw_buffer_store_b64(v, out, (int)off, 0, kAux);
  }
  // (the byte loops hold the row as a vector already)
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t, v2u32_t v, uint32_t off, uint32_t,
                                      uint32_t) {
    __builtin_amdgcn_raw_buffer_store_b64(v, out, (int)off, 0, kAux);
  }
};

template <int kLog2_>
struct BoxRows {
  static constexpr int kLog2 = kLog2_;
  static constexpr bool kCrop = false;
  static constexpr bool kNorm = false;
  static_assert(kLog2 >= 1 && kLog2 <= 3, "cells of 2, 4 or 8 pixels");
  static constexpr uint32_t kZeroSel = 0x0C0C0C0Cu;  // v_perm_b32: every byte the constant 0
  uint32_t ch;          // in-frame rows of the tile's block row, 1..8 (wave-uniform)
  uint32_t sel0, sel1;  // per lane: byte selectors of o0 / o1 (rows_of)
  uint32_t a0 = 0, a1 = 0;  // k = 1: 16-bit sums of cells 0,1 / 2,3; k = 2: of cell 0 / 1; k = 3: a0 alone
  // in-frame columns among the four of a word, from its selector (0x0C has bit 3, 0..3 have not)
  static __device__ __forceinline__ uint32_t live_cols(uint32_t sel) { return 4u - (uint32_t)__popc(sel & 0x08080808u); }
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t r, uint32_t o0, uint32_t o1, uint32_t,
                                      uint32_t rbase, uint32_t pitch) {
    constexpr uint32_t s = 1u << kLog2;
    const uint32_t dead = r >= ch ? kZeroSel : 0u;  // scalar
    o0 = __builtin_amdgcn_perm(0u, o0, max(sel0, dead));
    o1 = __builtin_amdgcn_perm(0u, o1, max(sel1, dead));
    if constexpr (kLog2 == 1) {
      a0 += (o0 & 0x00FF00FFu) + ((o0 >> 8) & 0x00FF00FFu);
      a1 += (o1 & 0x00FF00FFu) + ((o1 >> 8) & 0x00FF00FFu);
    } else if constexpr (kLog2 == 2) {
      a0 = __builtin_amdgcn_sad_u8(o0, 0u, a0);
      a1 = __builtin_amdgcn_sad_u8(o1, 0u, a1);
    } else {
      a0 = __builtin_amdgcn_sad_u8(o0, 0u, __builtin_amdgcn_sad_u8(o1, 0u, a0));
    }
    // the row is summed HERE, as a store would have consumed it here: left to the scheduler, the
    // sums of a row sink towards the rounding and the rows' symbols stay live (1/8 scale, raw
    // pixels, general step: 80 VGPRs and 12 bytes of scratch)
    if constexpr (kLog2 == 3)
      asm volatile("" : "+v"(a0));
    else
      asm volatile("" : "+v"(a0), "+v"(a1));
    if ((r & (s - 1u)) != s - 1u) return;
    const uint32_t Y = r >> kLog2;
    uint32_t v;
    if constexpr (kLog2 == 1) {
      const uint32_t twice = r == ch ? 1u : 0u;  // scalar: row r - 1 is the frame's last, alone in its cell
      v = __builtin_amdgcn_perm((((a1 << twice) + 0x00020002u) >> 2) & 0x00FF00FFu,
                                (((a0 << twice) + 0x00020002u) >> 2) & 0x00FF00FFu, 0x06040200u);
    } else {
      const uint32_t nh = mh_box_cell_live(ch, Y, kLog2);  // scalar
      if constexpr (kLog2 == 2)
        v = mh_box_round(a0, nh * live_cols(sel0)) | (mh_box_round(a1, nh * live_cols(sel1)) << 8);
      else
        v = mh_box_round(a0, nh * (live_cols(sel0) + live_cols(sel1)));
    }
    const int off = (int)(rbase + Y * pitch);
    if constexpr (kLog2 == 1)
      __builtin_amdgcn_raw_buffer_store_b32(v, out, off, 0, kAux);
    else if constexpr (kLog2 == 2)
      __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, out, off, 0, kAux);
    else
      __builtin_amdgcn_raw_buffer_store_b8((unsigned char)v, out, off, 0, kAux);
    a0 = a1 = 0u;
  }
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t r, v2u32_t v, uint32_t off, uint32_t rbase,
                                      uint32_t pitch) {
    row<kAux>(out, r, v.x, v.y, off, rbase, pitch);
  }
};

// CropRows (mh_decode_crops): the row moved onto the crop's own byte grid. With dx = x0 & 7, output
// word j of a crop row is bytes dx..7 of block j followed by bytes 0..dx-1 of block j + 1: bytes
// dx..dx+7 of the 16 bytes [o0, o1, n0, n1], (n0, n1) the row of the lane to the right. The three
// source words are (A, B, C) = (o0, o1, n0) for dx < 4 and (o1, n0, n1) for dx >= 4, and the output
// is alignbyte(B, A, dx & 3), alignbyte(C, B, dx & 3). The choice is a bit select by a per-lane mask
// `lo` (all ones: dx < 4), not a compare: a compare's result is an SGPR pair, live through the whole
// chain, which has none to spare (BoxRows above). With X = lo ? o0 : o1 and Y = lo ? o1 : o0 the
// neighbour's X and Y are C and, for dx >= 4, B: two DPP moves (wave_shl:1, lane i reads lane
// i + 1; lane 63 reads 0), three v_bfi_b32 and two v_alignbyte_b32 per row, no LDS traffic. Every
// lane runs every row in lock step (decode_block, flat8_block), so the neighbour's row is complete
// when it is read; lane 63 of a tile never stores (out_tile), nor does the last lane of
// decode_halves' first pass. dy and h are not here at all: they are in the tile's descriptor and
// the lane's first offset (out_tile). One aligned 8-byte store per row, as StoreRows.
struct CropRows {
  static constexpr int kLog2 = 0;
  static constexpr bool kCrop = true;
  static constexpr bool kNorm = false;
  uint32_t lo;  // per lane, wave-uniform in value: ~0 for dx < 4, else 0
  uint32_t k;   // per lane: dx & 3
  static __device__ __forceinline__ uint32_t right(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
  }
  static __device__ __forceinline__ uint32_t pick(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t, uint32_t o0, uint32_t o1, uint32_t off,
                                      uint32_t, uint32_t) {
    const uint32_t X = pick(lo, o0, o1), Y = pick(lo, o1, o0);
    const uint32_t nX = right(X), nY = right(Y);
    const uint32_t B = pick(lo, Y, nY);
    v2u32_t v;
    v.x = __builtin_amdgcn_alignbyte(B, X, k);
    v.y = __builtin_amdgcn_alignbyte(nX, B, k);
    __builtin_amdgcn_raw_buffer_store_b64(v, out, (int)off, 0, kAux);
  }
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t r, v2u32_t v, uint32_t off, uint32_t rbase,
                                      uint32_t pitch) {
    row<kAux>(out, r, v.x, v.y, off, rbase, pitch);
  }
};

// NormRows<kFmt> (mh_decode_crops_norm): CropRows' crop-aligned row, optionally mirrored, converted
// to the element T[v] = cvt(fmaf((float)v, scale, bias)) and stored 2 or 4 times as wide. The row's
// two words pass two v_perm_b32 over (v.x, v.y) with a per-lane selector: the identity (0x03020100,
// then 0x07060504) or the byte reversal (0x04050607, then 0x00010203) -- the second selector is the
// first ^ 0x04040404 in both cases, so one register holds the choice and the chain sees no compare.
// A mirrored word j lands at word OW - 1 - j of the row: that, and the element size, are in the
// lane's first offset (out_tile), so `off` is already the row's byte offset in the wide raster.
// scale, bias and the selector are per-lane VGPRs (the chain has no SGPR for them), and they are
// a crop's, not a tile's: the kernel makes them once, ahead of the persistent loop (NormMap).
// Conversion: v_cvt_f32_ubyte*, one fused multiply-add in binary32, then a plain C cast to the
// format (round to nearest even, subnormals kept, overflow to inf). Converted and stored in halves
// -- four elements at a time -- so no more than four floats are live. One unconditional b128 store
// per row for the 16-bit formats, two for binary32.
typedef unsigned int v4u32_t __attribute__((ext_vector_type(4)));
template <uint32_t kFmt>
struct NormRows : CropRows {
  static_assert(kFmt <= MH_NORM_F32, "binary16, bfloat16 or binary32");
  static constexpr bool kNorm = true;
  static constexpr uint32_t kElem = kFmt == MH_NORM_F32 ? 4u : 2u;  // bytes per element
  uint32_t sel;       // per lane: the first word's byte selector
  float scale, bias;  // per lane
  __device__ __forceinline__ float el(uint32_t w, int i) const {
    return __builtin_fmaf((float)((w >> (8 * i)) & 0xFFu), scale, bias);
  }
  // two elements -> one word of the 16-bit format
  static __device__ __forceinline__ uint32_t pack(float a, float b) {
    if constexpr (kFmt == MH_NORM_F16) {
      typedef _Float16 h2 __attribute__((ext_vector_type(2)));
      h2 h;
      h.x = (_Float16)a;
      h.y = (_Float16)b;
      return __builtin_bit_cast(uint32_t, h);
    } else {
      typedef __bf16 b2 __attribute__((ext_vector_type(2)));
      b2 h;
      h.x = (__bf16)a;
      h.y = (__bf16)b;
      return __builtin_bit_cast(uint32_t, h);
    }
  }
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t, uint32_t o0, uint32_t o1, uint32_t off,
                                      uint32_t, uint32_t) {
    const uint32_t X = pick(lo, o0, o1), Y = pick(lo, o1, o0);
    const uint32_t nX = right(X), nY = right(Y);
    const uint32_t B = pick(lo, Y, nY);
    const uint32_t c0 = __builtin_amdgcn_alignbyte(B, X, k), c1 = __builtin_amdgcn_alignbyte(nX, B, k);
    // the second word's selector is the first's ^ 0x04040404, which is the first's with the two
    // sources exchanged: no second selector register
    const uint32_t w0 = __builtin_amdgcn_perm(c1, c0, sel);
    uint32_t w1 = __builtin_amdgcn_perm(c0, c1, sel);
    // converted where the row is stored, a word at a time (as BoxRows sums its rows where a store
    // would have consumed them): left to the scheduler, the rows' floats stay live along the chain
    v4u32_t v;
    if constexpr (kFmt == MH_NORM_F32) {
      // one v_fma_f32 per element, kept apart: packed (v_pk_fma_f32) they take scale and bias as
      // aligned register PAIRS, two more VGPRs than the raw-pixel kernel has
      asm volatile("" : "+v"(w1));
      v.x = __builtin_bit_cast(uint32_t, el(w0, 0));
      asm volatile("" : "+v"(v.x));
      v.y = __builtin_bit_cast(uint32_t, el(w0, 1));
      asm volatile("" : "+v"(v.y));
      v.z = __builtin_bit_cast(uint32_t, el(w0, 2));
      asm volatile("" : "+v"(v.z));
      v.w = __builtin_bit_cast(uint32_t, el(w0, 3));
      __builtin_amdgcn_raw_buffer_store_b128(v, out, (int)off, 0, kAux);
      asm volatile("" : "+v"(w1));
      v.x = __builtin_bit_cast(uint32_t, el(w1, 0));
      asm volatile("" : "+v"(v.x));
      v.y = __builtin_bit_cast(uint32_t, el(w1, 1));
      asm volatile("" : "+v"(v.y));
      v.z = __builtin_bit_cast(uint32_t, el(w1, 2));
      asm volatile("" : "+v"(v.z));
      v.w = __builtin_bit_cast(uint32_t, el(w1, 3));
      __builtin_amdgcn_raw_buffer_store_b128(v, out, (int)(off + 16u), 0, kAux);
    } else {
      v.x = pack(el(w0, 0), el(w0, 1));
      v.y = pack(el(w0, 2), el(w0, 3));
      asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(w1));
      v.z = pack(el(w1, 0), el(w1, 1));
      v.w = pack(el(w1, 2), el(w1, 3));
      __builtin_amdgcn_raw_buffer_store_b128(v, out, (int)off, 0, kAux);
    }
  }
  template <int kAux>
  __device__ __forceinline__ void row(__amdgpu_buffer_rsrc_t out, uint32_t r, v2u32_t v, uint32_t off, uint32_t rbase,
                                      uint32_t pitch) {
    row<kAux>(out, r, v.x, v.y, off, rbase, pitch);
  }
};

// One lane decodes one 8x8 block: 64 serial steps of AAPLShaders.metal:241-268
// (cursor advance + delta fold); each finished 8-pixel block row is stored at once.
//
// Lane state: a 64-bit window hi:lo of big-endian code words, the LDS address
// `wa` of hi in the staged span, the prefetched next word `nw`, and
//   S: bits 0-7 = kCur - sh (sh = bits of hi:lo already consumed, 0..63),
//      bits 8-15 = prev (the running delta sum), bits 16+ = don't care.
// (hi:lo) >> (S & 63) = (hi:lo) >> (kCur - 64 - sh) puts the next kBits code bits
// at bits 1..kBits, i.e. the byte address of their u16 table entry; one add of the
// entry's step word then advances sh and prev together (the low byte stays in
// [kCur - 63, kCur], so it never borrows from prev).
// kRows: the block rows the lane decodes, 8 or -- half a block from a mid-block mark
// (mh_decode_frame_marked_kernel) -- 4: 8 kRows steps from bit p with the running sum `prev`, stored
// as rows 0 .. kRows - 1 from row0 on (the lane of rows 4-7 brings row0 + 4 * pitch).
template <bool kDelta, class Cfg, int kRows = 8, class Src, class Out = StoreRows>
__device__ __forceinline__ void decode_block(const Src &src, const uint8_t *lut, uint32_t p,
                                             uint32_t prev, __amdgpu_buffer_rsrc_t out,
                                             uint32_t row0, uint32_t pitch, bool dead MH_ROWS_PARAM,
                                             Out sink = Out()) {
  if constexpr (Cfg::kFlat8) {
    // 64 one-byte codes from bit p of the staged (big-endian word) span: 17 words, each
    // output word a 64-bit funnel shift (any bit alignment); code c is symbol c
    typedef const __attribute__((address_space(3))) uint32_t *lds_u32;
    typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
    const lds_u32 wp = (lds_u32)(src.w + (p >> 5) * 4u);
    const uint32_t sh = p & 31u;
    uint32_t w[2 * kRows + 1];
#pragma unroll
    for (int j = 0; j < 2 * kRows + 1; ++j) w[j] = wp[j];
    const uint32_t rbase = dead ? 0x80000000u : row0;
    uint32_t s = prev;
#pragma unroll
    for (uint32_t r = 0; r < (uint32_t)kRows; ++r) {
      uint32_t c[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const uint32_t j = 2 * r + h;
        c[h] = (uint32_t)(((((uint64_t)w[j]) << 32 | w[j + 1]) << sh) >> 32);  // big-endian: symbol 4j+i = byte 3-i
      }
      v2u32 v;
      if (kDelta) {
        uint32_t sv[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
          for (int i = 0; i < 4; ++i) sv[i] = s = s + ((c[h] >> (24 - 8 * i)) & 0xFFu);
          const uint32_t o = pack_lo4(sv[0], sv[1], sv[2], sv[3]);
          if (h) v.y = o; else v.x = o;
        }
      } else {
        v.x = bswap32(c[0]);
        v.y = bswap32(c[1]);
      }
      sink.template row<Cfg::kAux>(out, r, v, rbase + r * pitch, rbase, pitch);
    }
    return;
  }
  // wa: LDS address of hi's word in the staged span. An explicit local-address-space
  // pointer keeps its arithmetic 32-bit (a generic pointer was carried as a 64-bit value:
  // one 64-bit add per refill) and lets the reads fold their constant offsets.
  typedef const __attribute__((address_space(3))) uint8_t *lds_u8;
  typedef const __attribute__((address_space(3))) uint32_t *lds_u32;
  const lds_u8 base = (lds_u8)src.w;
  lds_u8 wa = base + (p >> 5) * 4u;
  const auto rd = [&](lds_u8 q) -> uint32_t {
    if constexpr (Cfg::kSwz)
      return *(lds_u32)(base + swz_off((uint32_t)(q - base)));
    else
      return *(lds_u32)q;
  };
  uint32_t S = (prev << 8) + Cfg::kCur - (p & 31u);
  // An odd refill bound (the 14-bit table's) goes in as an opaque scalar: as a literal
  // the compiler rewrites (S & 0xFF) <= K as (S & 0xFE) < K + 1, which no longer folds
  // into a byte-select (SDWA) compare -- one more VALU on every refill step's chain.
  uint32_t kRefill = Cfg::kRefillAt;
  if constexpr ((Cfg::kRefillAt & 1u) != 0u) asm("s_mov_b32 %0, %1" : "=s"(kRefill) : "n"(Cfg::kRefillAt));
  uint32_t hi = rd(wa);
  uint32_t lo = rd(wa + 4);
  uint32_t nw = rd(wa + 8);

  // sh <= 47 at every lookup keeps >= 16 valid window bits.
#define MH_LOOKUP(A1)                                                               \
  uint32_t e = *reinterpret_cast<const uint16_t *>(lut + (A1));
#define MH_FINISH(J, OW)                                                            \
  {                                                                                 \
    if constexpr (Cfg::kEsc) {                                                      \
      const bool esc = e < kEscapeBelow;                                            \
      if (__builtin_expect(__ballot(esc) != 0, 0)) {                                \
        const uint64_t x = (((uint64_t)hi) << 32) | lo;                             \
        const uint32_t x3 = (uint32_t)(x >> ((S - 2u) & 63u)) & 7u;                 \
        const uint32_t e2 = *reinterpret_cast<const uint16_t *>(                    \
            lut + 2u * (kL1Entries + ((e & 0xFFu) << kL2Bits) + x3));               \
        e = esc ? e2 : e;                                                           \
      }                                                                             \
    }                                                                               \
    S += e;                                                                         \
    if (kDelta) {                                                                   \
      sv[J] = S;  /* packed four at a time (pack_prev4) */                         \
    } else {                                                                        \
      OW = __builtin_amdgcn_perm(e + 0xFFu, OW, ins_sel1(J));  /* byte 1: symbol */  \
    }                                                                               \
  }
#define MH_STEP(J, OW)                                                              \
  {                                                                                 \
    const uint64_t x = (((uint64_t)hi) << 32) | lo;                                 \
    MH_LOOKUP((uint32_t)(x >> (S & 63u)) & Cfg::kMask)                              \
    MH_FINISH(J, OW)                                                                \
  }
  // keep sh < 32 at the start of every symbol pair (each code is <= 16 bits)
#define MH_REFILL_C(c)                                                              \
  {                                                                                 \
    hi = c ? lo : hi;                                                               \
    lo = c ? nw : lo;                                                               \
    const uint32_t d = c ? 4u : 0u;                                                 \
    wa += d;                                                                        \
    /* swizzled stage: keep wa one register (else it is re-derived as a sum of */  \
    /* every step's d inside each masked refill, which spills)                */  \
    if constexpr (Cfg::kSwz) asm volatile("" : "+v"(wa));                          \
    /* masked refill: the selects stay selects (v_cndmask) -- else the compiler   */  \
    /* folds them into the masked read's if-block as exec-masked copies (8 moves  */  \
    /* at every row start)                                                        */  \
    if constexpr (Cfg::kMasked) asm volatile("" : "+v"(hi), "+v"(lo));             \
    S += d * 8u;                                                                    \
    if constexpr (!Cfg::kMasked) nw = rd(wa + 8);                                   \
  }
  // The lazy step in two halves, so that the row loop can end right behind a lookup:
  // MH_ISSUE_L reads the entry at the cursor into eL, MH_TAIL_L is the rest of that step.
#define MH_ISSUE_L() MH_ISSUE_LQ(const)
#define MH_ISSUE_LQ(Q)                                                              \
  {                                                                                 \
    const uint64_t x = (((uint64_t)hi) << 32) | lo;                                 \
    eL = *(Q __attribute__((address_space(3))) uint16_t *)((lds_u8)lut + ((uint32_t)(x >> (S & 63u)) & Cfg::kMask)); \
  }
#define MH_TAIL_L(J, OW)                                                            \
  {                                                                                 \
    uint32_t e = eL;                                                                \
    /* off the chain: refill from the cursor this lookup used */                    \
    const bool c = (S & 0xFFu) <= kRefill;                                         \
    hi = c ? lo : hi;                                                               \
    lo = c ? nw : lo;                                                               \
    const uint32_t d = c ? 4u : 0u;                                                 \
    wa += d;                                                                        \
    S += d * 8u;                                                                    \
    /* keep S + d*8 one add ahead of S + e (else it is re-associated onto the  */  \
    /* chain), and the selects as selects                                       */  \
    asm volatile("" : "+v"(S), "+v"(hi), "+v"(lo));                                \
    /* the next word at even steps only: wa changes only at a refill and no     */  \
    /* refill follows a refill, so an even step lies between two refills and its */ \
    /* read lands a step before the next one needs it (half the stage reads)     */ \
    if constexpr (((J) & 1) == 0) nw = rd(wa + 8);                                 \
    MH_FINISH(J, OW)                                                                \
  }
#define MH_STEP_R(J, OW)                                                            \
  {                                                                                 \
    const bool c = (S & 0xFFu) <= kRefill;                                         \
    MH_REFILL_C(c)                                                                  \
    MH_STEP(J, OW)                                                                  \
    /* masked: only lanes that consumed a word fetch the next (issued behind the */ \
    /* lookup; fewer active lanes -> fewer LDS bank conflicts)                   */ \
    if constexpr (Cfg::kMasked) {                                                   \
      if (c) nw = rd(wa + 8);                                                       \
    }                                                                               \
  }

  // dead lanes store at >= 2^31 + r * pitch: past every output descriptor's range
  // (<= 0x7FFFFFF0 bytes), so the hardware drops them -- one select per tile, not per row
  const uint32_t rbase = (dead || MH_DIAG_DROP_STORES) ? 0x80000000u : row0;
  // Unconditional 8-byte row store (exact vmcnt counting): lanes without a
  // block and rows below the frame use offsets outside the descriptor's range,
  // which the hardware drops. A right-edge block writes its 8 bytes into the
  // row's pitch padding (pitch >= round_up(W, 8)).
  // (StoreRows; another output stage takes the row number and works out its own offset)
  const auto store_row = [&](uint32_t r, uint32_t o0, uint32_t o1, uint32_t off) {
    sink.template row<Cfg::kAux>(out, r, o0, o1, off, rbase, pitch);
  };
  MH_ROW_STAMP(8);
  if constexpr (Cfg::kLazy) {
    // The small-launch chain is a real loop over rows (kLazyRowsPerIter rows per trip; a row's
    // 8 steps stay unrolled): every wave runs the chain once, so unrolled it fetched ~7 KB of
    // code in a straight line per launch, and the first launch after other work stalled on it
    // (profiles/chain_rows_stamps.txt). The loop is rotated: a trip ends
    // with the lookup of the next row's first symbol, so the back-edge lies in that read's LDS
    // shadow; it still costs ~80 cycles when taken, which is why a trip is 4 rows and not 1 or 2
    // (profiles/chain_loop_stamps.txt). The lookup behind the last row reads a valid table
    // entry (the address is masked) and is dropped.
    uint32_t eL;
    uint32_t off = rbase;  // the row's store offset, advancing by pitch
    constexpr uint32_t kPerTrip = kLazyRowsPerIter < kRows ? kLazyRowsPerIter : kRows;  // (half a block: one trip)
    MH_ISSUE_L();
#pragma unroll 1
    for (uint32_t r = 0; r < (uint32_t)kRows; r += kPerTrip) {
#pragma unroll
      for (uint32_t q = 0; q < kPerTrip; ++q) {
        uint32_t o0 = 0, o1 = 0;
        uint32_t sv[4];  // S after each symbol of the current output word (delta mode)
        (void)sv;
        MH_TAIL_L(0, o0);
        MH_ISSUE_L();
        MH_TAIL_L(1, o0);
        MH_ISSUE_L();
        MH_TAIL_L(2, o0);
        MH_ISSUE_L();
        MH_TAIL_L(3, o0);
        if (kDelta) o0 = pack_prev4(sv[0], sv[1], sv[2], sv[3]);
        MH_ISSUE_L();
        MH_TAIL_L(0, o1);
        MH_ISSUE_L();
        MH_TAIL_L(1, o1);
        MH_ISSUE_L();
        MH_TAIL_L(2, o1);
        MH_ISSUE_L();
        MH_TAIL_L(3, o1);
        if (kDelta) o1 = pack_prev4(sv[0], sv[1], sv[2], sv[3]);
        // A trip's last lookup is a volatile read: it stays in front of the back-edge (a plain
        // one, dead on the loop's exit, is sunk into the next trip's head, behind the branch),
        // and the row store stays behind it, off the chain.
        if (q + 1 == kPerTrip && kPerTrip < (uint32_t)kRows) {
          MH_ISSUE_LQ(const volatile);
        } else {
          MH_ISSUE_L();
        }
        store_row(r + q, o0, o1, off);
        off += pitch;
        MH_ROW_STAMP(r + q);
      }
    }
  } else {
#pragma unroll
  for (uint32_t r = 0; r < (uint32_t)kRows; ++r) {
    uint32_t o0 = 0, o1 = 0;
    uint32_t sv[4];  // S after each symbol of the current output word (delta mode)
    (void)sv;
    if (r) {
      MH_STEP_R(0, o0);
    } else {
      MH_STEP(0, o0);
    }
    MH_STEP(1, o0);
    MH_STEP_R(2, o0);
    MH_STEP(3, o0);
    if (kDelta) o0 = pack_prev4(sv[0], sv[1], sv[2], sv[3]);
    MH_STEP_R(0, o1);
    MH_STEP(1, o1);
    MH_STEP_R(2, o1);
    MH_STEP(3, o1);
    if (kDelta) o1 = pack_prev4(sv[0], sv[1], sv[2], sv[3]);
    store_row(r, o0, o1, rbase + r * pitch);
    MH_ROW_STAMP(r);
  }
  }
#undef MH_STEP
#undef MH_STEP_R
#undef MH_ISSUE_L
#undef MH_ISSUE_LQ
#undef MH_TAIL_L
#undef MH_LOOKUP
#undef MH_FINISH
#undef MH_REFILL_C
}

constexpr int kStageChunks = (kStageBytes / 16 + 63) / 64;  // 16-B chunks per lane (5)

// Buffer descriptors from provably wave-uniform inputs (readfirstlane), so hipcc
// does not wrap each buffer op in a waterfall loop (cdna_hip_programming.md T20).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void *base, uint32_t bytes) {
  const uint64_t p = (uint64_t)base;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
  return __builtin_amdgcn_make_buffer_rsrc((void *)(((uint64_t)hi << 32) | lo), (short)0,
                                           (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// A tile's header loads (issued one tile ahead; all VMEM so that no scalar load
// is pending in lgkmcnt while the decode waits on LDS reads).
// tile -> frame. A launch of one frame skips the division (a uniform branch): the
// division is ~30 instructions ahead of a wave's first HBM load (its block offsets).
__device__ __forceinline__ uint32_t frame_of(const DecodeArgs &a, uint32_t tile) {
  if (a.total_tiles <= a.tiles_per_frame) return 0u;
  return tile / a.tiles_per_frame;
}

// Tile -> blocks: the mapping policy of the helpers below (a type, and for a region an object).
// FrameMap, the default: tile t of a frame is blocks [64 t, 64 t + 64) of the frame in block
//   order; tiles count through the batch (frame_of) and the last tile of a frame may be short.
// RegionMap (mh_decode_region): a tile is a run of <= 64 consecutive blocks inside ONE block row
//   of the region [bx0, bx0 + bw) x [by0, by0 + bh): S = ceil(bw / 64) tiles per row, tile t =
//   (row r = t / S, segment s = t - r S), first block (by0 + r) * a.bw + bx0 + 64 s of the frame,
//   min(64, bw - 64 s) live lanes, stored at region row 8 r, byte 8 (64 s + lane). Tiles are
//   relative to the workgroup's frame `f` (a.total_tiles == a.tiles_per_frame == bh * S), and
//   a.bw / a.nb stay the FRAME's: offsets and block_init are indexed by the frame's block number.
// WindowMap (mh_decode_windows): a RegionMap whose frame and origin come from the workgroup's window
//   descriptor, and whose raster slot is the window's index `slot`, not the frame: `f` addresses
//   what is read (offsets, codes, block_init), raster_slot() what is written. Its report() writes
//   the window's status word (slice_decode calls every map's; the others report nothing).
// CropMap (mh_decode_crops): a WindowMap at a pixel origin. Block row r of the crop is frame block
//   row by0 + r, by0 = y0 >> 3; a tile is a run of <= 64 blocks that yields <= 63 output words (word
//   j needs blocks j and j + 1), so tiles step by 63 blocks: tile (r, s) starts at block bx0 + 63 s,
//   bx0 = x0 >> 3, and holds min(64, NB - 63 s) live blocks, NB = ceil((dx + w) / 8) the blocks a row
//   of the crop touches (`bw`; x0 + w <= W keeps them inside the grid). `rem` packs what the output
//   addressing needs: dx | dy << 4 | OW << 8, OW = ceil(w / 8) <= 8192.
struct FrameMap {
  static constexpr bool kRegion = false;
  static constexpr bool kCrop = false;
  static constexpr bool kOwnBase = false;
  static constexpr bool kOwnTiles = false;  // tiles count through the batch (frame_of)
  static constexpr bool kResume = false;    // batch_loop stays in its slow loop behind an oversize tile
  __device__ __forceinline__ void report(uint32_t, uint32_t) const {}
};
struct RegionMap {
  static constexpr bool kRegion = true;
  static constexpr bool kCrop = false;
  static constexpr bool kOwnBase = false;  // a.offsets / a.block_init are the batch's: frame f's entries at + f * a.nb
  static constexpr bool kOwnTiles = false;  // (a region's tiles are frame relative by kRegion itself)
  static constexpr bool kResume = false;
  static constexpr uint32_t kStep = 64u;  // blocks from one tile of a row to the next
  uint32_t f, bx0, by0, bw, S;
  // BoxRows only: the frame's pixels from the region's origin on, (W - 8 bx0) | (H - 8 by0) << 16
  // (both <= 65535) -- one SGPR for a tile's edge facts, where W, H and the origin would be four
  uint32_t rem = 0;
  __device__ __forceinline__ uint32_t raster_slot() const { return f; }
  __device__ __forceinline__ void report(uint32_t, uint32_t) const {}
};
struct WindowMap : RegionMap {
  uint32_t slot;
  int32_t *wstatus;  // d_window_status or null
  __device__ __forceinline__ uint32_t raster_slot() const { return slot; }
  // the window's status word = its frame's (0: MH_OK), written by one thread of slice 0 with a vector store
  __device__ __forceinline__ void report(uint32_t frame_status, uint32_t slice) const {
    if (wstatus && slice == 0 && threadIdx.x == 0) wstatus[slot] = (int32_t)frame_status;
  }
};

struct CropMap : WindowMap {
  static constexpr bool kCrop = true;
  static constexpr uint32_t kStep = 63u;
  __device__ __forceinline__ uint32_t dx() const { return rem & 7u; }
  __device__ __forceinline__ uint32_t dy() const { return (rem >> 4) & 7u; }
  __device__ __forceinline__ uint32_t ow() const { return rem >> 8; }
};

// NormMap (mh_decode_crops_norm): a CropMap that also carries what the NormRows stage takes per
//   tile: bit 3 of `rem` (free between dx and dy) is the crop's mirror flag; the stage's byte
//   selector, scale and bias are per-lane VGPRs for the workgroup's whole life, so neither an SGPR
//   nor a move per tile is spent on them.
struct NormMap : CropMap {
  uint32_t sel;
  float scale, bias;
  __device__ __forceinline__ uint32_t mirror() const { return (rem >> 3) & 1u; }
};

// SetCropMap / SetNormMap (mh_decode_set_crops, mh_decode_set_crops_norm_planes): the crop maps over
//   a frame SET, whose frames differ in size. The entry has read the frame's geometry record and
//   put the frame's own block grid into the workgroup's DecodeArgs: a.bw and a.nb are this frame's,
//   and a.offsets / a.block_init are already based at the frame's first block (kOwnBase), so the
//   header loads add no f * a.nb. `f` still addresses the codes, the table and the status word.
struct SetCropMap : CropMap {
  static constexpr bool kOwnBase = true;
};
struct SetNormMap : NormMap {
  static constexpr bool kOwnBase = true;
};

// SetFrameMap (mh_decode_set_frames): FrameMap's tiles -- 64 consecutive blocks of the frame in block
//   order, every lane of every tile but the frame's last holding a block -- over a frame SET. The
//   frames differ in size, so no tile index runs through the set: tiles count from the frame's own
//   block 0 (kOwnTiles: a.total_tiles == a.tiles_per_frame == the frame's tiles, no f * tiles and no
//   tile -> frame division anywhere), the arrays are based at the frame's first block (kOwnBase) and
//   the raster's base is the frame's own (slot 0, stride 0). `f` still addresses the codes, the table
//   and the status word; report() carries the frame's status word into the set's.
struct SetFrameMap {
  static constexpr bool kRegion = false;
  static constexpr bool kCrop = false;
  static constexpr bool kOwnBase = true;
  static constexpr bool kOwnTiles = true;
  static constexpr bool kResume = true;  // back to the pipelined loop behind one oversize tile
  uint32_t f;
  int32_t *sstatus;  // d_set_status or null
  __device__ __forceinline__ void report(uint32_t frame_status, uint32_t slice) const {
    if (sstatus && slice == 0 && threadIdx.x == 0) sstatus[f] = (int32_t)frame_status;
  }
};

struct TileHdrBase {
  uint32_t tile;      // wave-uniform; >= total_tiles: no tile
  uint32_t off;       // this lane's block start bit
  uint32_t nxt;       // next block's start bit (this lane's block end)
  uint32_t fo_lo, fo_hi;  // lanes 0/1: frame_off[f], frame_off[f+1]
  uint32_t init;      // per-block initial prev (block_init) or 0
};
// ... and what a map adds to it (FrameMap: nothing; a region map of any kind: the same two words).
// A partial specialisation on Map::kRegion, so a new map adds no line here. (The same choice as a
// std::conditional_t alias is not the same code: it moved instructions in 12 kernels, the
// single-frame kernel among them -- DESIGN.md section 3i.)
template <class Map, bool = Map::kRegion>
struct TileHdrOf : TileHdrBase {};
template <class Map>
struct TileHdrOf<Map, true> : TileHdrBase {
  uint32_t r, s;      // the tile's region row and segment (wave-uniform)
};
using TileHdr = TileHdrOf<FrameMap>;

// tile -> (r, s). One segment per row skips the division (a uniform branch), as frame_of does
// for one frame: it sits ahead of the wave's first HBM load.
__device__ __forceinline__ void region_rs(const RegionMap &m, uint32_t tile, uint32_t &r, uint32_t &s) {
  r = tile;
  s = 0u;
  if (m.S != 1u) {
    r = tile / m.S;
    s = tile - r * m.S;
  }
}

template <class Map = FrameMap>
__device__ __forceinline__ void hdr_issue(const DecodeArgs &a, uint32_t tile, uint32_t lane,
                                          TileHdrOf<Map> &h, const Map &m = Map()) {
  // Branch-free: absent arrays (frame_off / block_init == NULL) get descriptors
  // with zero records, whose loads return 0 without touching memory; a past-the-end
  // tile reads through zero-record descriptors too. Unconditional loads keep the
  // compiler from waiting on the span prefetch to re-zero these registers.
  tile = __builtin_amdgcn_readfirstlane(tile);
  const bool live = tile < a.total_tiles;
  uint32_t f, b;
  if constexpr (Map::kRegion) {
    region_rs(m, tile, h.r, h.s);
    f = m.f;
    b = (live ? (m.by0 + h.r) * a.bw + m.bx0 + Map::kStep * h.s : 0u) + lane;
  } else if constexpr (Map::kOwnTiles) {
    f = m.f;
    b = (live ? tile * 64u : 0u) + lane;
  } else {
    f = live ? frame_of(a, tile) : 0u;
    b = (live ? (tile - f * a.tiles_per_frame) * 64u : 0u) + lane;
  }
  h.tile = tile;
  // the frame's first block in offsets / block_init: f * a.nb in a batch of one size; a set's entry
  // has based both arrays at it (kOwnBase)
  uint64_t fb = 0;
  if constexpr (!Map::kOwnBase) fb = (uint64_t)f * a.nb;
  const __amdgpu_buffer_rsrc_t ro = uniform_rsrc(a.offsets + fb, live ? a.nb * 4u : 0u);
  h.off = __builtin_amdgcn_raw_buffer_load_b32(ro, (int)(b * 4u), 0, 0);
  h.nxt = __builtin_amdgcn_raw_buffer_load_b32(ro, (int)(b * 4u + 4u), 0, 0);
  typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t rf = uniform_rsrc(
      a.frame_off ? (const void *)a.frame_off : (const void *)a.offsets,
      (live && a.frame_off) ? 0x7FFFFFF0u : 0u);
  const v2u32 v = __builtin_amdgcn_raw_buffer_load_b64(rf, (int)((f + (lane & 1u)) * 8u), 0, 0);
  h.fo_lo = v.x;
  h.fo_hi = v.y;
  const __amdgpu_buffer_rsrc_t ri = uniform_rsrc(
      a.block_init ? (const void *)(a.block_init + fb) : (const void *)a.offsets,
      (live && a.block_init) ? a.nb : 0u);
  h.init = __builtin_amdgcn_raw_buffer_load_b8(ri, (int)b, 0, 0);
}

// Everything derived from a header once its loads have landed.
struct TileBase {
  uint32_t tile, f, b0;  // f: the raster slot (the frame; a window's index under WindowMap)
  bool valid;          // this lane holds a block
  uint32_t p;          // lane's start bit relative to the staged span
  uint32_t start;      // span start byte (16-aligned, frame relative)
  uint32_t span;       // span bytes (0xFFFFFFFF: unknown / corrupt)
  uint32_t fb32;       // frame bytes (clamped to u32)
  uint64_t fbeg;
  uint32_t init;
  uint32_t span_end_bits;  // end bit of the tile's last block (frame relative)
};
template <class Map, bool = Map::kRegion>
struct TileOf : TileBase {};
template <class Map>
struct TileOf<Map, true> : TileBase {
  uint32_t r, s, n;    // region row, segment, blocks in the run (1..64)
};
using Tile = TileOf<FrameMap>;

template <class Map = FrameMap>
__device__ __forceinline__ TileOf<Map> hdr_resolve(const DecodeArgs &a, const TileHdrOf<Map> &h, uint32_t lane,
                                                   const Map &m = Map()) {
  TileOf<Map> t;
  t.tile = h.tile;
  if constexpr (Map::kRegion) {
    t.f = m.raster_slot();
    t.r = h.r;
    t.s = h.s;
    t.n = min(64u, m.bw - Map::kStep * h.s);
    t.b0 = (m.by0 + h.r) * a.bw + m.bx0 + Map::kStep * h.s;
  } else if constexpr (Map::kOwnTiles) {
    t.f = 0u;  // the raster's base is the frame's own
    t.b0 = h.tile * 64u;
  } else {
    t.f = frame_of(a, h.tile);
    t.b0 = (h.tile - t.f * a.tiles_per_frame) * 64u;
  }
  const uint32_t b = t.b0 + lane;
  // a region's lanes past the run are dead even where the frame has a block: those are real
  // blocks to the right of the region
  if constexpr (Map::kRegion)
    t.valid = lane < t.n;
  else
    t.valid = b < a.nb;
  uint64_t fbytes = a.codes_bytes;
  t.fbeg = 0;
  if (a.frame_off) {
    const uint64_t lo = ((uint64_t)__builtin_amdgcn_readlane(h.fo_hi, 0) << 32) |
                        __builtin_amdgcn_readlane(h.fo_lo, 0);
    const uint64_t hi = ((uint64_t)__builtin_amdgcn_readlane(h.fo_hi, 1) << 32) |
                        __builtin_amdgcn_readlane(h.fo_lo, 1);
    t.fbeg = lo;
    fbytes = hi - lo;
  }
  t.fb32 = (uint32_t)(fbytes > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : fbytes);
  const uint32_t fbits = t.fb32 > 0x1FFFFFFFu ? 0xFFFFFFFFu : t.fb32 * 8u;
  // a frame's last block ends at most 64 x 16 bits after its start, whatever the
  // buffer size (a reused streaming slot is larger than the frame it holds).
  // The sum wraps for a last block at or above bit 2^32 - 1024: the end then lies below the
  // tile's start, so the span below is "unknown" and the tile takes decode_halves, whose
  // (end - start) wraps again to a whole window from the half's own start.
  // (a region's run ends at the next block's offset too, though that block lies outside it)
  const uint32_t end_l = (b + 1u < a.nb) ? h.nxt : min(fbits, h.off + 64u * 16u);
  uint32_t last;  // last lane holding a block
  if constexpr (Map::kRegion)
    last = t.n - 1u;
  else
    last = min(63u, a.nb - 1u - t.b0);
  const uint32_t sb = __builtin_amdgcn_readfirstlane(h.off);
  const uint32_t eb = __builtin_amdgcn_readlane(end_l, last);
  t.span_end_bits = eb;
  t.start = (sb >> 3) & ~15u;
  uint32_t end = (eb >> 3) + 24u;
  // compared without the sum: fb32 + 16 wraps to 0 for a frame of 0xFFFFFFF0 bytes (end >= 24)
  if (end - 16u > t.fb32) end = t.fb32 + 16u;
  t.span = end > t.start ? ((end - t.start + 15u) & ~15u) : 0xFFFFFFFFu;
  t.p = t.valid ? h.off - t.start * 8u : 0u;
  t.init = h.init & 0xFFu;
  // materialise every header-derived value now: the loads are a tile old, and no
  // later use may make the compiler wait on the span prefetch issued after this
  asm volatile("" ::"v"(t.p), "v"(t.init));
  return t;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t codes_rsrc(const DecodeArgs &a, const TileBase &t) {
  return uniform_rsrc(a.codes + t.fbeg, t.fb32);
}

// Output addressing of a tile: a store descriptor based at the tile's first block
// row (64-bit base, so frames beyond 4 GB of raster work) and each lane's offset
// of its block's first row from there. Stores below row H fall outside the
// descriptor's range and are dropped.
struct OutTile {
  __amdgpu_buffer_rsrc_t rsrc;
  uint32_t row0;
};
template <class Map = FrameMap, class Out = StoreRows>
__device__ __forceinline__ OutTile out_tile(const DecodeArgs &a, const TileOf<Map> &t, uint32_t lane,
                                            const Map &m = Map()) {
  constexpr int kLog2 = Out::kLog2;
  static_assert(Map::kRegion || kLog2 == 0, "only a region is decoded at a reduced scale");
  if constexpr (Map::kCrop) {
    // Block row r holds crop rows 8 r - dy .. 8 r - dy + 7. The descriptor is based at the first of
    // them that exists (crop row 0 for r = 0) and limited by h * pitch (a.out_frame_bytes), so rows
    // >= h are dropped. The dy rows above the crop lie BELOW the base: the lane's first offset is
    // 8 (word) - dy * pitch in 32-bit arithmetic, so those rows' offsets are "negative", above every
    // descriptor's range (dy * pitch <= 7 * 2^20), and are dropped too; row dy lands on offset
    // 8 (word). The sum is formed in a register, never in the instruction's offset fields.
    // A lane stores word 63 s + lane while that is below OW and lane < 63; every other lane (the
    // 64th block, blocks past the crop, lanes without a block) takes the dead offset.
    const uint32_t dy = m.dy(), words = min(63u, m.ow() - 63u * t.s);
    const uint32_t top = t.r ? 8u * t.r - dy : 0u;
    const uint64_t base = (uint64_t)top * a.out_pitch;
    const uint64_t rem = a.out_frame_bytes > base ? a.out_frame_bytes - base : 0u;
    OutTile o;
    o.rsrc = uniform_rsrc(a.out + (uint64_t)t.f * a.out_frame_stride + base,
                          (uint32_t)(rem < 0x7FFFFFF0ull ? rem : 0x7FFFFFF0ull));
    const uint32_t above = t.r ? 0u : dy * (uint32_t)a.out_pitch;
    if constexpr (Out::kNorm) {
      // a word is 8 elements of Out::kElem bytes, and a mirrored crop's word j is the row's word
      // OW - 1 - j (w is a multiple of 8 then: the kernel's verdict). The second store of a binary32
      // row lies 16 bytes on: (word + 1) * 32 <= pitch (the host's check), so a row above the crop
      // stays "negative" and the dead offset stays out of range with it.
      // (by arithmetic, ~j + OW = OW - 1 - j: a select's mask would be one more SGPR pair)
      const uint32_t j = 63u * t.s + lane, mask = 0u - m.mirror(), word = (j ^ mask) + (mask & m.ow());
      o.row0 = lane < words ? word * (8u * Out::kElem) - above : 0x80000000u;
    } else {
      o.row0 = lane < words ? (63u * t.s + lane) * 8u - above : 0x80000000u;
    }
    asm volatile("" : "+v"(o.row0));
    return o;
  } else if constexpr (Map::kRegion) {
    // based at region row 8 r of the raster slot t.f (the frame; a window's index) and limited by
    // RH * pitch (a.out_frame_bytes): rows >= RH are dropped.
    // At scale 2^kLog2 a block row is c = 8 >> kLog2 output rows of c bytes per block, and the
    // limit is SH * pitch.
    constexpr uint32_t c = 8u >> kLog2;
    const uint64_t base = (uint64_t)t.r * c * a.out_pitch;
    const uint64_t rem = a.out_frame_bytes > base ? a.out_frame_bytes - base : 0u;
    OutTile o;
    o.rsrc = uniform_rsrc(a.out + (uint64_t)t.f * a.out_frame_stride + base,
                          (uint32_t)(rem < 0x7FFFFFF0ull ? rem : 0x7FFFFFF0ull));
    o.row0 = (64u * t.s + lane) * c;
    return o;
  } else {
    const uint32_t b = t.b0 + lane;
    const uint32_t bx = b % a.bw, by = b / a.bw;
    const uint32_t by0 = __builtin_amdgcn_readfirstlane(t.b0 / a.bw);
    const uint64_t base = (uint64_t)by0 * 8u * a.out_pitch;
    const uint64_t rem = a.out_frame_bytes > base ? a.out_frame_bytes - base : 0u;
    OutTile o;
    o.rsrc = uniform_rsrc(a.out + (uint64_t)t.f * a.out_frame_stride + base,
                          (uint32_t)(rem < 0x7FFFFFF0ull ? rem : 0x7FFFFFF0ull));
    o.row0 = (by - by0) * 8u * (uint32_t)a.out_pitch + bx * 8u;
    return o;
  }
}

// A tile's output stage (StoreRows / BoxRows above). StoreRows has no state. BoxRows takes the
// tile's edge facts: how many rows of its block row lie inside the frame (a region tile lies in
// one block row, so this is wave-uniform) and the lane's column selectors.
template <class Out, class Map>
__device__ __forceinline__ Out rows_of(const DecodeArgs &a, const TileOf<Map> &t, uint32_t lane, const Map &m) {
  if constexpr (Out::kCrop) {
    static_assert(Map::kCrop, "a crop's output stage takes a crop's map");
    Out o;
    o.lo = m.dx() < 4u ? ~0u : 0u;
    o.k = m.dx() & 3u;
    asm volatile("" : "+v"(o.lo), "+v"(o.k));  // per-lane registers: the chain has no SGPR for either
    if constexpr (Out::kNorm) {
      o.sel = m.sel;
      o.scale = m.scale;
      o.bias = m.bias;
    }
    return o;
  } else if constexpr (Out::kLog2 == 0) {
    return Out();
  } else {
    static_assert(Map::kRegion, "only a region is decoded at a reduced scale");
    Out o;
    const uint32_t cols = (m.rem & 0xFFFFu) - 512u * t.s;  // in-frame columns from the tile's first block on
    o.ch = __builtin_amdgcn_readfirstlane(min(8u, (m.rem >> 16) - 8u * t.r));
    const uint32_t cw = (uint32_t)min(max((int)cols - 8 * (int)lane, 0), 8);  // 0: a dead lane past the frame
    // byte i of a word keeps selector i while its column is inside the frame, else the constant 0;
    // at scale 2 a last column alone in its cell (cw odd) is copied into its neighbour
    const uint64_t keep = cw >= 8u ? ~0ull : (1ull << (8u * cw)) - 1ull;
    uint64_t sel = (0x0302010003020100ull & keep) | (0x0C0C0C0C0C0C0C0Cull & ~keep);
    if (Out::kLog2 == 1 && (cw & 1u)) sel = (sel & ~(0xFFull << (8u * cw))) | ((uint64_t)((cw - 1u) & 3u) << (8u * cw));
    o.sel0 = (uint32_t)sel;
    o.sel1 = (uint32_t)(sel >> 32);
    return o;
  }
}

template <int kChunks>
__device__ __forceinline__ void span_issue(const DecodeArgs &a, const TileBase &t, uint32_t lane,
                                           v4u32 (&R)[kChunks], bool on = true) {
  // Unconditional loads (no exec-masked branches, so the compiler can count them
  // in vmcnt); chunks past the span use an offset outside the descriptor's range,
  // which returns 0 without a memory access.
  // not `on`: a zero-record descriptor, so no offset can reach memory
  const __amdgpu_buffer_rsrc_t rc = uniform_rsrc(a.codes + (on ? t.fbeg : 0ull), on ? t.fb32 : 0u);
  // one wave-uniform byte count, so the compiler cannot split the loads by `on`
  const uint32_t span = __builtin_amdgcn_readfirstlane(on ? t.span : 0u);
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const uint32_t c = lane + 64u * k;
    const uint32_t off = c * 16u < span ? t.start + c * 16u : 0xFFFFFFF0u;
    R[k] = __builtin_amdgcn_raw_buffer_load_b128(rc, (int)off, 0, 0);
  }
}

template <bool kSwz = false, int kChunks>
__device__ __forceinline__ void span_write(const TileBase &t, uint32_t lane, const v4u32 (&R)[kChunks],
                                           uint8_t *stage) {
#pragma unroll
  for (int k = 0; k < kChunks; ++k) {
    const uint32_t c = lane + 64u * k;
    if (c * 16u < t.span) {
      v4u32 v = R[k];
      v.x = bswap32(v.x);
      v.y = bswap32(v.y);
      v.z = bswap32(v.z);
      v.w = bswap32(v.w);
      *reinterpret_cast<v4u32 *>(stage + (kSwz ? swz_off(c * 16u) : c * 16u)) = v;
    }
  }
}

// A workgroup barrier for LDS-only hand-offs: waits for this wave's LDS operations
// (lgkmcnt), not its global ones -- __syncthreads()'s workgroup-scope fence also waits
// for every outstanding global load (vmcnt(0)), here the first header.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The unstaged paths' staging: `span` bytes of the frame's codes from byte `start` (16-aligned) into
// the wave's window, 16 bytes per lane and trip, byte-swapped as span_write does. Loads past the
// frame's bytes return 0 (the descriptor). Used by decode_halves and by the marked single-frame
// kernel's oversize tile.
template <bool kSwz = false>
__device__ __forceinline__ void stage_window(__amdgpu_buffer_rsrc_t rc, uint32_t start, uint32_t span, uint32_t lane,
                                             uint8_t *stage) {
  for (uint32_t c = lane; c * 16u < span; c += 64u) {
    v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(rc, (int)(start + c * 16u), 0, 0);
    v.x = bswap32(v.x);
    v.y = bswap32(v.y);
    v.z = bswap32(v.z);
    v.w = bswap32(v.w);
    *reinterpret_cast<v4u32 *>(stage + (kSwz ? swz_off(c * 16u) : c * 16u)) = v;
  }
}

// Oversize tile: stage + decode lanes [0,32) then [32,64), each from its own span.
// A crop's output stage reads the lane to the right, so its first pass is lanes [0,33): lane 32
// decodes there for lane 31's sake alone (its own stores go to the dead offset) and again, for its
// own word, in the second pass, where lane 33 runs beside it. 33 blocks are at most 33 x 128 B
// plus the span's slack of under 64 B, inside the 4352-byte window.
template <bool kDelta, class Cfg, class Map = FrameMap, class Out = StoreRows>
__device__ __forceinline__ void decode_halves(const DecodeArgs &a, const TileOf<Map> &t, uint32_t lane,
                                              const uint8_t *lut, uint8_t *stage,
                                              __amdgpu_buffer_rsrc_t out, uint32_t row0, bool dead, Out sink = Out()) {
  const __amdgpu_buffer_rsrc_t rc = codes_rsrc(a, t);
  const uint32_t my_off = t.p + t.start * 8u;  // lane's absolute start bit
  const uint32_t fbits = t.fb32 > 0x1FFFFFFFu ? 0xFFFFFFFFu : t.fb32 * 8u;
#pragma unroll 1
  for (uint32_t h = 0; h < 2; ++h) {
    const uint32_t first = h * 32u;
    const uint32_t lanes = 32u + ((Out::kCrop && h == 0u) ? 1u : 0u);
    const uint32_t sb = __builtin_amdgcn_readlane(my_off, first);
    // end of the half: start bit of lane first+32 (or the tile's last block end)
    uint32_t nblk;  // blocks in this tile (may be < 64)
    if constexpr (Map::kRegion)
      nblk = t.n;
    else
      nblk = a.nb - t.b0;
    if (first >= nblk) break;
    uint32_t eb;
    if (first + lanes < nblk) {
      eb = __builtin_amdgcn_readlane(my_off, first + lanes);
    } else {
      eb = t.span_end_bits;
    }
    const uint32_t start = (sb >> 3) & ~15u;
    uint32_t end = (eb >> 3) + 24u;
    if (end - 16u > t.fb32) end = t.fb32 + 16u;  // as hdr_resolve: no wrapping sum
    const uint32_t span = min((end - start + 15u) & ~15u, (uint32_t)kStageBytes);
    __builtin_amdgcn_s_waitcnt(0);  // rare path: drain before reusing the window
    stage_window<Cfg::kSwz>(rc, start, span, lane, stage);
    wave_sync();
    if (lane >= first && lane < first + lanes) {
      LdsWords src{stage};
      const uint32_t r0 = (Out::kCrop && h == 0u && lane == 32u) ? 0x80000000u : row0;
      decode_block<kDelta, Cfg>(src, lut, t.valid ? my_off - start * 8u : 0u, t.init, out, r0,
                                (uint32_t)a.out_pitch, dead MH_ROWS_NONE, sink);  // (a lane stores in one half only)
    }
    wave_sync();
  }
  __builtin_amdgcn_s_waitcnt(0);
  (void)fbits;
}

#if MH_DIAG_STAMPS
#define MH_TS_PARAM , unsigned long long (&ts)[kDiagSlots]
#define MH_TS_ARG , ts
#else
#define MH_TS_PARAM
#define MH_TS_ARG
#endif

// static grid-stride schedule; a tile id >= total_tiles means "no tile"
__device__ __forceinline__ uint32_t next_tile(const DecodeArgs &a, uint32_t t, uint32_t gstride) {
  return t < a.total_tiles ? min(t + gstride, a.total_tiles) : a.total_tiles;
}

// The batch kernel's persistent loop for ONE step flavour (Cfg), entered with the first
// tile's header in flight (hc) and, when `synced`, the table in LDS. Software-pipelined
// one tile ahead: while tile i decodes (LDS + VALU only), the header of tile i+2 and the
// code span of tile i+1 are in flight into registers; the span is written to the wave's
// LDS window once tile i has finished reading it. One instantiation per flavour, entered
// with nothing but the first header live (a flavour branch with the first span in
// flight spilled: 80 VGPRs + 40 B of scratch).
template <bool kDelta, class Cfg, class Map = FrameMap, class Out = StoreRows>
__device__ __forceinline__ void batch_loop(const DecodeArgs &a, uint32_t lane, uint8_t *stage,
                                           const uint8_t *lut, uint32_t t0, uint32_t gstride,
                                           const TileHdrOf<Map> &hc, bool synced MH_TS_PARAM, const Map &m = Map()) {
  // the header of the loop's first tile: the caller's, or (Map::kResume, below) that of the tile at
  // which the pipelined loop is entered again. By value: through a pointer it would live in scratch.
  TileHdrOf<Map> h0 = hc;
resume:
  TileHdrOf<Map> hn;
#if MH_DIAG_STAMPS
  bool first_tile = true;
#endif
  v4u32 R[kStageChunks];
  TileOf<Map> cur = hdr_resolve(a, h0, lane, m);
  MH_STAMP(1);
  bool cur_staged = cur.tile < a.total_tiles && cur.span <= (uint32_t)kStageBytes;
  span_issue(a, cur, lane, R, cur_staged);
  hdr_issue(a, next_tile(a, t0, gstride), lane, hn, m);
  if constexpr (Cfg::kEsc) {  // the general flavour: also an in-kernel table, or a copy loop
    if (!synced) {
      if (a.lut)
        __syncthreads();
      else
        build_lut(a.t1, a.t2, a.t2_entries, s_lut, &s_p0, threadIdx.x, a.nwaves * 64u, [] { __syncthreads(); });
    }
  }
  MH_STAMP(2);
  if (cur_staged) span_write<Cfg::kSwz>(cur, lane, R, stage);
  MH_STAMP(3);
  // Resolved even past the end (zero-record loads): every Tile field is defined
  // before span_issue builds a descriptor from it.
  TileOf<Map> nxt = hdr_resolve(a, hn, lane, m);

  // Per iteration the only VMEM issued after a prefetch is the 8 unconditional row
  // stores, so every wait below is an exact vmcnt that leaves the stores in flight.
  while (cur.tile < a.total_tiles) {  // wave-uniform
    if (__builtin_expect(!cur_staged, 0)) break;  // oversize span: finish in the slow loop
    const bool nxt_live = nxt.tile < a.total_tiles;
    const bool nxt_staged = nxt_live && nxt.span <= (uint32_t)kStageBytes;
    span_issue(a, nxt, lane, R, nxt_staged);  // unconditional (all out of range if not staged)
    hdr_issue(a, next_tile(a, nxt.tile, gstride), lane, hn, m);

    wave_sync();  // this tile's staging writes -> reads
    {
      const bool dead = !cur.valid;
      const OutTile ot = out_tile<Map, Out>(a, cur, lane, m);
      LdsWords src{stage};
      // waves with more tiles left run first (the arbiter otherwise favours the oldest)
      set_prio(min((a.total_tiles - 1u - cur.tile) / gstride, 3u));
      decode_block<kDelta, Cfg>(src, lut, cur.p, cur.init, ot.rsrc, ot.row0, (uint32_t)a.out_pitch, dead MH_ROWS_NONE,
                                rows_of<Out>(a, cur, lane, m));
    }
#if MH_DIAG_STAMPS
    if (first_tile) MH_STAMP(4);
    first_tile = false;
#endif
    wave_sync();  // this tile's reads -> next tile's staging writes
    if (nxt_staged) span_write<Cfg::kSwz>(nxt, lane, R, stage);
    const TileOf<Map> nn = hdr_resolve(a, hn, lane, m);
    cur = nxt;
    cur_staged = nxt_staged;
    nxt = nn;
  }

  // Slow loop (rare): a tile whose code span exceeds the LDS window (long codes in
  // most of its 64 blocks) and every later tile of this wave, without prefetch.
  // Kept after the pipelined loop so its waits never merge into that loop.
  for (uint32_t t = cur.tile; t < a.total_tiles; t = next_tile(a, t, gstride)) {
    __builtin_amdgcn_s_waitcnt(0);
    TileHdrOf<Map> h;
    hdr_issue(a, t, lane, h, m);
    const TileOf<Map> tt = hdr_resolve(a, h, lane, m);
    const OutTile ot = out_tile<Map, Out>(a, tt, lane, m);
    decode_halves<kDelta, Cfg, Map>(a, tt, lane, lut, stage, ot.rsrc, ot.row0, !tt.valid, rows_of<Out>(a, tt, lane, m));
    // Map::kResume: only the oversize tile itself is decoded here. The wave issues its next tile's
    // header and enters the pipelined loop again, so one dense tile early in a frame does not put
    // the wave's other tiles (about ten in a set launch) on the unpipelined path.
    if constexpr (Map::kResume) {
      t0 = next_tile(a, t, gstride);
      if (t0 >= a.total_tiles) return;
      hdr_issue(a, t0, lane, h0, m);
      goto resume;
    }
  }
}

// Flat 8-bit tables (every code 8 bits: all 256 symbols, canonical, so code c is symbol c
// -- the prepared table's flat8 word, which its builder sets only when every first-level
// entry says so, mh_lut.hpp): a block's 64 codes are its 64
// symbol bytes, MSB-first bytes in stream order. A lane decodes its block with byte
// arithmetic -- no table lookup and no serial bit cursor: 17 dwords of codes, realigned
// by v_alignbyte, one SDWA byte add per symbol for the delta sum, 3 VALU per output word.
// The uniform-random 8192^2 stress frame is such a table.
// A tile with a block that does not start on a byte (no reference producer writes one)
// takes a staged funnel-shift step. (Both kernels; the lookup chain for flat tables is the
// round-5 A/B baseline: profiles/r05_flat8_ab.txt, r05_flat8_small_ab.txt.)
struct Flat8Codes {
  uint32_t w[17];  // the block's 64 code bytes from the dword below its first byte
};

__device__ __forceinline__ void flat8_issue(const DecodeArgs &a, const TileBase &t, Flat8Codes &c) {
  // unconditional loads (a fixed count, exact vmcnt); a lane without a block reads far
  // past the frame (out of range: 0, no access)
  const __amdgpu_buffer_rsrc_t rc = codes_rsrc(a, t);
  const uint32_t byte = t.start + (t.p >> 3);  // the block's first code byte (frame relative)
  const uint32_t base = t.valid ? (byte & ~3u) : 0xFFFFFF00u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const v4u32 v = __builtin_amdgcn_raw_buffer_load_b128(rc, (int)(base + 16u * k), 0, 0);
    c.w[4 * k] = v.x;
    c.w[4 * k + 1] = v.y;
    c.w[4 * k + 2] = v.z;
    c.w[4 * k + 3] = v.w;
  }
  c.w[16] = __builtin_amdgcn_raw_buffer_load_b32(rc, (int)(base + 64u), 0, 0);
}

template <bool kDelta, class Map = FrameMap, class Out = StoreRows>
__device__ __forceinline__ void flat8_block(const DecodeArgs &a, const TileOf<Map> &t, uint32_t lane,
                                            const Flat8Codes &c, Out sink = Out(), const Map &m = Map()) {
  typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
  const uint32_t sb = (t.start + (t.p >> 3)) & 3u;
  const OutTile ot = out_tile<Map, Out>(a, t, lane, m);
  const uint32_t rbase = (t.valid && !MH_DIAG_DROP_STORES) ? ot.row0 : 0x80000000u;
  const uint32_t pitch = (uint32_t)a.out_pitch;
  uint32_t s = t.init;  // running delta sum (byte 0)
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) {
    // stream bytes 8r .. 8r + 7 (little-endian in each word: byte i = symbol 4j + i)
    const uint32_t c0 = __builtin_amdgcn_alignbyte(c.w[2 * r + 1], c.w[2 * r], sb);
    const uint32_t c1 = __builtin_amdgcn_alignbyte(c.w[2 * r + 2], c.w[2 * r + 1], sb);
    v2u32 v;
    if (kDelta) {
      uint32_t sv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) sv[i] = s = s + ((c0 >> (8 * i)) & 0xFFu);
      v.x = pack_lo4(sv[0], sv[1], sv[2], sv[3]);
#pragma unroll
      for (int i = 0; i < 4; ++i) sv[i] = s = s + ((c1 >> (8 * i)) & 0xFFu);
      v.y = pack_lo4(sv[0], sv[1], sv[2], sv[3]);
    } else {
      v.x = c0;
      v.y = c1;
    }
    sink.template row<kBatchStoreAux>(ot.rsrc, r, v, rbase + r * pitch, rbase, pitch);
  }
}

// The batch kernel's loop for flat 8-bit tables: the same static tile schedule, software
// pipelined like batch_loop -- while a tile decodes, the next tile's codes and the one
// after's header are in flight, all issued before this tile's row stores, so no wait
// below is for a store.
template <bool kDelta, class Map = FrameMap, class Out = StoreRows>
__device__ __forceinline__ void flat8_loop(const DecodeArgs &a, uint32_t lane, uint8_t *stage, const uint8_t *lut,
                                           uint32_t t0, uint32_t gstride, const TileHdrOf<Map> &hc MH_TS_PARAM,
                                           const Map &m = Map()) {
  TileHdrOf<Map> h;
  Flat8Codes cc, cn;
  TileOf<Map> cur = hdr_resolve(a, hc, lane, m);
  MH_STAMP(1);
  flat8_issue(a, cur, cc);
  hdr_issue(a, next_tile(a, t0, gstride), lane, h, m);
#if MH_DIAG_STAMPS
  ts[2] = ts[1];
  ts[3] = ts[1];
  bool first_tile = true;
#endif
  while (cur.tile < a.total_tiles) {  // wave-uniform
    // a block off the byte grid: this tile and the rest in the slow loop below
    if (__builtin_expect(__ballot(cur.valid && ((cur.p & 7u) != 0u)) != 0, 0)) break;
    const TileOf<Map> nxt = hdr_resolve(a, h, lane, m);
    flat8_issue(a, nxt, cn);
    hdr_issue(a, next_tile(a, nxt.tile, gstride), lane, h, m);
    flat8_block<kDelta, Map>(a, cur, lane, cc, rows_of<Out>(a, cur, lane, m), m);
#if MH_DIAG_STAMPS
    if (first_tile) MH_STAMP(4);  // the first tile's codes landed and its stores issued
    first_tile = false;
#endif
    cur = nxt;
    cc = cn;
  }
  // Slow loop (no reference producer gets here): each half tile staged in LDS and decoded
  // with the funnel-shift byte step (any bit alignment), no prefetch; no table needed.
  using Batch8 = StepCfg<kLutBits, true, false, false, kBatchStoreAux, false, true>;
  for (uint32_t t = cur.tile; t < a.total_tiles; t = next_tile(a, t, gstride)) {
    __builtin_amdgcn_s_waitcnt(0);
    TileHdrOf<Map> hs;
    hdr_issue(a, t, lane, hs, m);
    const TileOf<Map> tt = hdr_resolve(a, hs, lane, m);
    const OutTile ot = out_tile<Map, Out>(a, tt, lane, m);
    decode_halves<kDelta, Batch8, Map>(a, tt, lane, lut, stage, ot.rsrc, ot.row0, !tt.valid,
                                       rows_of<Out>(a, tt, lane, m));
  }
}

// The batch kernel: persistent workgroups (wave w of workgroup g decodes tiles
// g*W + w, + grid*W, ...). A common prologue (table copy, first two headers, first
// span) and then one instantiation of the persistent loop per step flavour, chosen
// from the prepared table's code lengths (kernel-uniform): no code longer than 13 bits
// -> escape-free; one code length only -> escape-free with the swizzled stage. An
// in-kernel table (no prepared LUT) keeps the general step.
template <bool kDelta>
// Leading scalar arguments: preloaded into SGPRs at wave launch (as the small kernel's).
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint16_t *p_lut,
    uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_total_tiles, uint32_t p_nwaves, uint32_t p_grid,
    const DecodeArgs a0) {
  DecodeArgs a = a0;
  a.offsets = p_offsets;
  a.frame_off = p_frame_off;
  a.block_init = p_block_init;
  a.lut = p_lut;
  a.nb = p_nb;
  a.tiles_per_frame = p_tiles_per_frame;
  a.total_tiles = p_total_tiles;
  a.nwaves = p_nwaves;
  a.grid = p_grid;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t nwaves = a.nwaves;
  const uint32_t nthreads = nwaves * 64u;
  const uint32_t gstride = a.grid * nwaves;
  uint8_t *stage = s_stage + wave * kStageBytes;
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s_lut);
#if MH_DIAG_STAMPS
  unsigned long long ts[kDiagSlots] = {};
#endif
  MH_STAMP(0);

  const uint32_t t0 = min(blockIdx.x * nwaves + wave, a.total_tiles);
  TileHdr hc;
  // ---- lookup table into LDS (shared by the workgroup) ----
  // A fixed count of unconditional 16-B loads per thread (chunks past the table fall
  // outside the descriptor and return 0), issued FIRST, all in flight together; the
  // first header follows. The table is stored and the workgroup barrier passed as soon
  // as the table's (L2) loads land -- an LDS-only barrier, so no wave waits there for
  // another wave's (HBM, cold) header. Round 3's loop of dependent copies, behind the
  // header, cost 3 L2 round trips plus the slowest header of the workgroup before the
  // first span could be staged (profiles/r04_v3_tile_start_ab.txt). A launch with a
  // prepared table has >= 5 waves per workgroup (smaller ones take the small-launch
  // kernel), so 4 loads per thread cover the table.
  constexpr uint32_t kLutChunks = kLutBytes / 16, kLutPer = 4;
  const bool fixed_copy = a.lut && nthreads * kLutPer >= kLutChunks;
  // The prepared table's [longest, shortest, flat8] word (mh_lut.hpp): the oldest load of
  // the wave (a vector load through the table's descriptor, empty without a prepared table),
  // so it has landed by the time the table's loads have and the decisions below cost the
  // copy no wait. (A scalar load needs a branch or a kernarg pointer to guard the no-table
  // case, and either waits for a scalar round trip before the table's loads go out.)
  const v4u32 lw = __builtin_amdgcn_raw_buffer_load_b128(
      uniform_rsrc(a.lut, a.lut ? (uint32_t)kPreparedBytes : 0u), kMaxLenOff, 0, 0);
  v4u32 L[kLutPer];
  {
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(a.lut, fixed_copy ? (uint32_t)kLutBytes : 0u);
#pragma unroll
    for (uint32_t k = 0; k < kLutPer; ++k)
      L[k] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)((threadIdx.x + k * nthreads) * 16u), 0, 0);
  }
  hdr_issue(a, t0, lane, hc);
  // The step flavour, from the prepared table's code lengths (kernel-uniform):
  //   2: one code length (flat), <= 13 bits -> escape-free step, swizzled stage
  //   1: no code over 13 bits               -> escape-free step
  //   0: general step (escapes), also for an in-kernel table and for a flat table of
  //      14- to 16-bit codes, whose every window escapes to the second level
  const uint32_t mx = a.lut ? __builtin_amdgcn_readfirstlane(lw.x) : 16u;
  const uint32_t mn = __builtin_amdgcn_readfirstlane(lw.y), f8 = __builtin_amdgcn_readfirstlane(lw.z);
  // A flat 8-bit identity table (code c = symbol c, the prepared table's flat8 word,
  // mh_lut.hpp) decodes by byte arithmetic with no table in LDS: no copy, no barrier. The
  // table's loads above were issued anyway (before the word is known) and land unused.
  // (The copy stays a block of its own in front of the flavour branch: with the branch
  // first, the compiler hoisted the loops' common header code above it, and the table
  // stores then waited for the header's HBM round trip -- vmcnt(0).)
  // (The stores themselves do not wait for the word: only the barrier does.)
  if (fixed_copy) {
    v4u32 *dstv = reinterpret_cast<v4u32 *>(s_lut);
#pragma unroll
    for (uint32_t k = 0; k < kLutPer; ++k)
      if (threadIdx.x + k * nthreads < kLutChunks) dstv[threadIdx.x + k * nthreads] = L[k];
    if (!f8) lds_barrier();
  } else if (a.lut && !f8) {
    const v4u32 *src = reinterpret_cast<const v4u32 *>(a.lut);
    v4u32 *dstv = reinterpret_cast<v4u32 *>(s_lut);
    for (uint32_t i = threadIdx.x; i < kLutChunks; i += nthreads) dstv[i] = src[i];
  }

  // the escape-free flavours need a prepared table, so a full fixed copy (>= 5 waves)
  const uint32_t flavor = !fixed_copy ? 0u : mx > (uint32_t)kLutBits ? 0u : mx == mn ? 2u : 1u;
  if (f8)
    flat8_loop<kDelta>(a, lane, stage, lut, t0, gstride, hc MH_TS_ARG);
  else if (flavor == 1)
    batch_loop<kDelta, Lut13NoEsc>(a, lane, stage, lut, t0, gstride, hc, true MH_TS_ARG);
  else if (flavor == 2)
    batch_loop<kDelta, Lut13Flat>(a, lane, stage, lut, t0, gstride, hc, true MH_TS_ARG);
  else
    batch_loop<kDelta, Lut13>(a, lane, stage, lut, t0, gstride, hc, fixed_copy MH_TS_ARG);
#if MH_DIAG_STAMPS
  MH_STAMP(5);
  __builtin_amdgcn_s_waitcnt(0);
  MH_STAMP(6);
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // HW_REG_XCC_ID[3:0]
  ts[7] = ((unsigned long long)xcc << 48) | ((unsigned long long)__smid() << 32) | blockIdx.x;
  const uint32_t gw = blockIdx.x * nwaves + wave;
  if (lane == 0 && gw < (uint32_t)kDiagWaves)
    for (int i = 0; i < kDiagSlots; ++i) g_stamps[gw * kDiagSlots + i] = ts[i];
#endif
}

#if !MH_LANE_PAIRS
// ---- a batch decoded straight from canonical headers (mh_decode_headers) ---------
// The 13-bit table is a pure function of the header's 256 code lengths, so a workgroup
// builds it in LDS itself: no table launch, no prepared buffer, no trip of the table
// through memory.
//
// Canonical codes are ordered by (length, symbol), so in the 16-bit window space the
// codes of length l fill [F[l], F[l+1]) with F[l+1] = F[l] + (count[l] << (16 - l)) -- the
// recurrence code = (code + count) << 1 of mh_tables.hip left-justified -- and windows at
// or above F[17] match no code. A window's code length is therefore 1 + the number of
// boundaries F[2..17] at or below it (16 compares against wave-uniform values), and its
// symbol is sorted[base[l] + (window >> (16 - l))], `sorted` the symbols in (length,
// symbol) order and base[l] = (symbols shorter than l) - first[l].
//
// The builder's scratch lives in the staging windows, which are idle until the first span
// is written behind the table's barrier.
struct HeaderScratch {
  uint32_t wcnt[4][16];  // codes of length l (index l - 1) among symbols 64 w .. 64 w + 63
  uint32_t too_long[4];  // wave w saw a length over 16
  int32_t base[16];
  uint8_t sorted[256];
};
static_assert(33 * 128 + 64 <= kStageBytes, "decode_halves' 33-lane pass fits the staging window");
static_assert(sizeof(HeaderScratch) <= kStageBytes, "the builder's scratch fits one staging window");

struct HeaderFacts {
  uint32_t mx, mn, flat8;  // the prepared table's lengths word (mh_lut.hpp, mh_tables.hip's sampling rule)
  int32_t status;          // MH_OK, MH_ERR_CODE_TOO_LONG or MH_ERR_TABLE, as mh_build_tables_device
};

// The 13-bit table (first level, escapes from P0, second level: mh_lut.hpp) of one header
// into `lut`, by a workgroup of 8 waves; L: symbol tid's code length (threads >= 256: 0).
// Every thread returns the same facts. A rejected header returns behind the first barrier
// with `lut` untouched; so does the flat 8-bit identity code when `skip_flat8` (it decodes
// without a table). Otherwise the caller's barrier follows the fill.
__device__ __forceinline__ HeaderFacts header_build(uint32_t L, uint16_t *lut, HeaderScratch *sc, uint32_t tid,
                                                    bool skip_flat8) {
  const uint32_t lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // codes per length and each symbol's rank among equal lengths: one ballot per length per wave
  uint32_t in_wave = 0;
  if (wave < 4) {
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t tl = __ballot(L > 16);
    uint32_t mine = 0;
    for (uint32_t l = 1; l <= 16; ++l) {
      const uint64_t m = __ballot(L == l);
      if (L == l) in_wave = (uint32_t)__popcll(m & below);
      if (lane == l - 1) mine = (uint32_t)__popcll(m);
    }
    if (lane < 16) sc->wcnt[wave][lane] = mine;
    if (lane == 16) sc->too_long[wave] = tl != 0;
  }
  lds_barrier();
  // every wave for itself, lane l - 1 for length l: the count, the left-justified first code
  // F[l] (exclusive prefix sum of count << (16 - l)) and the symbols shorter than l
  const uint32_t li = lane & 15u, sh = 15u - li;
  const uint32_t cnt = lane < 16 ? sc->wcnt[0][li] + sc->wcnt[1][li] + sc->wcnt[2][li] + sc->wcnt[3][li] : 0u;
  const uint32_t v = cnt << sh;
  uint32_t incl = v, upto = cnt;
#pragma unroll
  for (uint32_t d = 1; d < 16; d <<= 1) {
    const uint32_t y = __shfl_up(incl, d), z = __shfl_up(upto, d);
    if (lane >= d) {
      incl += y;
      upto += z;
    }
  }
  const uint32_t F = incl - v, shorter = upto - cnt;
  const uint32_t kraft = __builtin_amdgcn_readlane(incl, 15);
  const bool too_long = __ballot(sc->too_long[lane & 3u] != 0u) != 0;
  HeaderFacts hf;
  hf.status = too_long ? MH_ERR_CODE_TOO_LONG : kraft > 65536u ? MH_ERR_TABLE : MH_OK;
  // longest / shortest code as mh_prepare_lut samples them (windows at multiples of 4): a
  // length counts when one of its codes starts there -- the k-th code of length l starts at
  // F + (k << (16 - l)), and F is a multiple of 4 up to 14 bits
  const uint32_t seen = (uint32_t)__ballot(lane < 16 && cnt > (((0u - F) & 3u) >> sh)) & 0xFFFFu;
  hf.mx = seen ? 32u - (uint32_t)__clz(seen) : 0u;
  hf.mn = seen ? (uint32_t)__ffs(seen) : 255u;
  hf.flat8 = __builtin_amdgcn_readlane(cnt, 7) == 256u;  // all 256 symbols at 8 bits: code c = symbol c
  if (hf.status != MH_OK) {
    hf.mx = 0;
    hf.mn = 255;
    hf.flat8 = 0;
    return hf;
  }
  if (skip_flat8 && hf.flat8) return hf;
  // P0: the first 13-bit prefix of a code longer than 13 bits
  const uint32_t longs = (uint32_t)__ballot(lane < 16 && lane >= (uint32_t)kLutBits && cnt != 0u);
  const uint32_t P0 = longs ? __builtin_amdgcn_readlane(F, __ffs(longs) - 1) >> kL2Bits : (uint32_t)kL1Entries;
  uint32_t E[16];  // F[2..17], wave-uniform
#pragma unroll
  for (int i = 0; i < 16; ++i) E[i] = __builtin_amdgcn_readlane(incl, i);
  if (wave < 4) {
    const uint32_t lx = (L - 1u) & 15u;
    uint32_t pos = __shfl(shorter, lx) + in_wave;
    for (uint32_t w = 0; w < wave; ++w) pos += sc->wcnt[w][lx];
    if (L) sc->sorted[pos & 255u] = (uint8_t)tid;
  }
  if (tid < 16) sc->base[tid] = (int32_t)(shorter - (F >> sh));
  lds_barrier();
  // the step word of a 16-bit window (0: no code matches, the zero-width entry)
  const auto entry = [&](uint32_t w, uint32_t len) -> uint32_t {
    const uint32_t lc = min(len, 16u);
    const uint32_t pos = (uint32_t)(sc->base[lc - 1u] + (int32_t)(w >> (16u - lc))) & 255u;
    const uint32_t sym = sc->sorted[pos];
    return len > 16u ? 0u : ((sym << 8) - len) & 0xFFFFu;
  };
  const auto length_of = [&](uint32_t w) -> uint32_t {
    uint32_t len = 1;
#pragma unroll
    for (int i = 0; i < 16; ++i) len += (uint32_t)(w >= E[i]);
    return len;
  };
  const auto pack8 = [](const uint32_t (&x)[8]) -> v4u32 {
    v4u32 o;
    o.x = x[0] | (x[1] << 16);
    o.y = x[2] | (x[3] << 16);
    o.z = x[4] | (x[5] << 16);
    o.w = x[6] | (x[7] << 16);
    return o;
  };
  v4u32 *lutv = reinterpret_cast<v4u32 *>(lut);
  // First level: each thread owns two 16-byte chunks (8 prefixes = 64 windows each). A code
  // of <= 10 bits covers the whole chunk (one 16-byte store of its step word); a chunk that
  // no code reaches is zero; only chunks among the 11-13-bit codes or across P0 resolve
  // their entries one by one.
  constexpr uint32_t kL1Chunks = (uint32_t)kL1Entries / 8u;
  static_assert(kL1Chunks == 2u * 64u * kMaxWavesPerWG, "two first-level chunks per thread");
#pragma unroll 1
  for (uint32_t c = tid; c < kL1Chunks; c += 64u * kMaxWavesPerWG) {
    const uint32_t w0 = c << 6, len0 = length_of(w0);
    v4u32 o;
    if (len0 <= 10u) {
      const uint32_t e = entry(w0, len0), e2 = e | (e << 16);
      o.x = o.y = o.z = o.w = e2;
    } else if (len0 > 16u && P0 == (uint32_t)kL1Entries) {
      o.x = o.y = o.z = o.w = 0u;
    } else {
      uint32_t x[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t p = c * 8u + j, sub = p - P0 + 1u;
        const uint32_t w = p << kL2Bits;
        const uint32_t e = entry(w, length_of(w));
        x[j] = p >= P0 ? (sub < (uint32_t)kL2Subtables ? sub : 0u) : e;
      }
      o = pack8(x);
    }
    lutv[c] = o;
  }
  // Second level (130 chunks: subtable 0, <= 128 long-code prefixes, padding), on the last
  // threads -- the first four waves did the ballots
  constexpr uint32_t kL2Chunks = (uint32_t)(kLutEntries - kL1Entries) / 8u;
  const uint32_t j2 = 64u * kMaxWavesPerWG - 1u - tid;
  if (j2 < kL2Chunks) {
    const uint32_t nl2 = ((uint32_t)kL1Entries - P0) << kL2Bits;
    v4u32 o;
    o.x = o.y = o.z = o.w = 0u;
    if (j2 >= 1u && j2 < (uint32_t)kL2Subtables && (j2 - 1u) * 8u < nl2) {
      uint32_t x[8];
#pragma unroll
      for (uint32_t i = 0; i < 8; ++i) {
        const uint32_t w = (P0 << kL2Bits) + (j2 - 1u) * 8u + i;
        x[i] = entry(w, length_of(w));
      }
      o = pack8(x);
    }
    lutv[kL1Chunks + j2] = o;
  }
  return hf;
}

// ---- one frame slice per workgroup (mh_decode_frames / _headers / _region* / _windows* / _crops) --
// The batch kernel's machinery with another decomposition, shared by seven entries:
// workgroup g serves ONE frame, f = g / G, as slice j = g % G of it, so it brings frame f's
// table into LDS once and never crosses a frame. Wave w decodes the frame's tiles j*8 + w,
// stepping by 8*G: the persistent loops run on a workgroup-local DecodeArgs whose total_tiles
// is the workgroup's last tile + 1. Always 8 waves; waves without a tile idle behind the
// barrier. The step flavour comes from the frame's own [longest, shortest, flat8] facts, per
// workgroup. A frame whose status word is non-zero (rejected by the encoder or the table
// build) is left alone: the workgroup returns before any store. The grid is n_frames * G, not
// persistent across frames (DESIGN.md sections 3b-3d).
//
// Two things vary. The tile map:
//   FrameMap:  tiles count through the batch, f*tpf + j*8 + w below (f+1)*tpf (frame_of's
//              one-frame shortcut then holds for f = 0 only, where it is right; every other
//              frame divides).
//   RegionMap: runs of <= 64 blocks inside one block row of the region, stored into a raster of
//              the region's own size. Tiles are frame relative (the map carries the frame), so no
//              tile -> frame division; the tile -> (row, segment) division is skipped for regions
//              of <= 64 blocks per row.
//   WindowMap: a RegionMap per workgroup (mh_decode_windows): frame and origin from the window's
//              descriptor, the raster slot the window's index; behind the status load it writes the
//              window's status word (the frame's), so a skipped frame's windows carry it.
//   CropMap:   a WindowMap at a pixel origin (mh_decode_crops): tiles step by 63 blocks, and the
//              output stage (CropRows) moves every row onto the crop's byte grid.
// And where the 13-bit table comes from (a table source: `lut_of`, `issue`, `into_lds`):
//   PreparedTable: frame f's prepared table at luts + f * stride (stride 0: one table for all
//              frames), copied by four 16-byte loads per thread.
//   HeaderTable: built in LDS from frame f's 256 code lengths (header_build); slice 0 of every
//              frame that is not skipped by its status word writes the header's verdict, and a
//              rejected header returns before any store to the raster.
// Every load of the prologue is a vector load through a descriptor, issued oldest first: the
// status word (empty descriptor without a status array), the source's loads, the first tile
// header. So each has landed by the time the table's loads have (as the batch kernel's lengths
// word), and the barrier behind the table is LDS-only: no wave waits there for another wave's
// (HBM, cold) header.
struct TableFacts {
  uint32_t mx, mn, flat8;  // the prepared table's lengths word (mh_lut.hpp)
};

struct PreparedTable {
  const uint8_t *luts;
  uint64_t stride;
  static constexpr uint32_t kLutChunks = kLutBytes / 16, kLutPer = 4, kThreads = 64u * kMaxWavesPerWG;
  static_assert(kThreads * kLutPer >= kLutChunks, "four loads per thread cover the table");
  struct Loads {
    v4u32 lw, L[kLutPer];
  };
  __device__ __forceinline__ const uint16_t *lut_of(uint32_t f) const {
    return reinterpret_cast<const uint16_t *>(luts + (uint64_t)f * stride);
  }
  // the table's lengths word, then the table (from a.lut: the pointer is formed once, ahead of the status load)
  __device__ __forceinline__ void issue(const DecodeArgs &a, uint32_t, Loads &ld) const {
    ld.lw = __builtin_amdgcn_raw_buffer_load_b128(uniform_rsrc(a.lut, (uint32_t)kPreparedBytes), kMaxLenOff, 0, 0);
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(a.lut, (uint32_t)kLutBytes);
#pragma unroll
    for (uint32_t k = 0; k < kLutPer; ++k)
      ld.L[k] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)((threadIdx.x + k * kThreads) * 16u), 0, 0);
  }
  __device__ __forceinline__ bool into_lds(const Loads &ld, uint32_t, uint32_t, TableFacts &tf) const {
    tf.mx = __builtin_amdgcn_readfirstlane(ld.lw.x);
    tf.mn = __builtin_amdgcn_readfirstlane(ld.lw.y);
    tf.flat8 = __builtin_amdgcn_readfirstlane(ld.lw.z);
    v4u32 *dstv = reinterpret_cast<v4u32 *>(s_lut);
#pragma unroll
    for (uint32_t k = 0; k < kLutPer; ++k)
      if (threadIdx.x + k * kThreads < kLutChunks) dstv[threadIdx.x + k * kThreads] = ld.L[k];
    if (!tf.flat8) lds_barrier();  // the flat 8-bit identity table decodes without the table in LDS
    return true;
  }
};

struct HeaderTable {
  const uint8_t *headers;
  int32_t *verdict;
  struct Loads {
    uint32_t L;
  };
  __device__ __forceinline__ const uint16_t *lut_of(uint32_t) const { return nullptr; }
  // the frame's code lengths (threads past 255 read out of range: 0)
  __device__ __forceinline__ void issue(const DecodeArgs &, uint32_t f, Loads &ld) const {
    ld.L = __builtin_amdgcn_raw_buffer_load_b8(uniform_rsrc(headers + (uint64_t)f * 256u, 256u), (int)threadIdx.x,
                                               0, 0) & 0xFFu;
  }
  __device__ __forceinline__ bool into_lds(const Loads &ld, uint32_t f, uint32_t slice, TableFacts &tf) const {
    const HeaderFacts hf = header_build(ld.L, s_lut, reinterpret_cast<HeaderScratch *>(s_stage), threadIdx.x, true);
    if (verdict && slice == 0 && threadIdx.x == 0) verdict[f] = hf.status;
    if (hf.status != MH_OK) return false;  // workgroup-uniform: a rejected header, no store to the raster
    lds_barrier();  // the table is complete, and nobody reads the scratch in the staging windows any more
    tf = TableFacts{hf.mx, hf.mn, hf.flat8};
    return true;
  }
};

template <bool kDelta, class Out = StoreRows, class Map, class Src>
__device__ __forceinline__ void slice_decode(const DecodeArgs &a0, const uint32_t *p_offsets,
                                             const uint64_t *p_frame_off, const uint8_t *p_block_init,
                                             const int32_t *p_status, uint32_t p_nb, uint32_t p_tiles_per_frame,
                                             uint32_t G, uint32_t f, uint32_t slice, const Src &src, const Map &m) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  DecodeArgs a = a0;
  a.offsets = p_offsets;
  a.frame_off = p_frame_off;
  a.block_init = p_block_init;
  a.lut = src.lut_of(f);
  a.nb = p_nb;
  a.tiles_per_frame = p_tiles_per_frame;
  // this workgroup's tiles end with its frame
  if constexpr (Map::kOwnTiles)
    a.total_tiles = p_tiles_per_frame;  // a set's frame: tiles from its own block 0
  else
    a.total_tiles = Map::kRegion ? p_tiles_per_frame : (f + 1u) * p_tiles_per_frame;
  constexpr uint32_t nwaves = kMaxWavesPerWG;
  a.nwaves = nwaves;
  a.grid = G;
  const uint32_t gstride = G * nwaves;
  uint8_t *stage = s_stage + wave * kStageBytes;
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s_lut);
#if MH_DIAG_STAMPS
  unsigned long long ts[kDiagSlots] = {};
#endif
  MH_STAMP(0);

  uint32_t t0;
  if constexpr (Map::kOwnTiles)
    t0 = min(slice * nwaves + wave, a.total_tiles);
  else
    t0 = min((Map::kRegion ? 0u : f * p_tiles_per_frame) + slice * nwaves + wave, a.total_tiles);
  TileHdrOf<Map> hc;
  const uint32_t stv = __builtin_amdgcn_raw_buffer_load_b32(
      uniform_rsrc(p_status ? (const void *)(p_status + f) : (const void *)p_offsets, p_status ? 4u : 0u), 0, 0, 0);
  typename Src::Loads ld;
  src.issue(a, f, ld);
  hdr_issue<Map>(a, t0, lane, hc, m);
  const uint32_t st = __builtin_amdgcn_readfirstlane(stv);
  m.report(st, slice);  // WindowMap: the window's status word
  if (st != 0u) return;  // workgroup-uniform: a skipped frame, nothing stored
  TableFacts tf;
  if (!src.into_lds(ld, f, slice, tf)) return;
  if (tf.flat8)
    flat8_loop<kDelta, Map, Out>(a, lane, stage, lut, t0, gstride, hc MH_TS_ARG, m);
  else if (tf.mx == tf.mn && tf.mx <= (uint32_t)kLutBits)
    batch_loop<kDelta, Lut13Flat, Map, Out>(a, lane, stage, lut, t0, gstride, hc, true MH_TS_ARG, m);
  else if (tf.mx <= (uint32_t)kLutBits)
    batch_loop<kDelta, Lut13NoEsc, Map, Out>(a, lane, stage, lut, t0, gstride, hc, true MH_TS_ARG, m);
  else
    batch_loop<kDelta, Lut13, Map, Out>(a, lane, stage, lut, t0, gstride, hc, true MH_TS_ARG, m);
}

// The seven kernels (eleven with the scales, each in a raw and a delta instantiation: the rows of
// kSliceTable): names, launch bounds and argument order are the ABI of the launchers, the ISA
// guard and the diagnostic scripts; the leading 16 arguments are preloaded into SGPRs.
template <bool kDelta>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_multitable_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, uint64_t p_lut_stride, uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_groups,
    const DecodeArgs a0) {
  const uint32_t f = blockIdx.x / p_groups, slice = blockIdx.x - f * p_groups;
  slice_decode<kDelta>(a0, p_offsets, p_frame_off, p_block_init, p_status, p_nb, p_tiles_per_frame, p_groups, f, slice,
                       PreparedTable{p_luts, p_lut_stride}, FrameMap{});
}

template <bool kDelta>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_region_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, uint64_t p_lut_stride, uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_groups,
    uint32_t p_segs, uint32_t p_rbw, uint32_t p_rbx0, uint32_t p_rby0, const DecodeArgs a0) {
  const uint32_t f = blockIdx.x / p_groups, slice = blockIdx.x - f * p_groups;
  slice_decode<kDelta>(a0, p_offsets, p_frame_off, p_block_init, p_status, p_nb, p_tiles_per_frame, p_groups, f, slice,
                       PreparedTable{p_luts, p_lut_stride}, RegionMap{f, p_rbx0, p_rby0, p_rbw, p_segs});
}

// BoxRows' edge word (RegionMap::rem): the frame's pixels from an accepted origin on
__device__ __forceinline__ uint32_t box_rem(uint32_t W, uint32_t H, uint32_t bx0, uint32_t by0) {
  return (W - 8u * bx0) | ((H - 8u * by0) << 16);
}

// ... and the region at scale 2^kLog2 (kLog2 = 1..3): the region kernel with the BoxRows output stage
template <bool kDelta, int kLog2>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_region_scaled_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, uint64_t p_lut_stride, uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_groups,
    uint32_t p_segs, uint32_t p_rbw, uint32_t p_rbx0, uint32_t p_rby0, const DecodeArgs a0) {
  const uint32_t f = blockIdx.x / p_groups, slice = blockIdx.x - f * p_groups;
  slice_decode<kDelta, BoxRows<kLog2>>(a0, p_offsets, p_frame_off, p_block_init, p_status, p_nb, p_tiles_per_frame,
                                       p_groups, f, slice, PreparedTable{p_luts, p_lut_stride},
                                       RegionMap{f, p_rbx0, p_rby0, p_rbw, p_segs,
                                                 box_rem(a0.w, a0.h, p_rbx0, p_rby0)});
}

// ---- the list entries' steps (mh_decode_windows* / _crops* / _set_crops*) -------------------------
// A list kernel is an entry in front of slice_decode: workgroup g serves unit g / G of the list, reads
// the unit's 16-byte descriptor, judges it by itself before anything is addressed through it, and
// makes the workgroup's own DecodeArgs and map. Each step is written once here; a kernel below is
// the steps it takes, in its order, and a comment on what it adds ("The list
// entries' steps"). The kernels sit at the SGPR ceiling, so a step that makes a value opaque says
// what was lost without it, and the opaque statements keep their order within a kernel.

// unit -> (list index, slice)
struct ListUnit {
  uint32_t p, slice;
};
__device__ __forceinline__ ListUnit list_unit(uint32_t groups) {
  const uint32_t p = blockIdx.x / groups;
  return {p, blockIdx.x - p * groups};
}
// ... and for samples of planes, unit = (sample, plane): (sample p, plane c, slice). One plane skips
// the division (uniform), as region_rs does for one segment.
struct PlaneUnit {
  uint32_t p, c, slice;
};
__device__ __forceinline__ PlaneUnit plane_unit(uint32_t groups, uint32_t n_planes) {
  const ListUnit u = list_unit(groups);
  uint32_t p = u.p, c = 0u;
  if (n_planes != 1u) {
    p = u.p / n_planes;
    c = u.p - p * n_planes;
  }
  return {p, c, u.slice};
}

// The unit's 16-byte descriptor, wave-uniform: the one dependent trip ahead of slice_decode's prologue.
__device__ __forceinline__ v4u32 desc_load(const void *desc) {
  v4u32 d = __builtin_amdgcn_raw_buffer_load_b128(uniform_rsrc(desc, 16u), 0, 0, 0);
  d.x = __builtin_amdgcn_readfirstlane(d.x), d.y = __builtin_amdgcn_readfirstlane(d.y);
  d.z = __builtin_amdgcn_readfirstlane(d.z), d.w = __builtin_amdgcn_readfirstlane(d.w);
  return d;
}

// A rejected descriptor (workgroup-uniform): MH_ERR_DIMS into the unit's status word, which one thread
// writes -- `writer`: slice 0's first, of plane 0 for a sample -- and the kernel returns having loaded
// nothing through the descriptor and stored nothing else. (The kernel forms `writer`: formed in a
// helper it becomes one vector compare, and the delta windows kernel's SGPR count moves.)
__device__ __forceinline__ void list_reject(int32_t *status, uint32_t p, bool writer) {
  if (status && writer) status[p] = MH_ERR_DIMS;
}

// The verdict on a descriptor's own words (frame | origin | flags), true = rejected. The origin is
// compared with the last one that fits, max_x0 = W - w and max_y0 = H - h from the host (which has
// checked w <= W and h <= H; blocks for windows, pixels for crops), so no sum of descriptor values
// is formed and nothing wraps; the limits arrive with the other scalars, ahead of the descriptor.
// `no_frame` is the entry's own frame rule. Word 3 may hold the bits `flag_bits` (none: a reserved
// word, zero), and MH_CROP_MIRROR is refused on a width that is no multiple of 8 (odd_w = 1, from
// the host: a mirrored row would carry its unspecified tail at its front).
__device__ __forceinline__ bool mirror_bad(uint32_t flags, uint32_t odd_w) { return (flags & odd_w) != 0u; }
__device__ __forceinline__ bool desc_bad(const v4u32 d, bool no_frame, uint32_t max_x0, uint32_t max_y0,
                                         uint32_t flag_bits = 0u, uint32_t odd_w = 0u) {
  return no_frame | (d.y > max_x0) | (d.z > max_y0) | ((d.w & ~flag_bits) != 0u) | mirror_bad(d.w, odd_w);
}

// The slot folded into the raster's base, the slot stride 0 from then on: raster_slot() * 0 is no
// instruction, and the slot index lives no longer than report(). The scaled windows' body has no
// SGPR to spare for it (raw pixels at 1/4 scale spilled with it), and neither have the crops'.
__device__ __forceinline__ DecodeArgs slot_args(const DecodeArgs &a0, uint8_t *base) {
  DecodeArgs a = a0;
  a.out = base;
  a.out_frame_stride = 0;
  return a;
}
__device__ __forceinline__ DecodeArgs slot_args(const DecodeArgs &a0, uint32_t p) {
  return slot_args(a0, a0.out + (uint64_t)p * a0.out_frame_stride);
}

// The rows of a window that lie inside the frame: its row limit, in place of a0.out_frame_bytes.
__device__ __forceinline__ uint32_t window_rows(uint32_t H, uint32_t by0, uint32_t bh) {
  return min(H, 8u * (by0 + bh)) - 8u * by0;
}

// A crop's own geometry, from an accepted origin: the block rows it touches -- (dy + h + 7) >> 3 of
// them, at most the CBH the grid was sized for (p_tiles_per_crop, the grid's worst case, is not used),
// so the workgroup's tiles end with its last needed block row and a row the crop does not reach
// (which may lie outside the frame) is never addressed --, the blocks a row touches (NB), and the
// packed dx | flags << 3 | dy << 4 | OW << 8 of the output stage (CropMap, NormMap).
struct CropGeom {
  uint32_t rows, nblk, rem;
};
__device__ __forceinline__ CropGeom crop_geom(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags = 0u) {
  const uint32_t dx = x0 & 7u, dy = y0 & 7u;
  const uint32_t rows = (dy + h + 7u) >> 3, nblk = (dx + w + 7u) >> 3, ow = (w + 7u) >> 3;
  return {rows, nblk, dx | (flags << 3) | (dy << 4) | (ow << 8)};
}
// ... under NormRows, `rem` one opaque word: seen through, its parts stay live beside it and the
// raw-pixel body is an SGPR short
__device__ __forceinline__ CropGeom norm_geom(uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags) {
  CropGeom g = crop_geom(x0, y0, w, h, flags);
  asm volatile("" : "+s"(g.rem));
  return g;
}

// NormRows' byte selector (mirrored or not), scale and bias: per-lane and opaque (NormMap)
struct NormConsts {
  uint32_t sel;
  float scale, bias;
};
__device__ __forceinline__ NormConsts norm_consts(uint32_t flags, float scale, float bias) {
  NormConsts n{flags ? 0x04050607u : 0x03020100u, scale, bias};
  asm volatile("" : "+v"(n.sel), "+v"(n.scale), "+v"(n.bias));
  return n;
}

// mh_decode_windows: window g / G's frame and block origin from its descriptor, the slot the
// window's index (WindowMap reports the frame's status word into the window's). a0.out_frame_stride
// is the window stride.
template <bool kDelta>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_windows_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const mh_window *p_windows, uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_groups,
    uint32_t p_segs, uint32_t p_rbw, uint32_t p_rbh, uint32_t p_nframes, uint32_t p_max_bx0, uint32_t p_max_by0,
    uint64_t p_lut_stride, int32_t *p_wstatus, const DecodeArgs a0) {
  const ListUnit u = list_unit(p_groups);
  const v4u32 wd = desc_load(p_windows + u.p);
  const uint32_t f = wd.x, bx0 = wd.y, by0 = wd.z;
  if (desc_bad(wd, f >= p_nframes, p_max_bx0, p_max_by0)) 
    return list_reject(p_wstatus, u.p, u.slice == 0 && threadIdx.x == 0);
  DecodeArgs aw = a0;
  aw.out_frame_bytes = (uint64_t)window_rows(a0.h, by0, p_rbh) * a0.out_pitch;
  slice_decode<kDelta>(aw, p_offsets, p_frame_off, p_block_init, p_status, p_nb, p_tiles_per_frame, p_groups, f,
                       u.slice, PreparedTable{p_luts, p_lut_stride},
                       WindowMap{{f, bx0, by0, p_rbw, p_segs}, u.p, p_wstatus});
}

// ... and the windows at scale 2^kLog2 (kLog2 = 1..3): the BoxRows output stage, so the window's edge
// word and its row limit SH_p * pitch, formed behind the verdict from the accepted origin only, and
// the slot folded into the base.
template <bool kDelta, int kLog2>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_windows_scaled_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const mh_window *p_windows, uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_groups,
    uint32_t p_segs, uint32_t p_rbw, uint32_t p_rbh, uint32_t p_nframes, uint32_t p_max_bx0, uint32_t p_max_by0,
    uint64_t p_lut_stride, int32_t *p_wstatus, const DecodeArgs a0) {
  const ListUnit u = list_unit(p_groups);
  const v4u32 wd = desc_load(p_windows + u.p);
  const uint32_t f = wd.x, bx0 = wd.y, by0 = wd.z;
  if (desc_bad(wd, f >= p_nframes, p_max_bx0, p_max_by0)) 
    return list_reject(p_wstatus, u.p, u.slice == 0 && threadIdx.x == 0);
  constexpr uint32_t s = 1u << kLog2;
  DecodeArgs aw = slot_args(a0, u.p);
  aw.out_frame_bytes = (uint64_t)((window_rows(a0.h, by0, p_rbh) + s - 1u) >> kLog2) * a0.out_pitch;
  slice_decode<kDelta, BoxRows<kLog2>>(
      aw, p_offsets, p_frame_off, p_block_init, p_status, p_nb, p_tiles_per_frame, p_groups, f, u.slice,
      PreparedTable{p_luts, p_lut_stride},
      WindowMap{{f, bx0, by0, p_rbw, p_segs, box_rem(a0.w, a0.h, bx0, by0)}, u.p, p_wstatus});
}

// mh_decode_crops: crop g / G, a w x h rectangle at a PIXEL origin: the windows' verdict in pixels,
// then the crop's own tiles and the CropRows output stage. a0.out_frame_bytes is h * pitch, every
// crop's row limit; a0.out_frame_stride is the crop stride.
template <bool kDelta>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_crops_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const mh_crop *p_crops, uint32_t p_nb, uint32_t p_tiles_per_crop, uint32_t p_groups,
    uint32_t p_segs, uint32_t p_w, uint32_t p_h, uint32_t p_nframes, uint32_t p_max_x0, uint32_t p_max_y0,
    uint64_t p_lut_stride, int32_t *p_cstatus, const DecodeArgs a0) {
  const ListUnit u = list_unit(p_groups);
  const v4u32 cd = desc_load(p_crops + u.p);
  const uint32_t f = cd.x, x0 = cd.y, y0 = cd.z;
  if (desc_bad(cd, f >= p_nframes, p_max_x0, p_max_y0))
    return list_reject(p_cstatus, u.p, u.slice == 0 && threadIdx.x == 0);
  const CropGeom g = crop_geom(x0, y0, p_w, p_h);
  const DecodeArgs ac = slot_args(a0, u.p);
  slice_decode<kDelta, CropRows>(ac, p_offsets, p_frame_off, p_block_init, p_status, p_nb, g.rows * p_segs, p_groups,
                                 f, u.slice, PreparedTable{p_luts, p_lut_stride},
                                 CropMap{{{f, x0 >> 3, y0 >> 3, g.nblk, p_segs, g.rem}, u.p, p_cstatus}});
}

// mh_decode_crops_norm: the crops' entry with the flags word in the verdict and the NormRows<kFmt>
// output stage. a0.out_pitch / out_frame_stride / out_frame_bytes are bytes of the wide raster.
template <bool kDelta, uint32_t kFmt>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_normcrops_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const mh_norm_crop *p_crops, uint32_t p_nb, uint32_t p_tiles_per_crop, uint32_t p_groups,
    uint32_t p_segs, uint32_t p_w, uint32_t p_h, uint32_t p_nframes, uint32_t p_max_x0, uint32_t p_max_y0,
    uint64_t p_lut_stride, int32_t *p_cstatus, float p_scale, float p_bias, uint32_t p_odd_w, const DecodeArgs a0) {
  const ListUnit u = list_unit(p_groups);
  const v4u32 cd = desc_load(p_crops + u.p);
  const uint32_t f = cd.x, x0 = cd.y, y0 = cd.z, flags = cd.w;
  if (desc_bad(cd, f >= p_nframes, p_max_x0, p_max_y0, MH_CROP_MIRROR, p_odd_w))
    return list_reject(p_cstatus, u.p, u.slice == 0 && threadIdx.x == 0);
  const DecodeArgs ac = slot_args(a0, u.p);
  const NormConsts nc = norm_consts(flags, p_scale, p_bias);
  const CropGeom g = norm_geom(x0, y0, p_w, p_h, flags);
  slice_decode<kDelta, NormRows<kFmt>>(
      ac, p_offsets, p_frame_off, p_block_init, p_status, p_nb, g.rows * p_segs, p_groups, f, u.slice,
      PreparedTable{p_luts, p_lut_stride},
      NormMap{{{{f, x0 >> 3, y0 >> 3, g.nblk, p_segs, g.rem}, u.p, p_cstatus}}, nc.sel, nc.scale, nc.bias});
}

// mh_decode_crops_norm_planes: a descriptor is a SAMPLE of n_planes planes, plane c the same crop of
// frame f + c * frame_stride under its own (scale[c], bias[c]), stored out_stride bytes behind plane
// c - 1. Workgroup g serves unit g / G = (sample, plane). What a plane changes is workgroup-constant
// and made ahead of slice_decode: the frame (and with it the table), the raster's base and the
// stage's per-lane (scale, bias). The body, the maps and NormRows are the normalised crops'. The
// verdict is that kernel's with the frame compared against p_max_frame = n_frames - 1 -
// (n_planes - 1) * frame_stride from the host, so the sample's LAST plane names a frame and no sum
// of descriptor words is formed ahead of it.
struct PlaneArgs {
  uint32_t n_planes, frame_stride;
  uint64_t out_stride;
  float scale[MH_MAX_PLANES], bias[MH_MAX_PLANES];
};
// ... plane c's NormRows constants (pl by value: its eight words are loaded, then selected)
__device__ __forceinline__ NormConsts plane_consts(uint32_t flags, const PlaneArgs pl, uint32_t c) {
  return norm_consts(flags, c == 0u ? pl.scale[0] : c == 1u ? pl.scale[1] : c == 2u ? pl.scale[2] : pl.scale[3],
                     c == 0u ? pl.bias[0] : c == 1u ? pl.bias[1] : c == 2u ? pl.bias[2] : pl.bias[3]);
}
// A sample is written whole or not at all: every one of its workgroups loads the status words of all
// its frames (workgroup-uniform, empty descriptors for the planes past n_planes and without a status
// array; f0 + (n_planes - 1) * frame_stride < n_frames has passed), so all reach one decision -- the
// first non-zero word in plane order -- and the body gets no status pointer. plane_verdict writes
// the sample's status word, by plane 0's slice 0.
struct PlaneStatus {
  uint32_t w[MH_MAX_PLANES];
};
__device__ __forceinline__ PlaneStatus plane_status_issue(const int32_t *status, const void *any, uint32_t f0,
                                                          const PlaneArgs &pl) {
  PlaneStatus s;
#pragma unroll
  for (uint32_t i = 0; i < MH_MAX_PLANES; ++i) {
    const bool on = status && i < pl.n_planes;
    s.w[i] = __builtin_amdgcn_raw_buffer_load_b32(
        uniform_rsrc(on ? (const void *)(status + f0 + (uint64_t)i * pl.frame_stride) : any, on ? 4u : 0u), 0, 0, 0);
  }
  return s;
}
__device__ __forceinline__ uint32_t plane_verdict(const PlaneStatus &s, int32_t *status, uint32_t p, bool writer) {
  uint32_t st = 0u;
#pragma unroll
  for (int i = MH_MAX_PLANES - 1; i >= 0; --i) {
    const uint32_t w = __builtin_amdgcn_readfirstlane(s.w[i]);
    st = w ? w : st;
  }
  if (status && writer) status[p] = (int32_t)st;
  return st;
}
// The plane's frame and raster base, opaque from here on: seen through, the sums' terms stay live
// beside them through the body, and the raw 16-bit instantiations spilled three VGPRs.
struct PlaneSlot {
  uint32_t f;
  uint8_t *out;
};
__device__ __forceinline__ PlaneSlot plane_slot(const DecodeArgs &a0, const PlaneArgs &pl, uint32_t f0, uint32_t p,
                                                uint32_t c) {
  uint32_t f = f0 + c * pl.frame_stride;
  const uint64_t base = (uint64_t)a0.out + (uint64_t)p * a0.out_frame_stride + (uint64_t)c * pl.out_stride;
  uint32_t base_lo = (uint32_t)base, base_hi = (uint32_t)(base >> 32);
  asm volatile("" : "+s"(f), "+s"(base_lo), "+s"(base_hi));
  return {f, (uint8_t *)(((uint64_t)base_hi << 32) | base_lo)};
}

template <bool kDelta, uint32_t kFmt>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_planes_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const mh_norm_crop *p_crops, uint32_t p_nb, uint32_t p_tiles_per_crop, uint32_t p_groups,
    uint32_t p_segs, uint32_t p_w, uint32_t p_h, uint32_t p_max_frame, uint32_t p_max_x0, uint32_t p_max_y0,
    uint64_t p_lut_stride, int32_t *p_cstatus, uint32_t p_odd_w, const PlaneArgs pl, const DecodeArgs a0) {
  const PlaneUnit u = plane_unit(p_groups, pl.n_planes);
  const v4u32 cd = desc_load(p_crops + u.p);
  const uint32_t f0 = cd.x, x0 = cd.y, y0 = cd.z, flags = cd.w;
  const bool writer = u.c == 0u && u.slice == 0u && threadIdx.x == 0u;
  if (desc_bad(cd, f0 > p_max_frame, p_max_x0, p_max_y0, MH_CROP_MIRROR, p_odd_w))
    return list_reject(p_cstatus, u.p, writer);
  // workgroup-uniform: a skipped sample, no plane of it is stored
  if (plane_verdict(plane_status_issue(p_status, p_offsets, f0, pl), p_cstatus, u.p, writer) != 0u) return;
  const PlaneSlot ps = plane_slot(a0, pl, f0, u.p, u.c);
  const DecodeArgs ac = slot_args(a0, ps.out);
  const NormConsts nc = plane_consts(flags, pl, u.c);
  const CropGeom g = norm_geom(x0, y0, p_w, p_h, flags);
  slice_decode<kDelta, NormRows<kFmt>>(
      ac, p_offsets, p_frame_off, p_block_init, nullptr, p_nb, g.rows * p_segs, p_groups, ps.f, u.slice,
      PreparedTable{p_luts, p_lut_stride},
      NormMap{{{{ps.f, x0 >> 3, y0 >> 3, g.nblk, p_segs, g.rem}, 0u, nullptr}}, nc.sel, nc.scale, nc.bias});
}

// The crop entries over a frame SET (mh_decode_set_crops, mh_decode_set_crops_norm_planes): frames of
// different sizes, frame f's geometry in the 16-byte record p_geoms[f]. The entry is its parent's with
// a second dependent trip: desc_load and the verdict on the descriptor's own words; only then the
// record (geom_load, wave-uniform as desc_load) and the verdict on it (geom_bad); then the crop
// against the frame's own W_f x H_f (set_fit_bad). Behind the verdicts the workgroup's DecodeArgs get
// the frame's own grid (set_frame): bw, nb and the two arrays based at the frame's first block
// (first_block <= total_blocks - nb has passed, so the sums stay inside the arrays; the maps'
// kOwnBase makes hdr_issue add nothing to them). The offsets descriptor stays limited to the frame's
// nb * 4 bytes, so a frame's last block takes the min(fbits, off + 1024) end and never reads a
// neighbour's first offset. Codes, table and status word stay indexed by the frame number.
// p_total_blocks arrives where the parents' p_nb does; p_max_x0 / p_max_y0 (from the set's maxima)
// are not used.
__device__ __forceinline__ v4u32 geom_load(const mh_frame_geom *geoms, uint32_t f, bool on = true) {
  // off: a descriptor of zero records, whose load returns 0 without touching memory
  v4u32 d = __builtin_amdgcn_raw_buffer_load_b128(
      uniform_rsrc(on ? (const void *)(geoms + f) : (const void *)geoms, on ? 16u : 0u), 0, 0, 0);
  d.x = __builtin_amdgcn_readfirstlane(d.x), d.y = __builtin_amdgcn_readfirstlane(d.y);
  d.z = __builtin_amdgcn_readfirstlane(d.z), d.w = __builtin_amdgcn_readfirstlane(d.w);
  return d;
}
// the record's own verdict (step 2): true = rejected
__device__ __forceinline__ bool geom_bad(const v4u32 g, uint32_t total_blocks) {
  const uint32_t W = g.y, H = g.z;
  const uint32_t nb = ((W + 7u) >> 3) * ((H + 7u) >> 3);  // <= 2^26 for an accepted W, H
  return (g.w != 0u) | (W - 1u > 65534u) | (H - 1u > 65534u) | (nb > total_blocks) | (g.x > total_blocks - nb);
}
// the crop against the accepted record's W x H (step 3); the limits are formed from the record, and
// the sizes are judged first: a wrapped limit is never the verdict
__device__ __forceinline__ bool set_fit_bad(const v4u32 d, uint32_t W, uint32_t H, uint32_t w, uint32_t h) {
  return (w > W) | (h > H) | (d.y > W - w) | (d.z > H - h);
}
// The frame's grid and bases, opaque from here on: seen through, the record's words stay live beside
// them through the body, which has no SGPR to spare.
struct SetFrame {
  const uint32_t *offsets;
  const uint8_t *block_init;
  uint32_t bw, nb;
};
__device__ __forceinline__ SetFrame set_frame(const uint32_t *p_offsets, const uint8_t *p_block_init, uint32_t first,
                                              uint32_t W, uint32_t H) {
  uint32_t bw = (W + 7u) >> 3;
  uint32_t nb = bw * ((H + 7u) >> 3);
  const uint64_t o = (uint64_t)p_offsets + 4ull * first;
  const uint64_t i = p_block_init ? (uint64_t)p_block_init + first : 0ull;
  uint32_t o_lo = (uint32_t)o, o_hi = (uint32_t)(o >> 32), i_lo = (uint32_t)i, i_hi = (uint32_t)(i >> 32);
  asm volatile("" : "+s"(bw), "+s"(nb), "+s"(o_lo), "+s"(o_hi), "+s"(i_lo), "+s"(i_hi));
  return {(const uint32_t *)(((uint64_t)o_hi << 32) | o_lo), (const uint8_t *)(((uint64_t)i_hi << 32) | i_lo), bw, nb};
}

template <bool kDelta>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_setcrops_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const mh_crop *p_crops, uint32_t p_total_blocks, uint32_t p_tiles_per_crop,
    uint32_t p_groups, uint32_t p_segs, uint32_t p_w, uint32_t p_h, uint32_t p_nframes, uint32_t p_max_x0,
    uint32_t p_max_y0, uint64_t p_lut_stride, int32_t *p_cstatus, const mh_frame_geom *p_geoms, const DecodeArgs a0) {
  const ListUnit u = list_unit(p_groups);
  const v4u32 cd = desc_load(p_crops + u.p);
  const uint32_t f = cd.x, x0 = cd.y, y0 = cd.z;
  const bool writer = u.slice == 0 && threadIdx.x == 0;
  if (desc_bad(cd, f >= p_nframes, ~0u, ~0u)) return list_reject(p_cstatus, u.p, writer);
  const v4u32 gd = geom_load(p_geoms, f);
  if (geom_bad(gd, p_total_blocks)) return list_reject(p_cstatus, u.p, writer);
  const uint32_t W = gd.y, H = gd.z;
  if (set_fit_bad(cd, W, H, p_w, p_h)) return list_reject(p_cstatus, u.p, writer);
  const SetFrame sf = set_frame(p_offsets, p_block_init, gd.x, W, H);
  const CropGeom g = crop_geom(x0, y0, p_w, p_h);
  DecodeArgs ac = slot_args(a0, u.p);
  ac.bw = sf.bw;
  slice_decode<kDelta, CropRows>(
      ac, sf.offsets, p_frame_off, sf.block_init, p_status, sf.nb, g.rows * p_segs, p_groups, f, u.slice,
      PreparedTable{p_luts, p_lut_stride},
      SetCropMap{{{{f, x0 >> 3, y0 >> 3, g.nblk, p_segs, g.rem}, u.p, p_cstatus}}});
}

// ... and the samples of planes over a set. Step 2 covers the sample: every workgroup loads the
// records of all its n_planes frames (empty descriptors for the planes past n_planes, as the status
// words), judges each and requires every plane's (width, height) to equal plane 0's, so all the
// sample's workgroups reach one verdict. The status words depend on the descriptor alone and are
// loaded in the same trip; they are read behind the geometry's verdict, which keeps its precedence.
template <bool kDelta, uint32_t kFmt>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_setplanes_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const mh_norm_crop *p_crops, uint32_t p_total_blocks, uint32_t p_tiles_per_crop,
    uint32_t p_groups, uint32_t p_segs, uint32_t p_w, uint32_t p_h, uint32_t p_max_frame, uint32_t p_max_x0,
    uint32_t p_max_y0, uint64_t p_lut_stride, int32_t *p_cstatus, uint32_t p_odd_w, const PlaneArgs pl,
    const mh_frame_geom *p_geoms, const DecodeArgs a0) {
  const PlaneUnit u = plane_unit(p_groups, pl.n_planes);
  const v4u32 cd = desc_load(p_crops + u.p);
  const uint32_t f0 = cd.x, x0 = cd.y, y0 = cd.z, flags = cd.w;
  const bool writer = u.c == 0u && u.slice == 0u && threadIdx.x == 0u;
  if (desc_bad(cd, f0 > p_max_frame, ~0u, ~0u, MH_CROP_MIRROR)) return list_reject(p_cstatus, u.p, writer);
  v4u32 gd[MH_MAX_PLANES];
#pragma unroll
  for (uint32_t i = 0; i < MH_MAX_PLANES; ++i) gd[i] = geom_load(p_geoms, f0 + i * pl.frame_stride, i < pl.n_planes);
  const PlaneStatus stv = plane_status_issue(p_status, p_offsets, f0, pl);
  const uint32_t W = gd[0].y, H = gd[0].z;
  bool bad = false;
  uint32_t first = gd[0].x;  // this workgroup's plane's
#pragma unroll
  for (uint32_t i = 0; i < MH_MAX_PLANES; ++i) {
    const bool on = i < pl.n_planes;
    bad |= on & (geom_bad(gd[i], p_total_blocks) | (gd[i].y != W) | (gd[i].z != H));
    first = u.c == i ? gd[i].x : first;
  }
  if (bad) return list_reject(p_cstatus, u.p, writer);
  if (set_fit_bad(cd, W, H, p_w, p_h) | mirror_bad(flags, p_odd_w)) return list_reject(p_cstatus, u.p, writer);
  if (plane_verdict(stv, p_cstatus, u.p, writer) != 0u) return;  // a skipped sample, as the planes entry's
  const SetFrame sf = set_frame(p_offsets, p_block_init, first, W, H);
  const PlaneSlot ps = plane_slot(a0, pl, f0, u.p, u.c);
  DecodeArgs ac = slot_args(a0, ps.out);
  ac.bw = sf.bw;
  const NormConsts nc = plane_consts(flags, pl, u.c);
  const CropGeom g = norm_geom(x0, y0, p_w, p_h, flags);
  slice_decode<kDelta, NormRows<kFmt>>(
      ac, sf.offsets, p_frame_off, sf.block_init, nullptr, sf.nb, g.rows * p_segs, p_groups, ps.f, u.slice,
      PreparedTable{p_luts, p_lut_stride},
      SetNormMap{{{{{ps.f, x0 >> 3, y0 >> 3, g.nblk, p_segs, g.rem}, 0u, nullptr}}, nc.sel, nc.scale, nc.bias}});
}

// mh_decode_set_frames: every frame of a set whole, each at its own size into its own raster. The
// grid is a list of workgroups, not of units of one size: workgroup g reads its frame number from
// the group map (one trip), then the frame's three 16-byte records, which depend on f alone (the
// second trip, as the set crops'): the geometry (geom_load / geom_bad), the share {first_group,
// groups, 0, 0} that says which slice of the frame g is, and the raster {offset, pitch, 0} that says
// where the frame is written. The slice count of a frame lives in its one share record, so the
// frame's workgroups cannot disagree about it. Verdicts, each before anything is addressed through
// what it judges:
//   map word >= n_frames                       -> return, nothing written;
//   share: reserved != 0, groups == 0 or > 2^20 (no frame has more tiles; it keeps G * 8 and every
//     tile sum far from 2^32), g outside [first_group, first_group + groups)
//                                              -> return, nothing written (not a workgroup of f);
//   geometry rejected                          -> MH_ERR_DIMS;
//   raster: reserved != 0, offset or pitch not a multiple of 8, pitch < round_up(W, 8) or > 2^20
//     (every entry's pitch limit: a lane's row offset stays below 2^31), or the last row's end
//     offset + (H - 1) pitch + round_up(W, 8) past out_bytes, formed so that nothing wraps
//                                              -> MH_ERR_CAPACITY.
// The two codes go to d_set_status[f] by slice 0's first thread; behind them SetFrameMap::report
// writes the frame's status word there (0: MH_OK). A corrupt share or map can lose or repeat tiles of
// its own frame only: offsets and block_init stay inside the frame's accepted [first, first + nb),
// every store inside the accepted raster.
__device__ __forceinline__ bool share_bad(const v4u32 s, uint32_t g) {
  return ((s.z | s.w) != 0u) | (s.y - 1u > 0xFFFFFu) | (g < s.x) | (g - s.x >= s.y);
}
__device__ __forceinline__ bool raster_bad(const v4u32 r, uint32_t W, uint32_t H, uint64_t out_bytes) {
  const uint64_t offset = ((uint64_t)r.y << 32) | r.x;
  const uint32_t pitch = r.z, rw = (W + 7u) & ~7u;
  const uint64_t tail = (uint64_t)(H - 1u) * pitch + rw;  // < 2^16 * 2^32 + 2^16
  return (r.w != 0u) | (((r.x | pitch) & 7u) != 0u) | (pitch < rw) | (pitch > (1u << 20)) | (tail > out_bytes) |
         (offset > out_bytes - tail);
}
__device__ __forceinline__ void set_reject(int32_t *status, uint32_t f, bool writer, int32_t code) {
  if (status && writer) status[f] = code;
}
// The frame's raster, opaque as set_frame's values and for the same reason.
struct SetRaster {
  uint8_t *out;
  uint32_t pitch;
  uint64_t bytes;  // H * pitch
};
__device__ __forceinline__ SetRaster set_raster(uint8_t *out, const v4u32 r, uint32_t H) {
  const uint64_t o = (uint64_t)out + (((uint64_t)r.y << 32) | r.x), n = (uint64_t)H * r.z;
  uint32_t o_lo = (uint32_t)o, o_hi = (uint32_t)(o >> 32), n_lo = (uint32_t)n, n_hi = (uint32_t)(n >> 32), pitch = r.z;
  asm volatile("" : "+s"(o_lo), "+s"(o_hi), "+s"(n_lo), "+s"(n_hi), "+s"(pitch));
  return {(uint8_t *)(((uint64_t)o_hi << 32) | o_lo), pitch, ((uint64_t)n_hi << 32) | n_lo};
}

template <bool kDelta>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_setframes_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_luts,
    const int32_t *p_status, const uint32_t *p_group_frame, uint32_t p_total_blocks, uint32_t p_nframes,
    uint64_t p_lut_stride, int32_t *p_sstatus, const mh_frame_geom *p_geoms, const mh_set_raster *p_rasters,
    const mh_set_share *p_shares, uint64_t p_out_bytes, const DecodeArgs a0) {
  const uint32_t g = blockIdx.x;
  const uint32_t f = __builtin_amdgcn_readfirstlane(
      __builtin_amdgcn_raw_buffer_load_b32(uniform_rsrc(p_group_frame + g, 4u), 0, 0, 0));
  if (f >= p_nframes) return;
  const v4u32 gd = geom_load(p_geoms, f);
  const v4u32 sd = desc_load(p_shares + f);
  const v4u32 rd = desc_load(p_rasters + f);
  if (share_bad(sd, g)) return;
  const uint32_t slice = g - sd.x, G = sd.y;
  const bool writer = slice == 0u && threadIdx.x == 0u;
  if (geom_bad(gd, p_total_blocks)) return set_reject(p_sstatus, f, writer, MH_ERR_DIMS);
  const uint32_t W = gd.y, H = gd.z;
  if (raster_bad(rd, W, H, p_out_bytes)) return set_reject(p_sstatus, f, writer, MH_ERR_CAPACITY);
  const SetFrame sf = set_frame(p_offsets, p_block_init, gd.x, W, H);
  const SetRaster sr = set_raster(a0.out, rd, H);
  DecodeArgs af = slot_args(a0, sr.out);
  af.w = W;
  af.h = H;
  af.bw = sf.bw;
  af.bh = (H + 7u) >> 3;
  af.out_pitch = sr.pitch;
  af.out_frame_bytes = sr.bytes;
  slice_decode<kDelta>(af, sf.offsets, p_frame_off, sf.block_init, p_status, sf.nb, (sf.nb + 63u) >> 6, G, f, slice,
                       PreparedTable{p_luts, p_lut_stride}, SetFrameMap{f, p_sstatus});
}

template <bool kDelta>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG, kMinWavesPerEU) mh_decode_headers_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint8_t *p_headers,
    const int32_t *p_status, int32_t *p_header_status, uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_groups,
    const DecodeArgs a0) {
  const uint32_t f = blockIdx.x / p_groups, slice = blockIdx.x - f * p_groups;
  slice_decode<kDelta>(a0, p_offsets, p_frame_off, p_block_init, p_status, p_nb, p_tiles_per_frame, p_groups, f, slice,
                       HeaderTable{p_headers, p_header_status}, FrameMap{});
}

// mh_header_luts_device: header_build's table and facts copied out at their prepared-table
// offsets, one workgroup per header, so a test can compare them with mh_build_luts_device's.
__global__ void __launch_bounds__(64 * kMaxWavesPerWG) mh_header_luts_kernel(const uint8_t *headers, uint8_t *luts,
                                                                             uint64_t lut_stride, int32_t *status) {
  const uint32_t hdr = blockIdx.x, tid = threadIdx.x;
  const uint32_t L = tid < 256u ? headers[(uint64_t)hdr * 256u + tid] : 0u;
  const HeaderFacts hf = header_build(L, s_lut, reinterpret_cast<HeaderScratch *>(s_stage), tid, false);
  __syncthreads();
  uint8_t *dst = luts + (uint64_t)hdr * lut_stride;
  const v4u32 *src = reinterpret_cast<const v4u32 *>(s_lut);
  v4u32 zero;
  zero.x = zero.y = zero.z = zero.w = 0u;
  for (uint32_t i = tid; i < (uint32_t)kLutBytes / 16u; i += blockDim.x)
    reinterpret_cast<v4u32 *>(dst)[i] = hf.status == MH_OK ? src[i] : zero;
  if (tid < 4)
    reinterpret_cast<uint32_t *>(dst + kMaxLenOff)[tid] = tid == 0 ? hf.mx : tid == 1 ? hf.mn : tid == 2 ? hf.flat8 : 0u;
  if (status && tid == 0) status[hdr] = hf.status;
}

// ---- the reference walk, one frame slice per workgroup (mh_check_frames / mh_check_headers) ------
// mh_check's report for a batch that brings a table per frame: the decomposition, the prologue and
// the table sources of slice_decode (workgroup g = frame g / G, slice g % G; the frame's table in
// LDS once), but every lane does the REFERENCE walk of its block (include/metalhuffman.h, mh_frame):
// 64 steps from offsets[b] over the slot's real bytes, zero at or past the slot's end, whatever the
// offsets are. Nothing is staged: a staged span is cut by the tile's recorded ends, which is what
// makes the decoders differ from the reference on unspecified blocks.
//
// Code bits: the lane reads aligned dwords of its frame's slot through a descriptor that covers the
// slot's whole dwords (a load is inside or outside as a whole); the slot's last 1..3 bytes come from
// byte loads through a descriptor of the slot's exact size, once per wave, and stand in for the dword
// they start (`tail`). kWalkGroup steps consume at most 16 * kWalkGroup bits, so the dwords a group
// can touch are the kWalkWords from the one its first bit lies in: their addresses depend on the
// group's start only, and all are issued before the first step. Inside the group they form a queue,
// q[0] the dword of the cursor's bit `o` (0..31); a step crosses at most one dword boundary (a code
// has at most 16 bits), where the queue moves up by one. Positions are 64 bits: an offset near 2^32
// plus 1,024 bits does not fit 32.
//
// A wave keeps its lanes' zero-width count, mismatches and first offending block in registers over
// all its tiles, reduces across lanes once, and lane 0 issues at most two atomic adds, one atomic min
// and the verdict's store (word [1], the truncated-T2 count, stays 0: a prepared or header-built
// table has no truncated T2). No workgroup waits for another.
constexpr int kWalkGroup = 8;
constexpr int kWalkWords = (31 + 16 * kWalkGroup + 31) / 32;  // 5
static_assert(64 % kWalkGroup == 0, "a block's 64 steps in whole groups");

struct WalkSlot {
  __amdgpu_buffer_rsrc_t words;  // the slot's whole dwords
  uint32_t tail_idx, tail;       // the dword the slot's last 1..3 bytes start, and those bytes (big-endian)
  uint64_t bits;                 // 8 x the slot's bytes
};

__device__ __forceinline__ uint32_t walk_word(const WalkSlot &sl, uint32_t idx) {
  return bswap32(__builtin_amdgcn_raw_buffer_load_b32(sl.words, (int)(idx * 4u), 0, 0));
}

// The step word of the 32 bits `w32` at the cursor: the 13-bit first level, the second level for an
// entry in (0, kEscapeBelow). 0: no code matches, the zero-width step.
__device__ __forceinline__ uint32_t walk_lookup(const uint16_t *lut, uint32_t w32) {
  uint32_t e = lut[w32 >> (32 - kLutBits)];
  if (e - 1u < kEscapeBelow - 1u)
    e = lut[(uint32_t)kL1Entries + e * (1u << kL2Bits) + ((w32 >> 16) & ((1u << kL2Bits) - 1u))];
  return e;
}

// The steps among the kWalkGroup from bit start + adv that advance, one at a time with two loads
// each: the rare path of a group that ended stalled.
__device__ __forceinline__ uint32_t walk_advancing(const WalkSlot &sl, const uint16_t *lut, uint32_t start,
                                                   uint32_t adv) {
  uint32_t n = 0;
#pragma unroll 1
  for (; n < (uint32_t)kWalkGroup; ++n) {
    const uint64_t pos = (uint64_t)start + adv;
    const uint32_t i = (uint32_t)(pos >> 5), o = (uint32_t)pos & 31u;
    uint32_t q0 = walk_word(sl, i), q1 = walk_word(sl, i + 1u);
    q0 = i == sl.tail_idx ? sl.tail : q0;
    q1 = i + 1u == sl.tail_idx ? sl.tail : q1;
    const uint32_t e = walk_lookup(lut, (uint32_t)(((((uint64_t)q0 << 32) | q1) << o) >> 32));
    if (e == 0u) break;
    adv += (0u - e) & 0xFFu;
  }
  return n;
}

// The end of the block that starts at bit `start` (64 steps), and its zero-width lookups. A
// zero-width step does not advance, so the next step sees the same bits and is zero-width too: a
// stall lasts to the block's end. Only a group whose last step is zero-width holds any, and it is
// walked again, step by step, to find where they begin.
__device__ __forceinline__ uint64_t walk_block(const WalkSlot &sl, const uint16_t *lut, uint32_t start, uint32_t &zero) {
  uint32_t p = start;  // the cursor's low 32 bits; the walk adds at most 1,024 to the start
#pragma unroll 1
  for (int g = 0; g < 64 / kWalkGroup; ++g) {
    const uint32_t p0 = p;
    const uint32_t i0 = (uint32_t)(((uint64_t)start + (p - start)) >> 5);  // < 2^27 + 64: the byte offset fits 32 bits
    uint32_t q[kWalkWords + 1];
#pragma unroll
    for (int j = 0; j < kWalkWords; ++j) q[j] = walk_word(sl, i0 + (uint32_t)j);
    q[kWalkWords] = 0u;
    if (sl.tail_idx - i0 < (uint32_t)kWalkWords) {  // the group reaches the slot's last, partial dword
#pragma unroll
      for (int j = 0; j < kWalkWords; ++j) q[j] = i0 + (uint32_t)j == sl.tail_idx ? sl.tail : q[j];
    }
    uint32_t o = p & 31u, e = 0u;
#pragma unroll
    for (int k = 0; k < kWalkGroup; ++k) {
      e = walk_lookup(lut, (uint32_t)(((((uint64_t)q[0] << 32) | q[1]) << o) >> 32));  // 32 bits from the cursor
      p += (0u - e) & 0xFFu;  // the step word's width; entry 0: the zero-width step
      const uint32_t o2 = p & 31u;
      const bool up = o2 < o;  // a step is at most 16 bits: the low five bits wrap at most once
      o = o2;
#pragma unroll
      for (int j = 0; j < kWalkWords; ++j) q[j] = up ? q[j + 1] : q[j];
    }
    if (e == 0u) zero += (uint32_t)kWalkGroup - walk_advancing(sl, lut, start, p0 - start);
  }
  return (uint64_t)start + (p - start);
}

// The clean report and the passed-through status word of every frame, ahead of the walk.
__global__ void __launch_bounds__(256) mh_walk_init_kernel(const int32_t *status, uint32_t *report, int32_t *verdict,
                                                           uint32_t n_frames) {
  const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= 4ull * n_frames) return;
  report[i] = (i & 3u) == 3u ? 0xFFFFFFFFu : 0u;
  if (verdict && (i & 3u) == 0u) verdict[i >> 2] = status ? status[i >> 2] : MH_OK;
}

// HeaderTable whose rejection also reaches the check's verdict word (slice 0 writes both).
struct WalkHeaderTable : HeaderTable {
  int32_t *walk_verdict;
  __device__ __forceinline__ bool into_lds(const Loads &ld, uint32_t f, uint32_t slice, TableFacts &tf) const {
    const HeaderFacts hf = header_build(ld.L, s_lut, reinterpret_cast<HeaderScratch *>(s_stage), threadIdx.x, true);
    if (slice == 0 && threadIdx.x == 0) {
      if (verdict) verdict[f] = hf.status;
      if (walk_verdict && hf.status != MH_OK) walk_verdict[f] = hf.status;
    }
    if (hf.status != MH_OK) return false;
    lds_barrier();
    tf = TableFacts{hf.mx, hf.mn, hf.flat8};
    return true;
  }
};

template <bool kBatch, class Src>
__device__ __forceinline__ void slice_walk(const uint32_t *p_offsets, const uint64_t *p_frame_off,
                                           const uint8_t *p_codes, uint64_t p_codes_bytes, const int32_t *p_status,
                                           uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t G, uint32_t f,
                                           uint32_t slice, const Src &src, uint32_t *p_report, int32_t *p_verdict) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  DecodeArgs a = {};
  a.offsets = p_offsets;
  a.frame_off = kBatch ? p_frame_off : nullptr;
  a.lut = src.lut_of(f);
  a.nb = p_nb;
  a.tiles_per_frame = p_tiles_per_frame;
  a.total_tiles = (f + 1u) * p_tiles_per_frame;  // this workgroup's tiles end with its frame
  const uint32_t gstride = G * (uint32_t)kMaxWavesPerWG;
  uint32_t tile = min(f * p_tiles_per_frame + slice * (uint32_t)kMaxWavesPerWG + wave, a.total_tiles);
  // the prologue's loads, oldest first: the status word, the table, the first offsets
  TileHdr hc;
  const uint32_t stv = __builtin_amdgcn_raw_buffer_load_b32(
      uniform_rsrc(p_status ? (const void *)(p_status + f) : (const void *)p_offsets, p_status ? 4u : 0u), 0, 0, 0);
  typename Src::Loads ld;
  src.issue(a, f, ld);
  hdr_issue(a, tile, lane, hc);
  if (__builtin_amdgcn_readfirstlane(stv) != 0u) return;  // workgroup-uniform: not walked, the init launch's words stand
  TableFacts tf;
  if (!src.into_lds(ld, f, slice, tf)) return;  // a rejected header: not walked either
  if (tile >= a.total_tiles) return;            // no barrier below
  // the frame's slot
  uint64_t fbeg = 0, fbytes = p_codes_bytes;
  if constexpr (kBatch) {
    fbeg = ((uint64_t)__builtin_amdgcn_readlane(hc.fo_hi, 0) << 32) | __builtin_amdgcn_readlane(hc.fo_lo, 0);
    fbytes = (((uint64_t)__builtin_amdgcn_readlane(hc.fo_hi, 1) << 32) | __builtin_amdgcn_readlane(hc.fo_lo, 1)) - fbeg;
  }
  // no walk reads at or past byte 2^29 + 160, so a larger slot's descriptor may end at 0xFFFFFFF0
  const uint32_t fb32 = (uint32_t)(fbytes > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : fbytes);
  WalkSlot sl;
  sl.words = uniform_rsrc(p_codes + fbeg, fb32 & ~3u);
  sl.tail_idx = fb32 >> 2;
  sl.bits = fbytes * 8u;  // fbytes < 2^61
  {
    const __amdgpu_buffer_rsrc_t rb = uniform_rsrc(p_codes + fbeg, fb32);
    uint32_t t = 0;
#pragma unroll
    for (uint32_t k = 0; k < 3u; ++k)
      t |= (__builtin_amdgcn_raw_buffer_load_b8(rb, (int)((fb32 & ~3u) + k), 0, 0) & 0xFFu) << (24u - 8u * k);
    sl.tail = __builtin_amdgcn_readfirstlane(t);
  }
  uint32_t zero = 0, mism = 0, first = 0xFFFFFFFFu;
  while (tile < a.total_tiles) {
    const uint32_t b = (tile - f * p_tiles_per_frame) * 64u + lane;
    const uint32_t off = hc.off, nxt = hc.nxt;
    tile = __builtin_amdgcn_readfirstlane(min(tile + gstride, a.total_tiles));
    hdr_issue(a, tile, lane, hc);  // the next tile's offsets, behind this tile's walk
    if (b < p_nb) {                // lanes without a block contribute nothing
      uint32_t z = 0;
      // the flat 8-bit code has no table in LDS and needs none: every lookup is 8 bits wide
      const uint64_t end = tf.flat8 ? (uint64_t)off + 512u
                                    : walk_block(sl, reinterpret_cast<const uint16_t *>(s_lut), off, z);
      // the last block's end is not recorded: it must lie inside the slot
      const bool bad = b + 1u < p_nb ? end != (uint64_t)nxt : end > sl.bits;
      zero += z;
      mism += bad ? 1u : 0u;
      if (z | (uint32_t)bad) first = min(first, b);
    }
  }
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) {
    zero += (uint32_t)__shfl_xor(zero, d);
    mism += (uint32_t)__shfl_xor(mism, d);
    first = min(first, (uint32_t)__shfl_xor(first, d));
  }
  if (lane == 0 && first != 0xFFFFFFFFu) {
    uint32_t *r = p_report + 4ull * f;
    if (zero) atomicAdd(&r[0], zero);
    if (mism) atomicAdd(&r[2], mism);
    atomicMin(&r[3], first);
    if (p_verdict) p_verdict[f] = MH_ERR_STREAM;
  }
}

// The two walk kernels, each with (kBatch) and without a frame-offset array; the leading 16
// arguments are preloaded into SGPRs, as the decode kernels'.
template <bool kBatch>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG) mh_walk_frames_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_codes, const uint8_t *p_luts,
    const int32_t *p_status, uint64_t p_lut_stride, uint64_t p_codes_bytes, uint32_t p_nb,
    uint32_t p_tiles_per_frame, uint32_t p_groups, uint32_t *p_report, int32_t *p_verdict) {
  const uint32_t f = blockIdx.x / p_groups, slice = blockIdx.x - f * p_groups;
  slice_walk<kBatch>(p_offsets, p_frame_off, p_codes, p_codes_bytes, p_status, p_nb, p_tiles_per_frame, p_groups, f,
                     slice, PreparedTable{p_luts, p_lut_stride}, p_report, p_verdict);
}

template <bool kBatch>
__global__ void __launch_bounds__(64 * kMaxWavesPerWG) mh_walk_headers_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_codes, const uint8_t *p_headers,
    const int32_t *p_status, int32_t *p_header_status, uint64_t p_codes_bytes, uint32_t p_nb,
    uint32_t p_tiles_per_frame, uint32_t p_groups, uint32_t *p_report, int32_t *p_verdict) {
  const uint32_t f = blockIdx.x / p_groups, slice = blockIdx.x - f * p_groups;
  slice_walk<kBatch>(p_offsets, p_frame_off, p_codes, p_codes_bytes, p_status, p_nb, p_tiles_per_frame, p_groups, f,
                     slice, WalkHeaderTable{{p_headers, p_header_status}, p_verdict}, p_report, p_verdict);
}
#endif  // !MH_LANE_PAIRS

// ---- small launches (<= one wave per SIMD, e.g. one 2048x1536 frame) -------------
// Every wave decodes one tile, one wave per SIMD: the wave's own instruction stream
// (the per-symbol dependency chain and the instructions beside it), not LDS or VALU
// throughput, sets the time. When the table has no code longer than 14 bits the
// single-level 14-bit table drops the escape test. Workgroups of 4 waves (one per
// SIMD; 192 for a 2048x1536 frame) beat 8 (two waves per SIMD, fewer table copies):
// 5.74 vs 5.89 us (profiles/r01_v15_small_step_ab.txt).
// Two entries share the decode (small_decode): mh_decode_frame_kernel for one frame without
// a frame-offset array, mh_decode_small_kernel for every other small launch.
constexpr int kSmallWaves = 4;  // waves per workgroup (one tile each)
constexpr int kSmallMaxTilesPerCU = 4;   // launches up to this many tiles per CU
__shared__ __attribute__((aligned(16))) uint16_t s_lut_small[kLut14Entries];  // 14-bit, or 13-bit L1+L2
static_assert(kLutBytes <= kLut14Bytes, "the 13-bit table fits the small kernel's LUT space");

// the small kernels' step flavours (all with write-through row stores)
using Small14 = StepCfg<kLut14Bits, false, false, false, kSmallStoreAux, true>;
using Small13 = StepCfg<kLutBits, false, true, false, kSmallStoreAux, true>;
using SmallFlat8 = StepCfg<kLutBits, false, false, false, kSmallStoreAux, false, true>;

#if MH_DIAG_STAMPS
// Diagnostic builds: a small-launch wave's stamps behind its decode (slots 4 to 7) and their write.
// c3: the core clock at stamp 3 (MH_DIAG_CLOCK); rowv: the row clocks (MH_DIAG_ROWS).
__device__ __forceinline__ void small_stamps(unsigned long long (&ts)[kDiagSlots], bool staged, unsigned long long c3,
                                             uint32_t lane, uint32_t gw, uint32_t rowv) {
  MH_STAMP(4);
#if MH_DIAG_CLOCK
  ts[5] = staged ? __builtin_amdgcn_s_memtime() - c3 : 0ull;  // core clocks of the decode
#elif !MH_DIAG_ARGS
  ts[5] = ts[4];
#endif
  __builtin_amdgcn_s_waitcnt(0);
  MH_STAMP(6);
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);  // HW_REG_XCC_ID[3:0]
  ts[7] = ((unsigned long long)xcc << 48) | ((unsigned long long)__smid() << 32) | blockIdx.x;
  if (lane == 0 && gw < (uint32_t)kDiagWaves)
    for (int i = 0; i < kDiagSlots; ++i) g_stamps[gw * kDiagSlots + i] = ts[i];
#if MH_DIAG_ROWS
  if (lane < (uint32_t)kDiagRowSlots && gw < (uint32_t)kDiagWaves) g_rows[gw * kDiagRowSlots + lane] = rowv;
#endif
  (void)staged;
  (void)c3;
  (void)rowv;
}
#endif

// The small-launch kernels' common tail, entered behind the table barrier with the tile's
// span in flight in R: stage it, decode the tile with the step flavour the lengths word
// picks (flat8 / l14, kernel-uniform), and (diagnostic builds) write the wave's stamps.
template <bool kDelta>
__device__ __forceinline__ void small_decode(const DecodeArgs &a, const Tile &t, uint32_t lane,
                                             const v4u32 (&R)[kStageChunks], bool live, bool staged, bool flat8,
                                             bool l14, uint8_t *stage, const uint8_t *lut, uint32_t gw MH_TS_PARAM) {
  if (!live) return;  // no barrier below
#if MH_DIAG_STAMPS && MH_DIAG_ARGS
  // slot 5: the output arguments are in registers (behind the kernarg segment's scalar
  // load where the kernel reads them from memory), in front of out_tile's divisions
  asm volatile("" ::"s"(a.out), "s"((uint32_t)a.out_pitch), "s"((uint32_t)a.out_frame_bytes), "s"(a.bw));
  MH_STAMP(5);
#endif
  const OutTile ot = out_tile(a, t, lane);
  const __amdgpu_buffer_rsrc_t out = ot.rsrc;
  const uint32_t row0 = ot.row0;
#if MH_DIAG_STAMPS
  unsigned long long c3 = 0;
  uint32_t rowv = 0;
#endif
#if MH_DIAG_ROWS
#define MH_ROWS_ARG , &rowv
#else
#define MH_ROWS_ARG
#endif
  // Code layout: the staged 14-bit chain (no code over 14 bits: the bench's frames) is the
  // fall-through behind the staging; the flat, escape and oversize flavours lie behind it, out
  // of its fetch path.
  if (__builtin_expect(staged, 1)) {
    span_write(t, lane, R, stage);
    wave_sync();
    MH_STAMP(3);
#if MH_DIAG_STAMPS && MH_DIAG_CLOCK
    c3 = __builtin_amdgcn_s_memtime();
#endif
    LdsWords src{stage};
    if (__builtin_expect(l14 && !flat8, 1))
      decode_block<kDelta, Small14>(src, lut, t.p, t.init, out, row0, (uint32_t)a.out_pitch, !t.valid MH_ROWS_ARG);
    else if (flat8)
      decode_block<kDelta, SmallFlat8>(src, lut, t.p, t.init, out, row0, (uint32_t)a.out_pitch, !t.valid);
    else
      decode_block<kDelta, Small13>(src, lut, t.p, t.init, out, row0, (uint32_t)a.out_pitch, !t.valid MH_ROWS_ARG);
  } else if (flat8) {
    decode_halves<kDelta, SmallFlat8>(a, t, lane, lut, stage, out, row0, !t.valid);
  } else if (l14) {
    decode_halves<kDelta, Small14>(a, t, lane, lut, stage, out, row0, !t.valid);
  } else {
    decode_halves<kDelta, Small13>(a, t, lane, lut, stage, out, row0, !t.valid);
  }
#if MH_DIAG_STAMPS
  small_stamps(ts, staged, c3, lane, gw, rowv);
#else
  (void)gw;
#endif
#undef MH_ROWS_ARG
}

template <bool kDelta>
// The kernel arguments the first loads depend on come first, as scalars: the code object
// preloads the leading kernarg dwords into SGPRs at wave launch (amdgpu-kernarg-preload,
// build.py), so the block-offset and table loads issue without waiting for a scalar load
// of the kernarg segment; the rest of DecodeArgs is read from memory behind them.
__global__ void __launch_bounds__(64 * kSmallWaves) mh_decode_small_kernel(
    const uint32_t *p_offsets, const uint64_t *p_frame_off, const uint8_t *p_block_init, const uint16_t *p_lut,
    uint32_t p_nb, uint32_t p_tiles_per_frame, uint32_t p_total_tiles, const DecodeArgs a0) {
  DecodeArgs a = a0;
  a.offsets = p_offsets;
  a.frame_off = p_frame_off;
  a.block_init = p_block_init;
  a.lut = p_lut;
  a.nb = p_nb;
  a.tiles_per_frame = p_tiles_per_frame;
  a.total_tiles = p_total_tiles;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t nwaves = kSmallWaves;  // launched with kSmallWaves waves per workgroup
  uint8_t *stage = s_stage + wave * kStageBytes;
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s_lut_small);
  const uint8_t *prepared = reinterpret_cast<const uint8_t *>(a.lut);
#if MH_DIAG_STAMPS
  unsigned long long ts[kDiagSlots] = {};
#endif
  MH_STAMP(0);

  // [longest code, shortest code, flat8] (mh_lut.hpp): one scalar load, first used behind
  // the header's loads
  const v4u32 lens = *reinterpret_cast<const v4u32 *>(prepared + kMaxLenOff);
  const uint32_t max_len = lens.x;
  const uint32_t tile = min(blockIdx.x * nwaves + wave, a.total_tiles);
  TileHdr h;
  hdr_issue(a, tile, lane, h);
  const bool l14 = max_len <= (uint32_t)kLut14Bits;
  // Table copy: a fixed count of unconditional 16-B loads per thread (chunks past
  // the table fall outside the descriptor), issued behind the offsets so that the
  // offsets wait below is an exact vmcnt leaving the table loads in flight; the
  // table's L2 round trip overlaps the offsets' HBM one.
  constexpr int kLutLoads = kLut14Bytes / 16 / (64 * kSmallWaves);  // 8
  static_assert(kLut14Bytes == kLutLoads * 16 * 64 * kSmallWaves, "whole table per pass");
  v4u32 L[kLutLoads];
  {
    const __amdgpu_buffer_rsrc_t rl =
        uniform_rsrc(prepared + (l14 ? kLut14Off : 0), l14 ? (uint32_t)kLut14Bytes : (uint32_t)kLutBytes);
#pragma unroll
    for (int k = 0; k < kLutLoads; ++k)
      L[k] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)((threadIdx.x + 64u * kSmallWaves * k) * 16u), 0, 0);
  }
  const Tile t = hdr_resolve(a, h, lane);
  MH_STAMP(1);
  const bool live = t.tile < a.total_tiles;
  const bool staged = live && t.span <= (uint32_t)kStageBytes;
  v4u32 R[kStageChunks];
  span_issue(a, t, lane, R, staged);
  {
    v4u32 *dst = reinterpret_cast<v4u32 *>(s_lut_small);
#pragma unroll
    for (int k = 0; k < kLutLoads; ++k) dst[threadIdx.x + 64u * kSmallWaves * k] = L[k];
  }
  // table in LDS: an LDS-only barrier (waits lgkmcnt, not vmcnt), so no wave waits here
  // for another wave's span (HBM, cold); each waits for its own span at its first read.
  // (Skipping the copy and barrier for flat tables put a branch on the lengths word in
  // front of the header's loads, which then waited for its scalar round trip: config 2
  // +4 %, the flat single frame gains nothing worth it.)
  lds_barrier();
  MH_STAMP(2);
  // a flat 8-bit identity table (code c = symbol c; the builder sets the word only when
  // every first-level entry says so): byte arithmetic from the staged span (kernel-uniform)
  small_decode<kDelta>(a, t, lane, R, live, staged, lens.z != 0u, l14, stage, lut,
                       blockIdx.x * nwaves + wave MH_TS_ARG);
}

// ---- one frame, prepared table, no frame-offset array: the single-frame entry ----
// The same decode as mh_decode_small_kernel with no scalar round trip on the wave's
// start path:
//   * the whole argument list is 14 dwords -- five pointers, then four dwords, no
//     padding -- which is what the kernarg preload holds (16 user SGPRs less the
//     kernarg pointer), so every argument is in an SGPR at wave launch and the kernel
//     never reads the kernarg segment. Everything else is derived: tiles from nb,
//     out_frame_bytes = h * pitch. launch() bounds what the narrow fields hold
//     (codes_bytes <= 0xFFFFFFF0 and pitch <= 2^20 in mh_decode, bw <= 8192,
//     h <= MH_MAX_DIM = 65535);
//   * the table's loads do not wait for the lengths word: the 14-bit table is loaded
//     unconditionally right behind the offsets; the word (scalar loads issued at entry)
//     is first read behind the span's loads and the table's LDS stores. A table with a code
//     over 14 bits (kernel-uniform, rare) then copies the 13-bit two-level table over
//     the 14-bit one before the barrier -- each thread overwrites only chunks it wrote
//     itself, and a wave's LDS stores stay in order.
// Waits before / after: profiles/frame_entry_prologue_waits.txt; stamps and A/B against
// mh_decode_small_kernel: profiles/frame_entry_stamps.txt, frame_entry_ab.txt.
constexpr uint32_t kFrameBwShift = 16;  // p_bw_h = bw << 16 | h
static_assert(MH_MAX_DIM <= 0xFFFFu && (MH_MAX_DIM + 7) / 8 < (1u << (32 - kFrameBwShift)),
              "bw and h share one dword");
template <bool kDelta>
__global__ void __launch_bounds__(64 * kSmallWaves) mh_decode_frame_kernel(
    const uint32_t *p_offsets, const uint16_t *p_lut, const uint8_t *p_codes, uint8_t *p_out,
    const uint8_t *p_block_init, uint32_t p_nb, uint32_t p_codes_bytes, uint32_t p_pitch, uint32_t p_bw_h) {
  DecodeArgs a{};  // t1 / t2 / frame_off stay null: the body reads none of them with a prepared table
  a.offsets = p_offsets;
  a.lut = p_lut;
  a.codes = p_codes;
  a.out = p_out;
  a.block_init = p_block_init;
  a.nb = p_nb;
  a.codes_bytes = p_codes_bytes;
  a.out_pitch = p_pitch;
  a.bw = p_bw_h >> kFrameBwShift;
  a.h = p_bw_h & ((1u << kFrameBwShift) - 1u);
  a.out_frame_bytes = (uint64_t)a.h * p_pitch;
  a.tiles_per_frame = a.total_tiles = (p_nb + 63u) / 64u;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  constexpr uint32_t nwaves = kSmallWaves;
  uint8_t *stage = s_stage + wave * kStageBytes;
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s_lut_small);
  const uint8_t *prepared = reinterpret_cast<const uint8_t *>(a.lut);
#if MH_DIAG_STAMPS
  unsigned long long ts[kDiagSlots] = {};
#endif
  MH_STAMP(0);

  // [longest code, shortest code, flat8] (mh_lut.hpp): the two words used, as two scalar
  // loads read below. (One 4-word load leaves two result registers dead; the compiler
  // reuses one and waits for the load before writing it -- in front of the span's loads.)
  const uint32_t *lens = reinterpret_cast<const uint32_t *>(prepared + kMaxLenOff);
  const uint32_t max_len = lens[0], flat8 = lens[2];
  const uint32_t tile = min(blockIdx.x * nwaves + wave, a.total_tiles);
  TileHdr h;
  hdr_issue(a, tile, lane, h);
  constexpr int kLutLoads = kLut14Bytes / 16 / (64 * kSmallWaves);  // 8
  static_assert(kLut14Bytes == kLutLoads * 16 * 64 * kSmallWaves, "whole table per pass");
  v4u32 L[kLutLoads];
  {
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(prepared + kLut14Off, (uint32_t)kLut14Bytes);
#pragma unroll
    for (int k = 0; k < kLutLoads; ++k)
      L[k] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)((threadIdx.x + 64u * kSmallWaves * k) * 16u), 0, 0);
  }
  const Tile t = hdr_resolve(a, h, lane);
  MH_STAMP(1);
  const bool live = t.tile < a.total_tiles;
  const bool staged = live && t.span <= (uint32_t)kStageBytes;
  v4u32 R[kStageChunks];
  span_issue(a, t, lane, R, staged);
  v4u32 *dst = reinterpret_cast<v4u32 *>(s_lut_small);
#pragma unroll
  for (int k = 0; k < kLutLoads; ++k) dst[threadIdx.x + 64u * kSmallWaves * k] = L[k];
  // keep the lengths word's wait below the span's loads and the table's stores
  __builtin_amdgcn_sched_barrier(0);
  const bool l14 = max_len <= (uint32_t)kLut14Bits;
  if (__builtin_expect(!l14, 0)) {
    constexpr uint32_t kChunks = kLutBytes / 16;
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(prepared, (uint32_t)kLutBytes);
#pragma unroll 1
    for (uint32_t c = threadIdx.x; c < kChunks; c += 64u * kSmallWaves)
      dst[c] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)(c * 16u), 0, 0);
  }
  lds_barrier();  // LDS only, as in mh_decode_small_kernel
  MH_STAMP(2);
  small_decode<kDelta>(a, t, lane, R, live, staged, flat8 != 0u, l14, stage, lut,
                       blockIdx.x * nwaves + wave MH_TS_ARG);
}

#if !MH_LANE_PAIRS
// ---- one frame with mid-block marks: two lanes per block, 32 steps each (mh_decode_marked) ----
// mh_decode_frame_kernel's launch with half the chain. A mark (metalhuffman.h) is a second, exact
// entry point at a block's symbol 32, so a wave serves 32 consecutive blocks: lanes l and l + 32
// hold block 32 tile + l, the lower lane decodes rows 0-3 from the block's offset with the tile's
// init, the upper lane rows 4-7 from offset + mark.bits with prev = mark.prev -- decode_block over
// 4 rows, the same steps. Nothing is speculated and the lanes never meet.
//   * Arguments: the marks pointer would make 16 dwords, two over the preload. nb is derived
//     (bw * ceil(h / 8): one scalar multiply ahead of the first load) and the marks travel as their
//     signed distance from the offsets in words (launch() takes mh_decode_frame_kernel where that
//     does not fit 32 bits): 14 dwords again, no read of the kernarg segment.
//   * Prologue order as there: offsets, and in the same trip the mark and the init byte; the table's
//     loads behind them; the span; the LDS-only barrier. No third dependent trip.
//   * 8 waves per workgroup: 192 workgroups for 2048x1536 as before, one table copy per CU, 4 table
//     chunks per thread, two waves per SIMD. 4 waves (384 workgroups, MH_MID_WAVES=4) ran at the
//     parent kernel's speed, 8 about 12 % above it: profiles/mid_marks_ab.txt.
//   * Stage: 32 blocks span about half of what 64 do, so a wave keeps 3 chunks per lane (3072 bytes)
//     in flight where mh_decode_frame_kernel keeps 5. A span over that (or an unknown one) is staged
//     through the wave's whole window -- 32 blocks are at most 32 x 128 bytes and the span's slack --
//     and decoded whole by the lower lanes, marks unused: wave-uniform, decided on the device.
//   * Marks are not trusted: bits is clamped to 512, so an upper lane starts no further than a
//     lower lane's 32nd step can reach and its 32 steps end where a 64-step lane's could. The span
//     and stage guarantees are those of mh_decode_frame_kernel for any mark bytes; the upper lane
//     stores rows 4-7 of its own block (row0 + 4 pitch, rows >= H outside the descriptor as ever).
#ifndef MH_MID_WAVES            // 4: the A/B build of profiles/mid_marks_ab.txt
#define MH_MID_WAVES 8
#endif
constexpr int kMidWaves = MH_MID_WAVES;
constexpr int kMidChunks = 3;                          // 16-B chunks per lane held in flight
constexpr int kMidStageBytes = kMidChunks * 64 * 16;   // the staged fast path's span limit
constexpr uint32_t kMarkMaxBits = 32u * 16u;
static_assert(kMidWaves <= kMaxWavesPerWG, "a window of s_stage per wave");
static_assert(kMidStageBytes <= kStageBytes && 32 * 128 + 64 <= kStageBytes, "32 whole blocks fit a wave's window");
template <bool kDelta>
__global__ void __launch_bounds__(64 * kMidWaves) mh_decode_frame_marked_kernel(
    const uint32_t *p_offsets, const uint16_t *p_lut, const uint8_t *p_codes, uint8_t *p_out,
    const uint8_t *p_block_init, int32_t p_marks_words, uint32_t p_codes_bytes, uint32_t p_pitch, uint32_t p_bw_h) {
  DecodeArgs a{};
  a.offsets = p_offsets;
  a.lut = p_lut;
  a.codes = p_codes;
  a.out = p_out;
  a.block_init = p_block_init;
  a.codes_bytes = p_codes_bytes;
  a.out_pitch = p_pitch;
  a.bw = p_bw_h >> kFrameBwShift;
  a.h = p_bw_h & ((1u << kFrameBwShift) - 1u);
  a.nb = a.bw * ((a.h + 7u) >> 3);
  a.out_frame_bytes = (uint64_t)a.h * p_pitch;
  const uint32_t ntiles = (a.nb + 31u) / 32u;
  a.tiles_per_frame = a.total_tiles = ntiles;
  const uint32_t *marks = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(p_offsets) +
                                                             (int64_t)p_marks_words * 4);
  const uint32_t lane = threadIdx.x & 63u, bl = lane & 31u;
  const bool upper = lane >= 32u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t *stage = s_stage + wave * kStageBytes;
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s_lut_small);
  const uint8_t *prepared = reinterpret_cast<const uint8_t *>(a.lut);
#if MH_DIAG_STAMPS
  unsigned long long ts[kDiagSlots] = {};
  unsigned long long c3 = 0;
  uint32_t rowv = 0;
#endif
  MH_STAMP(0);
  const uint32_t *lens = reinterpret_cast<const uint32_t *>(prepared + kMaxLenOff);
  const uint32_t max_len = lens[0], flat8 = lens[2];
  const uint32_t tile = __builtin_amdgcn_readfirstlane(min(blockIdx.x * (uint32_t)kMidWaves + wave, ntiles));
  const bool live = tile < ntiles;
  // the header's loads, branch-free as hdr_issue's: a wave without a tile reads through
  // zero-record descriptors
  const uint32_t b0 = live ? tile * 32u : 0u, b = b0 + bl;
  const __amdgpu_buffer_rsrc_t ro = uniform_rsrc(a.offsets, live ? a.nb * 4u : 0u);
  const uint32_t h_off = __builtin_amdgcn_raw_buffer_load_b32(ro, (int)(b * 4u), 0, 0);
  const uint32_t h_nxt = __builtin_amdgcn_raw_buffer_load_b32(ro, (int)(b * 4u + 4u), 0, 0);
  const __amdgpu_buffer_rsrc_t rm = uniform_rsrc(marks, live ? a.nb * 4u : 0u);
  const uint32_t h_mark = __builtin_amdgcn_raw_buffer_load_b32(rm, (int)(b * 4u), 0, 0);
  const __amdgpu_buffer_rsrc_t ri = uniform_rsrc(
      a.block_init ? (const void *)a.block_init : (const void *)a.offsets, (live && a.block_init) ? a.nb : 0u);
  const uint32_t h_init = __builtin_amdgcn_raw_buffer_load_b8(ri, (int)b, 0, 0);
  constexpr int kLutLoads = kLut14Bytes / 16 / (64 * kMidWaves);
  static_assert(kLut14Bytes == kLutLoads * 16 * 64 * kMidWaves, "whole table per pass");
  v4u32 L[kLutLoads];
  {
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(prepared + kLut14Off, (uint32_t)kLut14Bytes);
#pragma unroll
    for (int k = 0; k < kLutLoads; ++k)
      L[k] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)((threadIdx.x + 64u * kMidWaves * k) * 16u), 0, 0);
  }
  // hdr_resolve for a tile of 32 blocks held twice
  Tile t;
  t.tile = tile;
  t.f = 0u;
  t.b0 = b0;
  t.valid = b < a.nb;
  t.fbeg = 0;
  t.fb32 = p_codes_bytes;
  const uint32_t fbits = t.fb32 > 0x1FFFFFFFu ? 0xFFFFFFFFu : t.fb32 * 8u;
  const uint32_t end_l = (b + 1u < a.nb) ? h_nxt : min(fbits, h_off + 64u * 16u);
  const uint32_t last = live ? min(31u, a.nb - 1u - b0) : 0u;  // last lane pair holding a block
  const uint32_t sb = __builtin_amdgcn_readfirstlane(h_off);
  const uint32_t eb = __builtin_amdgcn_readlane(end_l, last);
  t.span_end_bits = eb;
  t.start = (sb >> 3) & ~15u;
  uint32_t end = (eb >> 3) + 24u;
  if (end - 16u > t.fb32) end = t.fb32 + 16u;  // as hdr_resolve: no wrapping sum
  t.span = end > t.start ? ((end - t.start + 15u) & ~15u) : 0xFFFFFFFFu;
  t.p = t.valid ? h_off - t.start * 8u : 0u;
  t.init = h_init & 0xFFu;
  // the lane's own entry point: the block's offset and init, or the (clamped) mark
  const uint32_t p = t.p + (upper ? min(h_mark & 0xFFFFu, kMarkMaxBits) : 0u);
  const uint32_t prev = upper ? (h_mark >> 16) & 0xFFu : t.init;
  asm volatile("" ::"v"(p), "v"(prev), "v"(t.p), "v"(t.init));
  MH_STAMP(1);
  const bool staged = live && t.span <= (uint32_t)kMidStageBytes;
  v4u32 R[kMidChunks];
  span_issue(a, t, lane, R, staged);
  v4u32 *dst = reinterpret_cast<v4u32 *>(s_lut_small);
#pragma unroll
  for (int k = 0; k < kLutLoads; ++k) dst[threadIdx.x + 64u * kMidWaves * k] = L[k];
  // keep the lengths word's wait below the span's loads and the table's stores
  __builtin_amdgcn_sched_barrier(0);
  const bool l14 = max_len <= (uint32_t)kLut14Bits;
  if (__builtin_expect(!l14, 0)) {
    constexpr uint32_t kChunks = kLutBytes / 16;
    const __amdgpu_buffer_rsrc_t rl = uniform_rsrc(prepared, (uint32_t)kLutBytes);
#pragma unroll 1
    for (uint32_t c = threadIdx.x; c < kChunks; c += 64u * kMidWaves)
      dst[c] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)(c * 16u), 0, 0);
  }
  lds_barrier();  // LDS only, as in mh_decode_small_kernel
  MH_STAMP(2);
  if (!live) return;  // no barrier below
  const OutTile ot = out_tile(a, t, bl);
  const uint32_t pitch = p_pitch;
  const bool dead = !t.valid;
#if MH_DIAG_ROWS
#define MH_ROWS_ARG , &rowv
#else
#define MH_ROWS_ARG
#endif
  LdsWords src{stage};
  if (__builtin_expect(staged, 1)) {
    span_write(t, lane, R, stage);
    wave_sync();
    MH_STAMP(3);
#if MH_DIAG_STAMPS && MH_DIAG_CLOCK
    c3 = __builtin_amdgcn_s_memtime();
#endif
    const uint32_t row0 = ot.row0 + (upper ? 4u * pitch : 0u);
    if (__builtin_expect(l14 && !flat8, 1))
      decode_block<kDelta, Small14, 4>(src, lut, p, prev, ot.rsrc, row0, pitch, dead MH_ROWS_ARG);
    else if (flat8)
      decode_block<kDelta, SmallFlat8, 4>(src, lut, p, prev, ot.rsrc, row0, pitch, dead);
    else
      decode_block<kDelta, Small13, 4>(src, lut, p, prev, ot.rsrc, row0, pitch, dead MH_ROWS_ARG);
  } else {
    // the oversize (or unknown) span: the whole window from the tile's start, whole blocks on the
    // lower lanes (decode_halves' staging, one pass of 32 whole blocks).
    stage_window(codes_rsrc(a, t), t.start, min(t.span, (uint32_t)kStageBytes), lane, stage);
    wave_sync();
    if (!upper) {
      if (flat8)
        decode_block<kDelta, SmallFlat8>(src, lut, t.p, t.init, ot.rsrc, ot.row0, pitch, dead);
      else if (l14)
        decode_block<kDelta, Small14>(src, lut, t.p, t.init, ot.rsrc, ot.row0, pitch, dead MH_ROWS_NONE);
      else
        decode_block<kDelta, Small13>(src, lut, t.p, t.init, ot.rsrc, ot.row0, pitch, dead MH_ROWS_NONE);
    }
  }
#undef MH_ROWS_ARG
#if MH_DIAG_STAMPS
  small_stamps(ts, staged, c3, lane, blockIdx.x * (uint32_t)kMidWaves + wave, rowv);
#endif
}
#endif  // !MH_LANE_PAIRS

#if MH_LANE_PAIRS
// ---- lane-pair variant of the small-launch kernel (MH_FLAG_LANE_PAIRS, A/B) -------
// north_star's lane-group cursor: each 8x8 block is decoded by two lanes of one
// wave, lanes l and l ^ 32 (32 blocks per wave, so twice the waves of the small
// kernel). Lane A starts at the block's first bit (AAPLShaders.metal:241-268);
// lane B starts speculatively at the block's middle bit M = off + len/2 (len from
// the next block's offset). Huffman paths re-synchronise: once A reaches a bit >= M
// at which B also started a symbol, the two paths coincide from there on, so A stops
// and B's symbols from that point are the block's remaining symbols (lp_decode).
// Round 3 rewrite: the round-2 kernel exchanged cursors and
// masks through three ds_bpermutes on every step and stored every symbol to LDS
// (35.7 vs 5.8 us); this one runs the default step with register output and swaps
// the window masks only at sparse checkpoints.
constexpr uint32_t kLpMinBits = 16;  // blocks shorter than 2x this decode on one lane
constexpr int kLpWaves = 4;
constexpr int kLpStageBytes = 4144;   // >= 15 + 32 blocks x 64 x 16 bits / 8 + 24, 16-B multiple
static_assert(kLpStageBytes <= kStageChunks * 64 * 16, "span_issue covers the lane-pair stage");
constexpr int kLpOutStride = 68;      // bytes per lane row (17 dwords: lanes spread over banks)
__shared__ __attribute__((aligned(16))) uint16_t s_lp_lut[kLut14Entries];
__shared__ __attribute__((aligned(16))) uint8_t s_lp_stage[kLpWaves * kLpStageBytes];
__shared__ __attribute__((aligned(16))) uint8_t s_lp_out[kLpWaves * 64 * kLpOutStride];

__device__ __forceinline__ uint32_t lane_xchg(uint32_t lane, uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane ^ 32u) << 2), (int)v);
}

// bytewise (mod 256) add of c to the four bytes of b
__device__ __forceinline__ uint32_t add_bytes(uint32_t b, uint32_t c) {
  const uint32_t c4 = c * 0x01010101u;
  return ((b & 0x7F7F7F7Fu) + (c4 & 0x7F7F7F7Fu)) ^ ((b ^ c4) & 0x80808080u);
}

// One block on two lanes (round 3: no per-step exchange).
//   * Both lanes run the default kernel's step (64-bit window, refill before every
//     symbol pair, masked next-word read) in one unrolled 64-step loop, so symbol n
//     goes to a fixed byte of the lane's 16 output registers (v_perm packing).
//   * Each lane records its own symbol starts in the window [mid, mid + 128) as a
//     128-bit mask (a 64-bit window leaves 8.4 % of BigBridge's blocks unmatched, this
//     one 1.4 %; scripts/sim_lane_pairs_ckpt.py). B stops at the block end; A stops at the first start that is also
//     one of B's, which it tests on every step once it holds B's final mask.
//   * B's mask reaches A through five ds_bpermutes at sparse checkpoints (every
//     4 steps from step 8, only while some lane of the wave still waits for it); A
//     lanes that were already past the meeting point by then stop at the checkpoint
//     (first common bit of the two masks; their extra symbols are the block's own).
//   * Afterwards one exchange settles the split: A keeps symbols [0, ia), B supplies
//     [ia, 64) from its own index jb; if B decoded too few (corrupt input, a partner
//     that never synchronised) A finishes the block alone. Rows are assembled from the
//     two lanes' register rows through LDS with dword reads and v_alignbyte; B's
//     running sums are rebased bytewise by the delta sum at the meeting point.
template <bool kDelta, class Cfg>
__device__ __forceinline__ void lp_decode(const uint8_t *stage, const uint8_t *lut, uint32_t *row_a,
                                          uint32_t *row_b, uint32_t lane, bool valid, uint32_t p,
                                          uint32_t mid, uint32_t end, bool spec, uint32_t init,
                                          __amdgpu_buffer_rsrc_t out, uint32_t row0, uint32_t pitch) {
  typedef const __attribute__((address_space(3))) uint8_t *lds_u8;
  typedef const __attribute__((address_space(3))) uint32_t *lds_u32;
  const bool is_b = lane >= 32u;
  const lds_u8 base = (lds_u8)stage;
  const uint32_t s0 = is_b ? mid : p;
  lds_u8 wa = base + (s0 >> 5) * 4u;
  uint32_t wbits = (s0 & ~31u) + Cfg::kCur;  // cursor bit = wbits - (S & 0xFF)
  uint32_t S = ((is_b ? 0u : init) << 8) + Cfg::kCur - (s0 & 31u);
  uint32_t kRefill = Cfg::kRefillAt;
  if constexpr ((Cfg::kRefillAt & 1u) != 0u) asm("s_mov_b32 %0, %1" : "=s"(kRefill) : "n"(Cfg::kRefillAt));
  uint32_t hi = *(lds_u32)wa, lo = *(lds_u32)(wa + 4), nw = *(lds_u32)(wa + 8);
  bool act = valid && (!is_b || spec);
  bool chk = valid && spec && !is_b;  // A: still looking for the meeting point
  bool have = false;                   // A: holds B's final window mask
  uint64_t mine0 = 0, mine1 = 0, other0 = 0, other1 = 0;  // starts at mid + [0,64), [64,128)
  uint32_t nd = 0, srel = 128u;        // symbols decoded; meeting point - mid (128: none)
  uint32_t o[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) o[k] = 0u;

  const auto step = [&](const int n) {
    bool c = false;
    if ((n & 1) == 0) {  // sh < 32 at every pair start (codes <= 16 bits)
      c = (S & 0xFFu) <= kRefill;
      hi = c ? lo : hi;
      lo = c ? nw : lo;
      const uint32_t d = c ? 4u : 0u;
      wa += d;
      wbits += d * 8u;
      S += d * 8u;
    }
    const uint64_t x = (((uint64_t)hi) << 32) | lo;
    uint32_t e = *(const __attribute__((address_space(3))) uint16_t *)(
        (lds_u8)lut + ((uint32_t)(x >> (S & 63u)) & Cfg::kMask));
    if ((n & 1) == 0) nw = *(lds_u32)(wa + 8);
    if constexpr (Cfg::kEsc) {
      const bool esc = e < kEscapeBelow;
      if (__builtin_expect(__ballot(esc) != 0, 0)) {
        const uint32_t x3 = (uint32_t)(x >> ((S - 2u) & 63u)) & 7u;
        const uint32_t e2 = *(const __attribute__((address_space(3))) uint16_t *)(
            (lds_u8)lut + 2u * (kL1Entries + ((e & 0xFFu) << kL2Bits) + x3));
        e = esc ? e2 : e;
      }
    }
    S += e;
    o[n >> 2] = __builtin_amdgcn_perm(kDelta ? S : e + 0xFFu, o[n >> 2], ins_sel1(n & 3));
  };

#pragma unroll
  for (int n = 0; n < 64; ++n) {
    if ((n & 1) == 0 && !__ballot(act)) break;  // wave-uniform
    if (n >= 8 && (n & 3) == 0) {
      const bool need = chk && !have;
      if (__ballot(need)) {
        const uint32_t pos = wbits - (S & 0xFFu);
        const bool fin = !act || (int)(pos - mid) >= 128;  // B: its window mask is final
        const uint32_t xf = lane_xchg(lane, fin ? 1u : 0u);
        const uint32_t x0 = lane_xchg(lane, (uint32_t)mine0);
        const uint32_t x1 = lane_xchg(lane, (uint32_t)(mine0 >> 32));
        const uint32_t x2 = lane_xchg(lane, (uint32_t)mine1);
        const uint32_t x3 = lane_xchg(lane, (uint32_t)(mine1 >> 32));
        if (need && xf) {
          have = true;
          other0 = ((uint64_t)x1 << 32) | x0;
          other1 = ((uint64_t)x3 << 32) | x2;
          const uint64_t c0 = mine0 & other0, c1 = mine1 & other1;
          if (c0 | c1) {  // already past the meeting point
            chk = false;
            act = false;
            srel = c0 ? (uint32_t)__builtin_ctzll(c0) : 64u + (uint32_t)__builtin_ctzll(c1);
          } else if ((int)(pos - mid) >= 128) {
            chk = false;  // passed the window without meeting: A decodes the block alone
          }
        }
      }
    }
    {
      // window bookkeeping, branch-free (selects, no exec-mask branches)
      const uint32_t rel = (wbits - (S & 0xFFu)) - mid;
      const bool inw = act && rel < 128u;
      const uint64_t bit = 1ull << (rel & 63u);
      const uint64_t b0 = (inw && rel < 64u) ? bit : 0ull;
      const uint64_t b1 = (inw && rel >= 64u) ? bit : 0ull;
      const bool look = chk && have;
      const bool hit = look && ((other0 & b0) | (other1 & b1)) != 0ull;
      srel = hit ? rel : srel;
      chk = chk && !hit && !(look && act && !inw && (int)rel >= 128);
      act = act && !hit;
      mine0 |= hit ? 0ull : b0;
      mine1 |= hit ? 0ull : b1;
    }
    if (act) {
      step(n);
      nd = (uint32_t)n + 1u;
      act = !((is_b && (wbits - (S & 0xFFu)) >= end) || n == 63);
    }
  }

  // the split: A's symbols before the meeting point (ia), B's (jb)
  const bool met = !is_b && srel < 128u;
  uint32_t ia = 64u, jb = 0u;
  if (met) {  // A's starts at or after the meeting point; B's before it
    const bool lo = srel < 64u;
    const uint32_t r = srel & 63u;
    ia = nd - (lo ? (uint32_t)__builtin_popcountll(mine0 >> r) + (uint32_t)__builtin_popcountll(mine1)
                  : (uint32_t)__builtin_popcountll(mine1 >> r));
    jb = lo ? (uint32_t)__builtin_popcountll(other0 & ((1ull << r) - 1ull))
            : (uint32_t)__builtin_popcountll(other0) + (uint32_t)__builtin_popcountll(other1 & ((1ull << r) - 1ull));
  }
  const uint32_t nb_b = lane_xchg(lane, nd);
  const bool ok = met && nb_b >= jb + 64u - ia;
  // B decoded too few symbols past the meeting point: A finishes the block alone
  const bool rep = met && !ok;
  if (__ballot(rep)) {
#pragma unroll
    for (int n = 0; n < 64; ++n)
      if (rep && (uint32_t)n >= nd) step(n);
  }
  const uint32_t dec = ok ? (0x80000000u | (ia << 8) | jb) : 0u;
  const uint32_t decx = lane_xchg(lane, dec);
  const uint32_t f = is_b ? decx : dec;
  const bool split = (f >> 31) != 0;
  ia = split ? (f >> 8) & 0x7Fu : 64u;
  jb = f & 0x7Fu;

  uint32_t *row = is_b ? row_b : row_a;
#pragma unroll
  for (int k = 0; k < 16; ++k) row[k] = o[k];
  wave_sync();  // both lanes' rows -> reads
  uint32_t cadd = 0;
  if (kDelta) {
    const uint32_t pa = ia ? reinterpret_cast<const uint8_t *>(row_a)[ia - 1u] : init;
    const uint32_t pb = jb ? reinterpret_cast<const uint8_t *>(row_b)[jb - 1u] : 0u;
    cadd = (pa - pb) & 0xFFu;
  }
  const uint32_t r0 = is_b ? 4u : 0u;
  typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
#pragma unroll
  for (uint32_t r = 0; r < 4; ++r) {
    v2u32 v;
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
      const uint32_t q = (r0 + r) * 2u + h;
      const uint32_t aw = row_a[q];
      // B byte index of output byte 4q, + 8 (>= 5 whenever a byte of this word is B's;
      // the clamp only keeps all-A words' unused reads inside the LDS rows)
      int u = (int)(4u * q + 8u + jb) - (int)ia;
      u = u < 4 ? 4 : u;
      uint32_t bw = __builtin_amdgcn_alignbyte(row_b[(u >> 2) - 1], row_b[(u >> 2) - 2], (uint32_t)u & 3u);
      if (kDelta) bw = add_bytes(bw, cadd);
      const int na = (int)ia - (int)(4u * q);  // leading bytes of this word from A
      const uint32_t m = na >= 4 ? 0xFFFFFFFFu : na <= 0 ? 0u : (1u << (8 * na)) - 1u;
      const uint32_t w = (aw & m) | (bw & ~m);
      if (h == 0) v.x = w; else v.y = w;
    }
    const uint32_t off = valid ? row0 + (r0 + r) * pitch : 0xFFFFFFF0u;
    __builtin_amdgcn_raw_buffer_store_b64(v, out, (int)off, 0, Cfg::kAux);
  }
}

template <bool kDelta>
__global__ void __launch_bounds__(64 * kLpWaves) mh_decode_lanepair_kernel(const DecodeArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t bl = lane & 31u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint8_t *stage = s_lp_stage + wave * kLpStageBytes;
  uint32_t *row_a = reinterpret_cast<uint32_t *>(s_lp_out + (wave * 64u + bl) * kLpOutStride);
  uint32_t *row_b = reinterpret_cast<uint32_t *>(s_lp_out + (wave * 64u + 32u + bl) * kLpOutStride);
  const uint8_t *lut = reinterpret_cast<const uint8_t *>(s_lp_lut);
  const uint8_t *prepared = reinterpret_cast<const uint8_t *>(a.lut);
  const uint32_t max_len = *reinterpret_cast<const uint32_t *>(prepared + kMaxLenOff);
  const bool l14 = max_len <= (uint32_t)kLut14Bits;

  // header: 32-block tiles (a.tiles_per_frame / a.total_tiles count them)
  const uint32_t tile = __builtin_amdgcn_readfirstlane(min(blockIdx.x * kLpWaves + wave, a.total_tiles));
  const bool live = tile < a.total_tiles;
  const uint32_t fi = live ? tile / a.tiles_per_frame : 0u;
  const uint32_t b0 = live ? (tile - fi * a.tiles_per_frame) * 32u : 0u;
  const uint32_t b = b0 + bl;
  const __amdgpu_buffer_rsrc_t ro = uniform_rsrc(a.offsets + (uint64_t)fi * a.nb, live ? a.nb * 4u : 0u);
  const uint32_t off = __builtin_amdgcn_raw_buffer_load_b32(ro, (int)(b * 4u), 0, 0);
  const uint32_t nxt = __builtin_amdgcn_raw_buffer_load_b32(ro, (int)(b * 4u + 4u), 0, 0);
  typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t rf = uniform_rsrc(
      a.frame_off ? (const void *)a.frame_off : (const void *)a.offsets,
      (live && a.frame_off) ? 0x7FFFFFF0u : 0u);
  const v2u32 fo = __builtin_amdgcn_raw_buffer_load_b64(rf, (int)((fi + (lane & 1u)) * 8u), 0, 0);
  const __amdgpu_buffer_rsrc_t ri = uniform_rsrc(
      a.block_init ? (const void *)(a.block_init + (uint64_t)fi * a.nb) : (const void *)a.offsets,
      (live && a.block_init) ? a.nb : 0u);
  const uint32_t init = __builtin_amdgcn_raw_buffer_load_b8(ri, (int)b, 0, 0) & 0xFFu;
  // table copy, unconditional 16-B loads issued behind the header (as the small kernel)
  constexpr int kLutLoads = kLut14Bytes / 16 / (64 * kLpWaves);
  static_assert(kLut14Bytes == kLutLoads * 16 * 64 * kLpWaves, "whole table per pass");
  v4u32 L[kLutLoads];
  {
    const __amdgpu_buffer_rsrc_t rl =
        uniform_rsrc(prepared + (l14 ? kLut14Off : 0), l14 ? (uint32_t)kLut14Bytes : (uint32_t)kLutBytes);
#pragma unroll
    for (int k = 0; k < kLutLoads; ++k)
      L[k] = __builtin_amdgcn_raw_buffer_load_b128(rl, (int)((threadIdx.x + 64u * kLpWaves * k) * 16u), 0, 0);
  }
  Tile t;
  t.tile = tile;
  t.f = fi;
  t.b0 = b0;
  t.valid = live && b < a.nb;
  uint64_t fbytes = a.codes_bytes;
  t.fbeg = 0;
  if (a.frame_off) {
    const uint64_t lo = ((uint64_t)__builtin_amdgcn_readlane(fo.y, 0) << 32) | __builtin_amdgcn_readlane(fo.x, 0);
    const uint64_t hi = ((uint64_t)__builtin_amdgcn_readlane(fo.y, 1) << 32) | __builtin_amdgcn_readlane(fo.x, 1);
    t.fbeg = lo;
    fbytes = hi - lo;
  }
  t.fb32 = (uint32_t)(fbytes > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : fbytes);
  const uint32_t fbits = t.fb32 > 0x1FFFFFFFu ? 0xFFFFFFFFu : t.fb32 * 8u;
  const bool exact_end = b + 1u < a.nb;
  const uint32_t end_l = exact_end ? nxt : min(fbits, off + 64u * 16u);
  const uint32_t last = live ? min(31u, a.nb - 1u - b0) : 0u;
  const uint32_t sb = __builtin_amdgcn_readfirstlane(off);
  const uint32_t eb = __builtin_amdgcn_readlane(end_l, last);
  t.start = (sb >> 3) & ~15u;
  uint32_t endb = (eb >> 3) + 24u;
  if (endb - 16u > t.fb32) endb = t.fb32 + 16u;  // as hdr_resolve: no wrapping sum
  t.span = endb > t.start ? min((endb - t.start + 15u) & ~15u, (uint32_t)kLpStageBytes) : 0u;
  t.p = t.valid ? off - t.start * 8u : 0u;
  t.init = init;
  v4u32 R[kStageChunks];
  span_issue(a, t, lane, R, live);
  {
    v4u32 *dst = reinterpret_cast<v4u32 *>(s_lp_lut);
#pragma unroll
    for (int k = 0; k < kLutLoads; ++k) dst[threadIdx.x + 64u * kLpWaves * k] = L[k];
  }
  __syncthreads();  // table in LDS
  if (!live) return;  // wave-uniform; no barrier below
  span_write(t, lane, R, stage);
  wave_sync();
  // output: descriptor at the tile's first block row (as out_tile, 32-block tiles)
  const uint32_t bx = b % a.bw, by = b / a.bw;
  const uint32_t by0 = __builtin_amdgcn_readfirstlane(b0 / a.bw);
  const uint64_t base = (uint64_t)by0 * 8u * a.out_pitch;
  const uint64_t rem = a.out_frame_bytes > base ? a.out_frame_bytes - base : 0u;
  const __amdgpu_buffer_rsrc_t out = uniform_rsrc(a.out + (uint64_t)fi * a.out_frame_stride + base,
                                                  (uint32_t)(rem < 0x7FFFFFF0ull ? rem : 0x7FFFFFF0ull));
  const uint32_t row0 = (by - by0) * 8u * (uint32_t)a.out_pitch + bx * 8u;
  const uint32_t len = end_l - off;
  const uint32_t mid = t.p + (len >> 1);
  const uint32_t end = t.p + len;
  // the frame's last block has no exact end: lane A alone
  const bool spec = t.valid && exact_end && len >= 2u * kLpMinBits && len <= 64u * 16u;
  if (l14)
    lp_decode<kDelta, StepCfg<kLut14Bits, false, false>>(stage, lut, row_a, row_b, lane, t.valid, t.p, mid, end,
                                                  spec, init, out, row0, (uint32_t)a.out_pitch);
  else
    lp_decode<kDelta, StepCfg<kLutBits, false, true>>(stage, lut, row_a, row_b, lane, t.valid, t.p, mid, end,
                                                spec, init, out, row0, (uint32_t)a.out_pitch);
}

#endif  // MH_LANE_PAIRS

// Per-device launch parameters (CU count, batch-kernel occupancy per workgroup
// size), computed once per device ordinal under a per-device mutex: no mutable state
// is shared between devices or written by concurrent callers (the reference keeps
// its tables in module statics, Shared/HuffmanUtil.cpp:87-102).
constexpr int kMaxDevices = 64;
// The kernels that decode one frame slice per workgroup (slice_decode): a SliceKernel is a row of
// kSliceTable, its family's first row + log2_scale (the region and the windows kernels exist at
// scale 2^0..2^3; scale 0 is the unscaled kernel; the crops kernel at scale 0 only).
constexpr int kSliceScales = 4;
enum SliceKernel {
  kSliceFrames,
  kSliceHeaders,
  kSliceRegion,
  kSliceWindows = kSliceRegion + kSliceScales,
  kSliceCrops = kSliceWindows + kSliceScales,  // one scale only
  kSliceNormCrops,                             // + the format (MH_NORM_*)
  kSlicePlanes = kSliceNormCrops + 3,          // + the format
  kSliceSetCrops = kSlicePlanes + 3,           // the crops and the planes over a frame set
  kSliceSetPlanes,                             // + the format
  kSliceSetFrames = kSliceSetPlanes + 3,       // the whole frames of a set
  kSliceKernels
};
#if !MH_LANE_PAIRS
// One row per kernel, [kDelta]: the row device_info() queries the occupancy of is the row
// launch_slices() launches. Kernels with one argument list share a pointer type; a row keeps its
// pair under one common function-pointer type, and launch_slices<Fn> casts back to the family's.
using FramesFn = decltype(&mh_decode_multitable_kernel<false>);
using HeadersFn = decltype(&mh_decode_headers_kernel<false>);
using RegionFn = decltype(&mh_decode_region_kernel<false>);    // = mh_decode_region_scaled_kernel<_, 1..3>
using WindowsFn = decltype(&mh_decode_windows_kernel<false>);  // = mh_decode_windows_scaled_kernel<_, 1..3>
using CropsFn = decltype(&mh_decode_crops_kernel<false>);
using NormCropsFn = decltype(&mh_decode_normcrops_kernel<false, MH_NORM_F16>);
using PlanesFn = decltype(&mh_decode_planes_kernel<false, MH_NORM_F16>);
using SetCropsFn = decltype(&mh_decode_setcrops_kernel<false>);
using SetPlanesFn = decltype(&mh_decode_setplanes_kernel<false, MH_NORM_F16>);
using SetFramesFn = decltype(&mh_decode_setframes_kernel<false>);
using AnyKernel = void (*)();
struct SliceRow {
  AnyKernel fn[2];
};
template <class Fn>
SliceRow slice_row(Fn raw, Fn delta) {
  return {{reinterpret_cast<AnyKernel>(raw), reinterpret_cast<AnyKernel>(delta)}};
}
const SliceRow kSliceTable[] = {
    slice_row<FramesFn>(mh_decode_multitable_kernel<false>, mh_decode_multitable_kernel<true>),
    slice_row<HeadersFn>(mh_decode_headers_kernel<false>, mh_decode_headers_kernel<true>),
    slice_row<RegionFn>(mh_decode_region_kernel<false>, mh_decode_region_kernel<true>),
    slice_row<RegionFn>(mh_decode_region_scaled_kernel<false, 1>, mh_decode_region_scaled_kernel<true, 1>),
    slice_row<RegionFn>(mh_decode_region_scaled_kernel<false, 2>, mh_decode_region_scaled_kernel<true, 2>),
    slice_row<RegionFn>(mh_decode_region_scaled_kernel<false, 3>, mh_decode_region_scaled_kernel<true, 3>),
    slice_row<WindowsFn>(mh_decode_windows_kernel<false>, mh_decode_windows_kernel<true>),
    slice_row<WindowsFn>(mh_decode_windows_scaled_kernel<false, 1>, mh_decode_windows_scaled_kernel<true, 1>),
    slice_row<WindowsFn>(mh_decode_windows_scaled_kernel<false, 2>, mh_decode_windows_scaled_kernel<true, 2>),
    slice_row<WindowsFn>(mh_decode_windows_scaled_kernel<false, 3>, mh_decode_windows_scaled_kernel<true, 3>),
    slice_row<CropsFn>(mh_decode_crops_kernel<false>, mh_decode_crops_kernel<true>),
    slice_row<NormCropsFn>(mh_decode_normcrops_kernel<false, MH_NORM_F16>, mh_decode_normcrops_kernel<true, MH_NORM_F16>),
    slice_row<NormCropsFn>(mh_decode_normcrops_kernel<false, MH_NORM_BF16>,
                           mh_decode_normcrops_kernel<true, MH_NORM_BF16>),
    slice_row<NormCropsFn>(mh_decode_normcrops_kernel<false, MH_NORM_F32>, mh_decode_normcrops_kernel<true, MH_NORM_F32>),
    slice_row<PlanesFn>(mh_decode_planes_kernel<false, MH_NORM_F16>, mh_decode_planes_kernel<true, MH_NORM_F16>),
    slice_row<PlanesFn>(mh_decode_planes_kernel<false, MH_NORM_BF16>, mh_decode_planes_kernel<true, MH_NORM_BF16>),
    slice_row<PlanesFn>(mh_decode_planes_kernel<false, MH_NORM_F32>, mh_decode_planes_kernel<true, MH_NORM_F32>),
    slice_row<SetCropsFn>(mh_decode_setcrops_kernel<false>, mh_decode_setcrops_kernel<true>),
    slice_row<SetPlanesFn>(mh_decode_setplanes_kernel<false, MH_NORM_F16>,
                           mh_decode_setplanes_kernel<true, MH_NORM_F16>),
    slice_row<SetPlanesFn>(mh_decode_setplanes_kernel<false, MH_NORM_BF16>,
                           mh_decode_setplanes_kernel<true, MH_NORM_BF16>),
    slice_row<SetPlanesFn>(mh_decode_setplanes_kernel<false, MH_NORM_F32>,
                           mh_decode_setplanes_kernel<true, MH_NORM_F32>),
    slice_row<SetFramesFn>(mh_decode_setframes_kernel<false>, mh_decode_setframes_kernel<true>),
};
static_assert(sizeof(kSliceTable) / sizeof(kSliceTable[0]) == kSliceKernels, "one row per SliceKernel");
static_assert(kMaxWavesPerWG == MH_DECODE_GROUP_WAVES, "mh_decode_set_plan caps a frame's groups by the waves of one");
#endif
struct DeviceInfo {
  std::mutex m;
  std::atomic<int> cus{0};  // nonzero once the entry is complete
  int occ[2][kMaxWavesPerWG + 1] = {};
  int occ_slice[kSliceKernels][2] = {};  // the frame-slice kernels at 8 waves (raw / delta)
  int occ_walk[2][2] = {};               // the walk kernels at 8 waves: [frames / headers][kBatch]
};
DeviceInfo g_devinfo[kMaxDevices];

template <class Kernel>
int occupancy_of(Kernel kernel, int nw) {
  int blocks = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, nw * 64, 0) != hipSuccess || blocks < 1)
    blocks = 1;
  return blocks;
}

template <bool kDelta>
int occupancy_query(int nw) {
  return occupancy_of(mh_decode_kernel<kDelta>, nw);
}

// The device a launch on `s` runs on (the stream's, or the caller's current one).
int stream_device(hipStream_t s) {
  int dev = -1;
  if (s && hipStreamGetDevice(s, &dev) == hipSuccess) return dev;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  return dev;
}

// Filled once per device under its mutex; a failed query leaves the entry empty,
// so the next call tries again (a transient HIP error does not stick).
const DeviceInfo *device_info(hipStream_t s) {
  const int dev = stream_device(s);
  if (dev < 0 || dev >= kMaxDevices) return nullptr;
  DeviceInfo &d = g_devinfo[dev];
  if (d.cus.load(std::memory_order_acquire)) return &d;
  std::lock_guard<std::mutex> lock(d.m);
  if (d.cus.load(std::memory_order_relaxed)) return &d;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess || prop.multiProcessorCount < 1) return nullptr;
  int cur = -1;
  const bool swap = hipGetDevice(&cur) == hipSuccess && cur != dev;
  if (swap && hipSetDevice(dev) != hipSuccess) return nullptr;
  for (int nw = 1; nw <= kMaxWavesPerWG; ++nw) {
    d.occ[0][nw] = occupancy_query<false>(nw);
    d.occ[1][nw] = occupancy_query<true>(nw);
  }
#if !MH_LANE_PAIRS
  for (int k = 0; k < kSliceKernels; ++k)
    for (int delta = 0; delta < 2; ++delta)
      d.occ_slice[k][delta] = occupancy_of(kSliceTable[k].fn[delta], kMaxWavesPerWG);
  d.occ_walk[0][0] = occupancy_of(mh_walk_frames_kernel<false>, kMaxWavesPerWG);
  d.occ_walk[0][1] = occupancy_of(mh_walk_frames_kernel<true>, kMaxWavesPerWG);
  d.occ_walk[1][0] = occupancy_of(mh_walk_headers_kernel<false>, kMaxWavesPerWG);
  d.occ_walk[1][1] = occupancy_of(mh_walk_headers_kernel<true>, kMaxWavesPerWG);
#endif
  if (swap) (void)hipSetDevice(cur);
  d.cus.store(prop.multiProcessorCount, std::memory_order_release);  // last: marks the entry complete
  return &d;
}

// One kernel launch; any_order (MH_FLAG_ANY_ORDER) clears the dispatch packet's
// barrier bit so the kernel may start while earlier work on the stream drains.
#define MH_LAUNCH(kernel, grid, block, s, any_order, ...)                                          \
  do {                                                                                            \
    if (any_order)                                                                                \
      hipExtLaunchKernelGGL(kernel, grid, block, 0, s, nullptr, nullptr, hipExtAnyOrderLaunch, __VA_ARGS__); \
    else                                                                                          \
      hipLaunchKernelGGL(kernel, grid, block, 0, s, __VA_ARGS__);                                 \
  } while (0)

// marks (mh_decode_marked): the frame's mid-block marks or null; used by the single-frame launch only
template <bool kDelta>
int launch(const DecodeArgs &a0, hipStream_t s, bool lane_pairs, bool any_order, const uint32_t *marks = nullptr) {
  DecodeArgs a = a0;
  const DeviceInfo *di = device_info(s);
  if (!di) return MH_ERR_HIP;
  const int cus = di->cus.load(std::memory_order_relaxed);
#if MH_LANE_PAIRS
  if (lane_pairs && a.lut && a.total_tiles <= (uint32_t)(kSmallMaxTilesPerCU * cus)) {
    // experimental lane-pair decode (MH_FLAG_LANE_PAIRS): 32-block tiles
    const uint32_t n_frames = a.total_tiles / a.tiles_per_frame;
    a.tiles_per_frame = (a.nb + 31u) / 32u;
    a.total_tiles = a.tiles_per_frame * n_frames;
    a.n_groups = (a.total_tiles + kLpWaves - 1) / kLpWaves;
    MH_LAUNCH(mh_decode_lanepair_kernel<kDelta>, dim3(a.n_groups), dim3(kLpWaves * 64), s, any_order, a);
    return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
  }
#else
  (void)lane_pairs;
#endif
  if (a.lut && a.total_tiles <= (uint32_t)(kSmallMaxTilesPerCU * cus)) {
    // one tile per wave, kSmallWaves waves per workgroup: fewer workgroups copy the
    // table (measured: 8-wave groups beat one 3-wave group per CU by ~5 %)
    const uint32_t nw = kSmallWaves;
    a.n_groups = (a.total_tiles + nw - 1) / nw;
    if (a.total_tiles == a.tiles_per_frame && !a.frame_off) {
#if !MH_LANE_PAIRS
      // ... with marks: two lanes per block, 32 blocks per wave. The marks travel as their distance
      // from the offsets in words; marks out of a signed 32-bit word's reach (never a producer's
      // layout, which puts them beside the offsets) are left unused.
      const int64_t dist = (int64_t)(uintptr_t)marks - (int64_t)(uintptr_t)a.offsets;
      if (marks && (dist & 3) == 0 && dist / 4 >= INT32_MIN && dist / 4 <= INT32_MAX) {
        const uint32_t groups = ((a.nb + 31u) / 32u + kMidWaves - 1) / kMidWaves;
        MH_LAUNCH(mh_decode_frame_marked_kernel<kDelta>, dim3(groups), dim3(kMidWaves * 64), s, any_order, a.offsets,
                  a.lut, a.codes, a.out, a.block_init, (int32_t)(dist / 4), (uint32_t)a.codes_bytes,
                  (uint32_t)a.out_pitch, (a.bw << kFrameBwShift) | a.h);
        return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
      }
#else
      (void)marks;
#endif
      // one frame, no frame-offset array: the entry whose arguments are all preloaded.
      // mh_decode has bounded what the 32-bit arguments hold (codes_bytes, pitch, dims).
      MH_LAUNCH(mh_decode_frame_kernel<kDelta>, dim3(a.n_groups), dim3(nw * 64), s, any_order, a.offsets, a.lut,
                a.codes, a.out, a.block_init, a.nb, (uint32_t)a.codes_bytes, (uint32_t)a.out_pitch,
                (a.bw << kFrameBwShift) | a.h);
      return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
    }
    MH_LAUNCH(mh_decode_small_kernel<kDelta>, dim3(a.n_groups), dim3(nw * 64), s, any_order, a.offsets,
              a.frame_off, a.block_init, a.lut, a.nb, a.tiles_per_frame, a.total_tiles, a);
    return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
  }
  // Waves per workgroup: spread a small launch (one 2048x1536 frame = 768 tiles)
  // over every CU; 8-wave workgroups (3 per CU by LDS) for batches.
  uint32_t nw = (a.total_tiles + (uint32_t)cus - 1) / (uint32_t)cus;
  if (nw < 1) nw = 1;
  if (nw > (uint32_t)kMaxWavesPerWG) nw = kMaxWavesPerWG;
  a.n_groups = (a.total_tiles + nw - 1) / nw;
  const uint32_t resident = (uint32_t)(cus * di->occ[kDelta ? 1 : 0][nw]);
  const uint32_t grid = a.n_groups < resident ? a.n_groups : resident;
  a.nwaves = nw;
  a.grid = grid;
  MH_LAUNCH(mh_decode_kernel<kDelta>, dim3(grid), dim3(nw * 64), s, any_order, a.offsets, a.frame_off,
            a.block_init, a.lut, a.nb, a.tiles_per_frame, a.total_tiles, a.nwaves, a.grid, a);
  return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
}

bool dims_ok(const mh_dims &d) {
  return d.width && d.height && d.width <= MH_MAX_DIM && d.height <= MH_MAX_DIM &&
         d.block_width == (d.width + 7) / 8 && d.block_height == (d.height + 7) / 8;
}

// A raster and its tiling. A region's: pixel size pw x ph (the frame's edge clips the last blocks),
// S = ceil(bw / 64) tiles per block row, bh * S tiles per frame (<= 8192 * 128).
// false: the region is empty or leaves the frame (`d` has passed dims_ok).
struct RegionExtent {
  uint64_t pw, ph;
  uint32_t segs, tiles;
};
bool region_extent(const mh_dims &d, const mh_region *rg, RegionExtent &e) {
  if (!rg->bw || !rg->bh || (uint64_t)rg->bx0 + rg->bw > d.block_width ||
      (uint64_t)rg->by0 + rg->bh > d.block_height)
    return false;
  const uint64_t x1 = 8ull * (rg->bx0 + rg->bw), y1 = 8ull * (rg->by0 + rg->bh);
  e.pw = (x1 < d.width ? x1 : d.width) - 8ull * rg->bx0;
  e.ph = (y1 < d.height ? y1 : d.height) - 8ull * rg->by0;
  e.segs = (rg->bw + 63u) / 64u;
  e.tiles = rg->bh * e.segs;
  return true;
}

// A crop's: pixel size w x h (rg->bw x rg->bh, in PIXELS), OW = ceil(w / 8) output words per row, 63
// of them per tile (word j needs blocks j and j + 1 of a wave's 64), S = ceil(OW / 63) tiles per
// block row, and CBH = (h + 14) / 8 block rows, the most any y0 & 7 needs.
// false: the size is empty or exceeds the frame.
bool crop_extent(const mh_dims &d, const mh_region *rg, RegionExtent &e) {
  if (!rg->bw || !rg->bh || rg->bw > d.width || rg->bh > d.height) return false;
  e.pw = rg->bw;
  e.ph = rg->bh;
  e.segs = ((rg->bw + 7u) / 8u + 62u) / 63u;
  e.tiles = ((rg->bh + 14u) / 8u) * e.segs;
  return true;
}

// One decode call, as every entry point describes it to the helpers below: where its Huffman tables
// come from (and so which table rules it checks), which part of the frames it decodes at which scale
// and, once call_geometry() has passed, the rasters and tiles that makes.
struct DecodeCall {
  enum Kind {
    kInFrame,   // mh_decode: the frame's own table1 / table2 (+ optional d_lut)
    kPrepared,  // mh_decode_frames: prepared tables at `ptr`, `stride` bytes apart
    kHeaders,   // mh_decode_headers: canonical headers at `ptr`, no alignment or stride rule
    kRegion,    // mh_decode_region[_scaled]: kPrepared over region `rg` at scale 2^log2_scale; stride 0
                // is one table for all frames
    kWindows,   // mh_decode_windows[_scaled]: kRegion with rg = {0, 0, bw, bh}, the windows' size, and
                // n_windows rasters, described by the device array `windows`
    kCrops,     // mh_decode_crops: kWindows with rg = {0, 0, w, h} in PIXELS, the crops' size, and the
                // descriptors' origins in pixels (scale 0 only)
    kNormCrops, // mh_decode_crops_norm: kCrops into rasters of `format`'s elements, 2 or 4 bytes each, under
                // the map (scale, bias); rows are stored 16 bytes at a time
  } kind;
  const void *ptr = nullptr;
  uint64_t stride = 0;
  const mh_region *rg = nullptr;
  uint32_t log2_scale = 0;  // 0: the unscaled kernel (c = 8, s = 1 in the rules below)
  const void *windows = nullptr;
  uint32_t n_windows = 0;
  uint32_t allowed_flags = MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER;
  uint32_t format = 0;  // kNormCrops: MH_NORM_*
  float scale = 1.0f, bias = 0.0f;
  // mh_decode_crops_norm_planes (kNormCrops): every descriptor is n_planes rasters, out_plane_stride
  // bytes apart, the crops of frames plane_frame_stride apart; one plane is mh_decode_crops_norm
  uint32_t n_planes = 1, plane_frame_stride = 0;
  uint64_t out_plane_stride = 0;
  // mh_decode_set_crops[_norm_planes] (kCrops / kNormCrops): the frames are a SET described by the
  // device array `geoms` over `total_blocks` offsets; dims carry the set's maxima and their block
  // counts are ignored (call_dims)
  bool set = false;
  const void *geoms = nullptr;
  uint32_t total_blocks = 0;
  // mh_decode_set_frames (kPrepared over a set): the rasters are described by the device records
  // `rasters` beside `shares` and the group map `group_frame` (n_groups words), inside out_bytes at
  // d_out; no pitch or stride arrives, so none of their rules applies, and stride 0 is one table
  bool set_frames = false;
  const void *rasters = nullptr, *shares = nullptr, *group_frame = nullptr;
  uint32_t n_groups = 0;
  uint64_t out_bytes = 0;
  // mh_check_frames / mh_check_headers (kPrepared / kHeaders): no raster and none of its rules, one
  // table for all frames at stride 0 as a region's, and `words`, the OR of the report's and the
  // verdict's addresses, 4-byte aligned
  bool walk = false;
  uintptr_t words = 0;
  // call_geometry()'s results: one raster's pixel size and tiles (segs: a region's only), and the
  // number of rasters, which is the number of units the grid is cut into
  RegionExtent re = {};
  uint32_t n_units = 0;
  bool rasterless() const { return walk || set_frames; }  // no out_pitch / out_frame_stride to judge
  bool cropped() const { return kind == kCrops || kind == kNormCrops; }
  bool windowed() const { return kind == kWindows || cropped(); }
  bool regional() const { return kind == kRegion || windowed(); }
  // the units the grid is cut into: a raster each (the tile cap bounds the product)
  uint32_t units() const { return n_units * n_planes; }
  // an element's bytes, and the row of its family in kSliceTable (the scale, or the format)
  uint32_t elem() const { return kind != kNormCrops ? 1u : format == MH_NORM_F32 ? 4u : 2u; }
  uint32_t table_row() const { return kind == kNormCrops ? format : log2_scale; }
};

// The rules that the decode entries and the *_shape entries share, in their one order: flags, the
// scale (a scale above 3 is reported where a bad flag is), dims, the region. A region's pixel size
// RW x RH -- for windows the full 8 bw x 8 bh: windows differ in RW / RH, and a size that is empty
// or exceeds the grid is MH_ERR_DIMS -- becomes SW x SH = ceil(RW / s) x ceil(RH / s) at scale s.
// The dims a call is judged and tiled by: the frame's, or for a set its maxima with the block counts
// that go with them (a width past MH_MAX_DIM may wrap here: dims_ok refuses it by the width).
mh_dims call_dims(const mh_frame *fr, const DecodeCall &c) {
  mh_dims d = fr->dims;
  if (c.set) {
    d.block_width = (d.width + 7u) / 8u;
    d.block_height = (d.height + 7u) / 8u;
  }
  return d;
}

int call_geometry(const mh_frame *fr, DecodeCall &c) {
  if (fr->flags & ~c.allowed_flags) return MH_ERR_INVALID_ARG;
  if (c.log2_scale > 3u) return MH_ERR_INVALID_ARG;
  if (c.kind == DecodeCall::kNormCrops && (c.format > MH_NORM_F32 || !std::isfinite(c.scale) || !std::isfinite(c.bias)))
    return MH_ERR_INVALID_ARG;
  const mh_dims d = call_dims(fr, c);
  if (!dims_ok(d)) return MH_ERR_DIMS;
  c.n_units = c.windowed() ? c.n_windows : fr->n_frames;
  if (!c.regional()) {
    c.re = {d.width, d.height, 0u, (d.block_width * d.block_height + 63) / 64};
    return MH_OK;
  }
  if (c.cropped()) {
    if (!crop_extent(d, c.rg, c.re)) return MH_ERR_DIMS;
    // the last plane of a sample of frame 0 names a frame (64-bit: the product does not wrap)
    return (uint64_t)(c.n_planes - 1u) * c.plane_frame_stride >= fr->n_frames ? MH_ERR_DIMS : MH_OK;
  }
  if (!region_extent(d, c.rg, c.re)) return MH_ERR_DIMS;
  if (c.windowed()) {
    c.re.pw = 8ull * c.rg->bw;
    c.re.ph = 8ull * c.rg->bh;
  }
  const uint64_t s = 1ull << c.log2_scale;
  c.re.pw = (c.re.pw + s - 1) >> c.log2_scale;
  c.re.ph = (c.re.ph + s - 1) >> c.log2_scale;
  return MH_OK;
}

// The tile cap: a launch addresses at most 2^31 - 1 tiles.
bool tiles_fit(const DecodeCall &c) { return (uint64_t)c.re.tiles * c.n_units * c.n_planes <= 0x7FFFFFFFull; }

// The argument checks of the decode entry points, all before any HIP call. Every entry runs
// the same rules in the same order; the frame's own table fields count only for kInFrame, and
// the other kinds check `ptr` / `stride` in their place, rule by rule. A region is checked with
// the dims (call_geometry), and its raster's size stands where W x H does in the pitch and stride
// rules; at scale 2^log2_scale c = 8 >> log2_scale stands where 8 does in the raster's alignment
// rules. Windows: n_windows rasters in the place of n_frames (`out_frame_stride` is the window
// stride), and the descriptor array checked where the tables are.
int check_decode_args(const mh_frame *fr, const uint8_t *d_out, size_t out_pitch, size_t out_frame_stride,
                      DecodeCall &c) {
  const bool in_frame = c.kind == DecodeCall::kInFrame, windowed = c.windowed(), regional = c.regional();
  const bool prepared = c.kind == DecodeCall::kPrepared || regional;
  if (!fr || (!c.walk && !d_out) || !fr->d_block_offsets || !fr->d_codes) return MH_ERR_INVALID_ARG;
  if (regional && !c.rg) return MH_ERR_INVALID_ARG;
  if (windowed && (!c.windows || c.n_windows == 0)) return MH_ERR_INVALID_ARG;
  if (c.set && (!c.geoms || c.total_blocks == 0)) return MH_ERR_INVALID_ARG;
  if (c.set_frames && (!c.rasters || !c.shares || !c.group_frame || c.n_groups == 0 || c.n_groups > 0x7FFFFFFFu ||
                       c.out_bytes == 0))
    return MH_ERR_INVALID_ARG;
  if (in_frame ? (!fr->d_table1 || !fr->d_table2) : !c.ptr) return MH_ERR_INVALID_ARG;
  if (fr->n_frames == 0 || (fr->n_frames > 1 && !fr->d_frame_code_offsets)) return MH_ERR_INVALID_ARG;
  const int rc = call_geometry(fr, c);
  if (rc != MH_OK) return rc;
  const uint32_t n_rasters = c.n_units;
  const bool norm = c.kind == DecodeCall::kNormCrops;
  const uint64_t am = norm ? 15u : (8u >> c.log2_scale) - 1u;  // the row store's width - 1
  // a row's bytes: normalised crops write round_up(w, 8) elements, which a pitch of w elements rounded
  // up to 16 bytes does not hold at 4 bytes each, so the whole words are asked for
  const uint64_t row_bytes = norm ? ((c.re.pw + 7u) & ~7ull) * c.elem() : c.re.pw;
  if (in_frame && (fr->table2_entries < 256 || (fr->table2_entries % 256) != 0 ||
                   fr->table2_entries > MH_TABLE2_MAX_ENTRIES))
    return MH_ERR_TABLE;
  if (((uintptr_t)fr->d_codes & 15u) || (out_pitch & am) || ((uintptr_t)d_out & am) ||
      (n_rasters > 1 && (out_frame_stride & am)) || (c.n_planes > 1 && (c.out_plane_stride & am)))
    return MH_ERR_ALIGN;
  if (windowed && (((uintptr_t)c.windows | (uintptr_t)c.geoms) & 15u)) return MH_ERR_ALIGN;
  if (c.set_frames && ((((uintptr_t)c.geoms | (uintptr_t)c.rasters | (uintptr_t)c.shares) & 15u) ||
                       ((uintptr_t)c.group_frame & 3u)))
    return MH_ERR_ALIGN;
  if (in_frame ? (((uintptr_t)fr->d_lut & 15u) != 0) : (prepared && (((uintptr_t)c.ptr & 15u) || (c.stride & 15u))))
    return MH_ERR_ALIGN;
  if (c.words & 3u) return MH_ERR_ALIGN;
  if (!c.rasterless() &&
      (out_pitch < row_bytes || out_pitch > (1u << 20) || (n_rasters > 1 && out_frame_stride < out_pitch * c.re.ph)))
    return MH_ERR_CAPACITY;
  // planes: a plane holds its h rows, and a slot its planes -- (n_planes - 1) * out_plane_stride +
  // out_pitch * h bytes, compared by division: the product may wrap
  if (c.n_planes > 1 && (c.out_plane_stride < out_pitch * c.re.ph ||
                         (n_rasters > 1 && (out_frame_stride - out_pitch * c.re.ph) / (c.n_planes - 1u) <
                                               c.out_plane_stride)))
    return MH_ERR_CAPACITY;
  if (fr->codes_bytes < MH_CODES_PAD) return MH_ERR_CAPACITY;
  if (fr->n_frames == 1 && !fr->d_frame_code_offsets && fr->codes_bytes > 0xFFFFFFF0ull)
    return MH_ERR_CAPACITY;
  if (prepared && c.stride < (uint64_t)kPreparedBytes && !((regional || c.rasterless()) && c.stride == 0))
    return MH_ERR_CAPACITY;  // mh_lut_bytes()
  return MH_OK;
}

// DecodeArgs from a checked call (tables excepted): the raster and the tiles are c.re's, and there
// are c.n_units rasters. MH_ERR_CAPACITY past the tile cap.
int fill_decode_args(const mh_frame *fr, uint8_t *d_out, size_t out_pitch, size_t out_frame_stride,
                     DecodeArgs &a, const DecodeCall &c) {
  const mh_dims d = call_dims(fr, c);
  a.offsets = fr->d_block_offsets;
  a.codes = fr->d_codes;
  a.frame_off = fr->d_frame_code_offsets;
  a.codes_bytes = fr->codes_bytes;
  a.block_init = fr->d_block_init;
  a.out = d_out;
  a.out_pitch = out_pitch;
  a.out_frame_stride = out_frame_stride;
  a.out_frame_bytes = c.re.ph * out_pitch;
  a.w = d.width;
  a.h = d.height;
  a.bw = d.block_width;
  a.bh = d.block_height;
  a.nb = d.block_width * d.block_height;
  a.tiles_per_frame = c.re.tiles;
  if (!tiles_fit(c)) return MH_ERR_CAPACITY;
  a.total_tiles = a.tiles_per_frame * c.units();
  return MH_OK;
}

#if !MH_LANE_PAIRS
// The frame-slice kernels' launch shape: G workgroups of 8 waves per frame,
//   G = clamp(ceil(R / n_frames), 1, ceil(tiles_per_frame / 8)),
// R = the workgroups resident on the device at once (CUs x the kernel's occupancy): about
// one resident round when the frames are few, one workgroup per frame when they are many.
// One rule for every row of kSliceTable, each with its own occupancy and (a region, windows) its own tiles.
// (the walk kernels of mh_check_frames / mh_check_headers follow it with their own occupancy: walk_shape)
uint32_t groups_for(const DeviceInfo *di, int occupancy, uint32_t n_frames, uint32_t tiles_per_frame) {
  const uint64_t resident = (uint64_t)di->cus.load(std::memory_order_relaxed) * (uint64_t)occupancy;
  const uint64_t want = (resident + n_frames - 1) / n_frames;
  const uint64_t most = (tiles_per_frame + (uint32_t)kMaxWavesPerWG - 1) / (uint32_t)kMaxWavesPerWG;
  return (uint32_t)(want < 1 ? 1 : want > most ? most : want);
}

int slice_shape(SliceKernel k, uint32_t n_frames, uint32_t tiles_per_frame, bool delta, hipStream_t s,
                uint32_t *groups) {
  const DeviceInfo *di = device_info(s);
  if (!di) return MH_ERR_HIP;
  *groups = groups_for(di, di->occ_slice[k][delta ? 1 : 0], n_frames, tiles_per_frame);
  return MH_OK;
}

int walk_shape(bool headers, bool batch, uint32_t n_frames, uint32_t tiles_per_frame, hipStream_t s,
               uint32_t *groups) {
  const DeviceInfo *di = device_info(s);
  if (!di) return MH_ERR_HIP;
  *groups = groups_for(di, di->occ_walk[headers ? 1 : 0][batch ? 1 : 0], n_frames, tiles_per_frame);
  return MH_OK;
}

// What every frame-slice entry does ahead of its launch: the checks, then DecodeArgs (t1 / t2 / lut
// stay null: every workgroup takes its frame's table from the table array or builds it from the
// frame's header) and the two decode flags. The raster and the tiling are left in c.re.
struct SliceArgs {
  DecodeArgs a;
  bool delta, any_order;
};
int slice_prologue(const mh_frame *fr, uint8_t *d_out, size_t out_pitch, size_t out_stride, DecodeCall &c,
                   SliceArgs &p) {
  int rc = check_decode_args(fr, d_out, out_pitch, out_stride, c);
  if (rc != MH_OK) return rc;
  p.a = DecodeArgs{};
  rc = fill_decode_args(fr, d_out, out_pitch, out_stride, p.a, c);
  p.delta = !(fr->flags & MH_FLAG_NO_DELTA);
  p.any_order = (fr->flags & MH_FLAG_ANY_ORDER) != 0;
  return rc;
}

// One launch of a frame-slice kernel: row `family` + c.log2_scale of kSliceTable, whose kernels are
// of type Fn. The kernels' argument lists differ only in the table arguments on either side of
// `status` (prepared tables: luts, stride; headers: headers, verdict; windows: luts, the descriptor
// array) and in the region's or the windows' scalars (`tail`), which follow the group count. The
// grid is cut into c.n_units units: the frames, or the windows.
template <class Fn, class Table, class TableAux, class... Tail>
int launch_slices(SliceKernel family, const DecodeCall &c, const SliceArgs &p, void *stream, Table table,
                  const int32_t *status, TableAux aux, Tail... tail) {
  const SliceKernel k = (SliceKernel)(family + c.table_row());
  const DecodeArgs &a = p.a;
  hipStream_t s = (hipStream_t)stream;
  uint32_t G = 0;
  const int rc = slice_shape(k, c.units(), a.tiles_per_frame, p.delta, s, &G);
  if (rc != MH_OK) return rc;
  const uint64_t grid = (uint64_t)G * c.units();
  if (grid > 0x7FFFFFFFull) return MH_ERR_CAPACITY;
  const Fn kernel = reinterpret_cast<Fn>(kSliceTable[k].fn[p.delta ? 1 : 0]);
  MH_LAUNCH(kernel, dim3((uint32_t)grid), dim3(kMaxWavesPerWG * 64), s, p.any_order, a.offsets, a.frame_off,
            a.block_init, table, status, aux, a.nb, a.tiles_per_frame, G, tail..., a);
  return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
}

// The DecodeCall of a list entry (windows, crops, normalised crops) or of its *_shape twin (no tables,
// no descriptors). It owns the size c.rg points to: blocks for windows, pixels for crops.
struct ListCall : DecodeCall {
  mh_region size;
  ListCall(Kind kind, uint32_t w, uint32_t h, uint32_t log2_scale, uint32_t n, const void *descriptors = nullptr,
           const void *luts = nullptr, uint64_t stride = 0)
      : DecodeCall{kind, luts, stride, &size, log2_scale, descriptors, n}, size{0u, 0u, w, h} {}
  // ... over a frame set (the crop kinds): the *_shape twins pass no records
  ListCall &over_set(const void *d_geoms = nullptr, uint32_t blocks = 0) {
    set = true;
    geoms = d_geoms;
    total_blocks = blocks;
    return *this;
  }
  // ... of samples of planes (kNormCrops): the *_shape twins pass no strides
  ListCall &planes(uint32_t fmt, uint32_t n, const PlaneArgs *pl = nullptr) {
    format = fmt;
    n_planes = n;
    plane_frame_stride = pl ? pl->frame_stride : 0u;
    out_plane_stride = pl ? pl->out_stride : 0u;
    return *this;
  }
  ListCall(const ListCall &) = delete;  // rg points into this object
};

// A list entry behind what it checks itself: the refusal of a status array that is the frame status it
// reads (MH_ERR_INVALID_ARG, as every refusal ahead of the prologue), the prologue and the launch.
// Behind the group count every list kernel takes the segments, the size, its verdict's frame limit
// (n_frames less `frames_short`) and last origin that fits (blocks for windows, pixels for crops),
// the table stride and its own status array, then `tail`.
template <class Fn, class Desc, class... Tail>
int decode_list(SliceKernel family, const mh_frame *fr, ListCall &c, const Desc *descriptors,
                const int32_t *frame_status, int32_t *list_status, void *d_out, size_t out_pitch, size_t out_stride,
                void *stream, uint32_t frames_short, Tail... tail) {
  if (list_status && list_status == frame_status) return MH_ERR_INVALID_ARG;
  SliceArgs p;
  const int rc = slice_prologue(fr, static_cast<uint8_t *>(d_out), out_pitch, out_stride, c, p);
  if (rc != MH_OK) return rc;
  const mh_dims d = call_dims(fr, c);
  // a set: the kernels take total_blocks where the others take the frames' nb, and make each
  // workgroup's nb and bw from its frame's geometry record
  if (c.set) p.a.nb = c.total_blocks;
  return launch_slices<Fn>(family, c, p, stream, static_cast<const uint8_t *>(c.ptr), frame_status, descriptors,
                           c.re.segs, c.size.bw, c.size.bh, fr->n_frames - frames_short,
                           (c.cropped() ? d.width : d.block_width) - c.size.bw,
                           (c.cropped() ? d.height : d.block_height) - c.size.bh, c.stride, list_status, tail...);
}

// mh_decode_*_shape: slice_shape for a frame description, the units and the tiles counted by the
// decode entries' own rules (call_geometry). The tile cap is reported for a region or windows only,
// as it always was: the whole-frame entries leave it to the decode call.
int slice_shape_entry(SliceKernel family, const mh_frame *fr, DecodeCall c, void *stream,
                      uint32_t *groups_per_unit, uint32_t *waves_per_group) {
  if (!fr || (c.regional() && !c.rg) || !groups_per_unit || !waves_per_group || fr->n_frames == 0)
    return MH_ERR_INVALID_ARG;
  if (c.windowed() && c.n_windows == 0) return MH_ERR_INVALID_ARG;
  int rc = call_geometry(fr, c);
  if (rc != MH_OK) return rc;
  if (c.regional() && !tiles_fit(c)) return MH_ERR_CAPACITY;
  rc = slice_shape((SliceKernel)(family + c.table_row()), c.units(), c.re.tiles, !(fr->flags & MH_FLAG_NO_DELTA),
                   (hipStream_t)stream, groups_per_unit);
  if (rc != MH_OK) return rc;
  *waves_per_group = kMaxWavesPerWG;
  return MH_OK;
}

// mh_check_frames / mh_check_headers behind what they check themselves (the three aliasing pairs and
// the report, MH_ERR_INVALID_ARG as every refusal ahead of the shared checks): the decode entries'
// checks without a raster, then two ordinary launches on the stream -- the init launch must have
// finished before a walk's atomics, so MH_FLAG_ANY_ORDER is accepted and not applied.
int check_walk(const mh_frame *fr, bool headers, const void *tables, uint64_t stride, const int32_t *frame_status,
               int32_t *header_status, uint32_t *report, int32_t *verdict, void *stream) {
  if (verdict && (verdict == frame_status || verdict == header_status)) return MH_ERR_INVALID_ARG;
  if (header_status && header_status == frame_status) return MH_ERR_INVALID_ARG;
  if (!report) return MH_ERR_INVALID_ARG;
  DecodeCall c{headers ? DecodeCall::kHeaders : DecodeCall::kPrepared, tables, stride};
  c.walk = true;
  c.words = (uintptr_t)report | (uintptr_t)verdict;
  int rc = check_decode_args(fr, nullptr, 0, 0, c);
  if (rc != MH_OK) return rc;
  if (!tiles_fit(c)) return MH_ERR_CAPACITY;
  const uint32_t nb = fr->dims.block_width * fr->dims.block_height, n = fr->n_frames;
  const bool batch = fr->d_frame_code_offsets != nullptr;
  hipStream_t s = (hipStream_t)stream;
  uint32_t G = 0;
  rc = walk_shape(headers, batch, n, c.re.tiles, s, &G);
  if (rc != MH_OK) return rc;
  const uint64_t grid = (uint64_t)G * n;
  if (grid > 0x7FFFFFFFull) return MH_ERR_CAPACITY;
  hipLaunchKernelGGL(mh_walk_init_kernel, dim3((uint32_t)((4ull * n + 255u) / 256u)), dim3(256), 0, s, frame_status,
                     report, verdict, n);
  const dim3 g((uint32_t)grid), b(kMaxWavesPerWG * 64);
  const uint8_t *t = static_cast<const uint8_t *>(tables);
  if (headers) {
    const auto k = batch ? mh_walk_headers_kernel<true> : mh_walk_headers_kernel<false>;
    hipLaunchKernelGGL(k, g, b, 0, s, fr->d_block_offsets, fr->d_frame_code_offsets, fr->d_codes, t, frame_status,
                       header_status, fr->codes_bytes, nb, c.re.tiles, G, report, verdict);
  } else {
    const auto k = batch ? mh_walk_frames_kernel<true> : mh_walk_frames_kernel<false>;
    hipLaunchKernelGGL(k, g, b, 0, s, fr->d_block_offsets, fr->d_frame_code_offsets, fr->d_codes, t, frame_status,
                       stride, fr->codes_bytes, nb, c.re.tiles, G, report, verdict);
  }
  return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
}

int check_walk_shape(const mh_frame *fr, bool headers, void *stream, uint32_t *groups_per_frame,
                     uint32_t *waves_per_group) {
  if (!fr || !groups_per_frame || !waves_per_group || fr->n_frames == 0) return MH_ERR_INVALID_ARG;
  DecodeCall c{headers ? DecodeCall::kHeaders : DecodeCall::kPrepared};
  int rc = call_geometry(fr, c);
  if (rc != MH_OK) return rc;
  rc = walk_shape(headers, fr->d_frame_code_offsets != nullptr, fr->n_frames, c.re.tiles, (hipStream_t)stream,
                  groups_per_frame);
  if (rc != MH_OK) return rc;
  *waves_per_group = kMaxWavesPerWG;
  return MH_OK;
}

// The planes entries' by-value arguments from the host arrays; false: a bad plane count or pair
// (values at index >= n_planes are not read). One plane ignores the strides.
bool plane_args(uint32_t n_planes, uint32_t plane_frame_stride, const float *scale, const float *bias,
                size_t out_plane_stride, PlaneArgs &pl) {
  if (n_planes == 0 || n_planes > MH_MAX_PLANES || !scale || !bias) return false;
  pl = {};
  for (uint32_t i = 0; i < n_planes; ++i) {
    if (!std::isfinite(scale[i]) || !std::isfinite(bias[i])) return false;
    pl.scale[i] = scale[i];
    pl.bias[i] = bias[i];
  }
  pl.n_planes = n_planes;
  pl.frame_stride = n_planes > 1 ? plane_frame_stride : 0u;
  pl.out_stride = n_planes > 1 ? out_plane_stride : 0u;
  return true;
}
#endif

}  // namespace

extern "C" {

#if !MH_LANE_PAIRS

#if MH_DIAG_STAMPS
int mh_diag_stamps(unsigned long long *host, size_t n) {
  if (n > sizeof(g_stamps) / sizeof(g_stamps[0])) n = sizeof(g_stamps) / sizeof(g_stamps[0]);
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_stamps), n * sizeof(unsigned long long), 0,
                             hipMemcpyDeviceToHost) == hipSuccess ? (int)n : -1;
}
#if MH_DIAG_ROWS
int mh_diag_rows(uint32_t *host, size_t n) {
  if (n > sizeof(g_rows) / sizeof(g_rows[0])) n = sizeof(g_rows) / sizeof(g_rows[0]);
  return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_rows), n * sizeof(uint32_t), 0, hipMemcpyDeviceToHost) == hipSuccess
             ? (int)n : -1;
}
#endif
#endif

#ifdef MH_TABLE_STAMPS  // diagnostic builds: room for the table kernel's phase stamps
size_t mh_lut_bytes(void) { return (size_t)kPreparedBytes + 256; }
#else
size_t mh_lut_bytes(void) { return (size_t)kPreparedBytes; }
#endif
int mh_lut_bits(void) { return kLutBits; }

int mh_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int mh_prepare_lut(const mh_lookup_symbol *d_table1, const mh_lookup_symbol *d_table2,
                   uint32_t table2_entries, uint16_t *d_lut, void *stream) {
  if (!d_table1 || !d_table2 || !d_lut) return MH_ERR_INVALID_ARG;
  if (table2_entries < 256 || (table2_entries % 256) != 0 || table2_entries > MH_TABLE2_MAX_ENTRIES)
    return MH_ERR_TABLE;
  if ((uintptr_t)d_lut & 15u) return MH_ERR_ALIGN;
  hipLaunchKernelGGL(mh_prepare_lut_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream,
                     reinterpret_cast<const uint16_t *>(d_table1),
                     reinterpret_cast<const uint16_t *>(d_table2), table2_entries,
                     reinterpret_cast<uint8_t *>(d_lut));
  return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
}

#endif  // !MH_LANE_PAIRS

// The decode entry point. The lane-pair diagnostic library exports the same body as
// mh_diag_decode_lanepairs (and nothing else): MH_FLAG_LANE_PAIRS is honoured only there;
// mh_decode accepts and ignores it.
#if MH_LANE_PAIRS
int mh_diag_decode_lanepairs(const mh_frame *fr, uint8_t *d_out, size_t out_pitch, size_t out_frame_stride,
                             void *stream) {
  const uint32_t *d_mid_marks = nullptr;
#else
int mh_decode(const mh_frame *fr, uint8_t *d_out, size_t out_pitch, size_t out_frame_stride,
              void *stream) {
  return mh_decode_marked(fr, nullptr, d_out, out_pitch, out_frame_stride, stream);
}

// mh_decode's body; the marks (optional) reach the single-frame launch alone.
int mh_decode_marked(const mh_frame *fr, const uint32_t *d_mid_marks, uint8_t *d_out, size_t out_pitch,
                     size_t out_frame_stride, void *stream) {
#endif
  // MH_FLAG_LANE_PAIRS: honoured by the diagnostic library only; the product library accepts
  // it (callers built against round-4 libraries pass it) and decodes with the default kernels
  DecodeCall c{DecodeCall::kInFrame};
  c.allowed_flags |= MH_FLAG_LANE_PAIRS;
  c.words = (uintptr_t)d_mid_marks;  // 4-byte aligned, judged with the other alignments
  int rc = check_decode_args(fr, d_out, out_pitch, out_frame_stride, c);
  if (rc != MH_OK) return rc;
  DecodeArgs a{};
  a.t1 = reinterpret_cast<const uint16_t *>(fr->d_table1);
  a.t2 = reinterpret_cast<const uint16_t *>(fr->d_table2);
  a.lut = fr->d_lut;
  a.t2_entries = fr->table2_entries;
  rc = fill_decode_args(fr, d_out, out_pitch, out_frame_stride, a, c);
  if (rc != MH_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool lp = (fr->flags & MH_FLAG_LANE_PAIRS) != 0;
  const bool ao = (fr->flags & MH_FLAG_ANY_ORDER) != 0;
  return (fr->flags & MH_FLAG_NO_DELTA) ? launch<false>(a, s, lp, ao, d_mid_marks)
                                        : launch<true>(a, s, lp, ao, d_mid_marks);
}

#if !MH_LANE_PAIRS
// The frame-slice entries. Each is its DecodeCall, the prologue and one launch of its row of
// kSliceTable with its own trailing scalars (the list entries: a ListCall and decode_list); each
// *_shape twin is the same call without tables.
int mh_decode_frames(const mh_frame *fr, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                     const int32_t *d_frame_status, uint8_t *d_out, size_t out_pitch, size_t out_frame_stride,
                     void *stream) {
  DecodeCall c{DecodeCall::kPrepared, d_luts, lut_stride_bytes};
  SliceArgs p;
  const int rc = slice_prologue(fr, d_out, out_pitch, out_frame_stride, c, p);
  if (rc != MH_OK) return rc;
  return launch_slices<FramesFn>(kSliceFrames, c, p, stream, reinterpret_cast<const uint8_t *>(d_luts),
                                 d_frame_status, lut_stride_bytes);
}

int mh_decode_frames_shape(const mh_frame *fr, void *stream, uint32_t *groups_per_frame,
                           uint32_t *waves_per_group) {
  return slice_shape_entry(kSliceFrames, fr, {DecodeCall::kPrepared}, stream, groups_per_frame, waves_per_group);
}

int mh_decode_headers(const mh_frame *fr, const uint8_t *d_canon_headers, const int32_t *d_frame_status,
                      int32_t *d_header_status, uint8_t *d_out, size_t out_pitch, size_t out_frame_stride,
                      void *stream) {
  if (d_header_status && d_header_status == d_frame_status) return MH_ERR_INVALID_ARG;
  DecodeCall c{DecodeCall::kHeaders, d_canon_headers};
  SliceArgs p;
  const int rc = slice_prologue(fr, d_out, out_pitch, out_frame_stride, c, p);
  if (rc != MH_OK) return rc;
  return launch_slices<HeadersFn>(kSliceHeaders, c, p, stream, d_canon_headers, d_frame_status, d_header_status);
}

int mh_decode_headers_shape(const mh_frame *fr, void *stream, uint32_t *groups_per_frame,
                            uint32_t *waves_per_group) {
  return slice_shape_entry(kSliceHeaders, fr, {DecodeCall::kHeaders}, stream, groups_per_frame, waves_per_group);
}

// The region at scale 2^log2_scale, same tiles and launch-shape rule at every scale: 0 is the region
// kernel itself (mh_decode_region); 1..3 are the region kernel with the box-filter output stage (BoxRows).
int mh_decode_region_scaled(const mh_frame *fr, const mh_region *rg, uint32_t log2_scale, const uint16_t *d_luts,
                            uint64_t lut_stride_bytes, const int32_t *d_frame_status, uint8_t *d_out,
                            size_t out_pitch, size_t out_frame_stride, void *stream) {
  DecodeCall c{DecodeCall::kRegion, d_luts, lut_stride_bytes, rg, log2_scale};
  SliceArgs p;
  const int rc = slice_prologue(fr, d_out, out_pitch, out_frame_stride, c, p);  // c.re.ph = SH: the descriptor's limit
  if (rc != MH_OK) return rc;
  return launch_slices<RegionFn>(kSliceRegion, c, p, stream, reinterpret_cast<const uint8_t *>(d_luts),
                                 d_frame_status, lut_stride_bytes, c.re.segs, rg->bw, rg->bx0, rg->by0);
}

int mh_decode_region(const mh_frame *fr, const mh_region *rg, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                     const int32_t *d_frame_status, uint8_t *d_out, size_t out_pitch, size_t out_frame_stride,
                     void *stream) {
  return mh_decode_region_scaled(fr, rg, 0, d_luts, lut_stride_bytes, d_frame_status, d_out, out_pitch,
                                 out_frame_stride, stream);
}

int mh_decode_region_scaled_shape(const mh_frame *fr, const mh_region *rg, uint32_t log2_scale, void *stream,
                                  uint32_t *groups_per_frame, uint32_t *waves_per_group) {
  return slice_shape_entry(kSliceRegion, fr, {DecodeCall::kRegion, nullptr, 0, rg, log2_scale}, stream,
                           groups_per_frame, waves_per_group);
}

int mh_decode_region_shape(const mh_frame *fr, const mh_region *rg, void *stream, uint32_t *groups_per_frame,
                           uint32_t *waves_per_group) {
  return mh_decode_region_scaled_shape(fr, rg, 0, stream, groups_per_frame, waves_per_group);
}

// A list of windows of one size, each with its own frame and origin, at scale 2^log2_scale: the
// region kernel's body with a map read from the window's descriptor (WindowMap); n_windows stands
// where n_frames does in the launch-shape rule and the grid. Scale 0 is the windows kernel itself
// (mh_decode_windows); 1..3 are the windows kernel with the box-filter output stage, every slot a
// raster of c bw x c bh (c = 8 >> log2_scale).
int mh_decode_windows_scaled(const mh_frame *fr, const mh_window *d_windows, uint32_t n_windows, uint32_t bw,
                             uint32_t bh, uint32_t log2_scale, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                             const int32_t *d_frame_status, int32_t *d_window_status, uint8_t *d_out,
                             size_t out_pitch, size_t out_window_stride, void *stream) {
  ListCall c(DecodeCall::kWindows, bw, bh, log2_scale, n_windows, d_windows, d_luts, lut_stride_bytes);
  return decode_list<WindowsFn>(kSliceWindows, fr, c, d_windows, d_frame_status, d_window_status, d_out, out_pitch,
                                out_window_stride, stream, 0u);
}

int mh_decode_windows(const mh_frame *fr, const mh_window *d_windows, uint32_t n_windows, uint32_t bw, uint32_t bh,
                      const uint16_t *d_luts, uint64_t lut_stride_bytes, const int32_t *d_frame_status,
                      int32_t *d_window_status, uint8_t *d_out, size_t out_pitch, size_t out_window_stride,
                      void *stream) {
  return mh_decode_windows_scaled(fr, d_windows, n_windows, bw, bh, 0, d_luts, lut_stride_bytes, d_frame_status,
                                  d_window_status, d_out, out_pitch, out_window_stride, stream);
}

int mh_decode_windows_scaled_shape(const mh_frame *fr, uint32_t n_windows, uint32_t bw, uint32_t bh,
                                   uint32_t log2_scale, void *stream, uint32_t *groups_per_window,
                                   uint32_t *waves_per_group) {
  return slice_shape_entry(kSliceWindows, fr, ListCall(DecodeCall::kWindows, bw, bh, log2_scale, n_windows), stream,
                           groups_per_window, waves_per_group);
}

int mh_decode_windows_shape(const mh_frame *fr, uint32_t n_windows, uint32_t bw, uint32_t bh, void *stream,
                            uint32_t *groups_per_window, uint32_t *waves_per_group) {
  return mh_decode_windows_scaled_shape(fr, n_windows, bw, bh, 0, stream, groups_per_window, waves_per_group);
}

// A list of crops of one pixel size, each with its own frame and PIXEL origin: the windows kernel's
// body with a crop's map and output stage (CropMap, CropRows). The checks are the windows', with
// n_crops rasters of w x h: a pitch that is a multiple of 8 and >= w holds the round_up(w, 8) bytes
// a row is written with.
int mh_decode_crops(const mh_frame *fr, const mh_crop *d_crops, uint32_t n_crops, uint32_t w, uint32_t h,
                    const uint16_t *d_luts, uint64_t lut_stride_bytes, const int32_t *d_frame_status,
                    int32_t *d_crop_status, uint8_t *d_out, size_t out_pitch, size_t out_crop_stride, void *stream) {
  ListCall c(DecodeCall::kCrops, w, h, 0u, n_crops, d_crops, d_luts, lut_stride_bytes);
  return decode_list<CropsFn>(kSliceCrops, fr, c, d_crops, d_frame_status, d_crop_status, d_out, out_pitch,
                              out_crop_stride, stream, 0u);
}

int mh_decode_crops_shape(const mh_frame *fr, uint32_t n_crops, uint32_t w, uint32_t h, void *stream,
                          uint32_t *groups_per_crop, uint32_t *waves_per_group) {
  return slice_shape_entry(kSliceCrops, fr, ListCall(DecodeCall::kCrops, w, h, 0u, n_crops), stream, groups_per_crop,
                           waves_per_group);
}

// The crops decoded straight into normalised elements: the crops kernel's entry and body with the
// NormRows output stage, one row of kSliceTable per format. The checks are mh_decode_crops' through
// the same helpers, with the format's element size in the raster rules and 16-byte row stores.
int mh_decode_crops_norm(const mh_frame *fr, const mh_norm_crop *d_crops, uint32_t n_crops, uint32_t w, uint32_t h,
                         uint32_t format, float scale, float bias, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                         const int32_t *d_frame_status, int32_t *d_crop_status, void *d_out, size_t out_pitch,
                         size_t out_crop_stride, void *stream) {
  ListCall c(DecodeCall::kNormCrops, w, h, 0u, n_crops, d_crops, d_luts, lut_stride_bytes);
  c.format = format;
  c.scale = scale;
  c.bias = bias;
  return decode_list<NormCropsFn>(kSliceNormCrops, fr, c, d_crops, d_frame_status, d_crop_status, d_out, out_pitch,
                                  out_crop_stride, stream, 0u, scale, bias, (w & 7u) ? 1u : 0u);
}

int mh_decode_crops_norm_shape(const mh_frame *fr, uint32_t n_crops, uint32_t w, uint32_t h, uint32_t format,
                               void *stream, uint32_t *groups_per_crop, uint32_t *waves_per_group) {
  ListCall c(DecodeCall::kNormCrops, w, h, 0u, n_crops);
  c.format = format;
  return slice_shape_entry(kSliceNormCrops, fr, c, stream, groups_per_crop, waves_per_group);
}

// Samples of n_planes planes into normalised [n, C, h, w] rasters: the normalised crops' checks with
// the planes' rules beside them (DecodeCall::n_planes), n_crops * n_planes units in the shape rule and
// the grid, and the planes kernel's rows of kSliceTable. The pairs are read here and travel by value.
// A bad plane count or pair is reported ahead of the dims, as a bad format is; one plane is
// mh_decode_crops_norm's call, the plane strides ignored.
int mh_decode_crops_norm_planes(const mh_frame *fr, const mh_norm_crop *d_crops, uint32_t n_crops, uint32_t w,
                                uint32_t h, uint32_t format, uint32_t n_planes, uint32_t plane_frame_stride,
                                const float *scale, const float *bias, const uint16_t *d_luts,
                                uint64_t lut_stride_bytes, const int32_t *d_frame_status, int32_t *d_crop_status,
                                void *d_out, size_t out_pitch, size_t out_plane_stride, size_t out_crop_stride,
                                void *stream) {
  PlaneArgs pl;
  if (!plane_args(n_planes, plane_frame_stride, scale, bias, out_plane_stride, pl)) return MH_ERR_INVALID_ARG;
  ListCall c(DecodeCall::kNormCrops, w, h, 0u, n_crops, d_crops, d_luts, lut_stride_bytes);
  c.planes(format, n_planes, &pl);
  // the kernel's p_max_frame = n_frames - 1 - (n_planes - 1) * frame_stride (call_geometry: it does not wrap)
  return decode_list<PlanesFn>(kSlicePlanes, fr, c, d_crops, d_frame_status, d_crop_status, d_out, out_pitch,
                               out_crop_stride, stream, 1u + (n_planes - 1u) * pl.frame_stride, (w & 7u) ? 1u : 0u, pl);
}

int mh_decode_crops_norm_planes_shape(const mh_frame *fr, uint32_t n_crops, uint32_t w, uint32_t h, uint32_t format,
                                      uint32_t n_planes, void *stream, uint32_t *groups_per_plane,
                                      uint32_t *waves_per_group) {
  if (n_planes == 0 || n_planes > MH_MAX_PLANES) return MH_ERR_INVALID_ARG;
  return slice_shape_entry(kSlicePlanes, fr,
                           ListCall(DecodeCall::kNormCrops, w, h, 0u, n_crops).planes(format, n_planes), stream,
                           groups_per_plane, waves_per_group);
}

// The crop entries over a frame set: their parents' calls with ListCall::over_set, the set kernels'
// rows and the geometry records as the kernels' last scalar. The prologue sizes the rasters and the
// grid from dims, the set's maxima; every workgroup takes its frame's own grid from its record.
int mh_decode_set_crops(const mh_frame *fr, const mh_frame_geom *d_geoms, uint32_t total_blocks,
                        const mh_crop *d_crops, uint32_t n_crops, uint32_t w, uint32_t h, const uint16_t *d_luts,
                        uint64_t lut_stride_bytes, const int32_t *d_frame_status, int32_t *d_crop_status,
                        uint8_t *d_out, size_t out_pitch, size_t out_crop_stride, void *stream) {
  ListCall c(DecodeCall::kCrops, w, h, 0u, n_crops, d_crops, d_luts, lut_stride_bytes);
  c.over_set(d_geoms, total_blocks);
  return decode_list<SetCropsFn>(kSliceSetCrops, fr, c, d_crops, d_frame_status, d_crop_status, d_out, out_pitch,
                                 out_crop_stride, stream, 0u, d_geoms);
}

int mh_decode_set_crops_shape(const mh_frame *fr, uint32_t n_crops, uint32_t w, uint32_t h, void *stream,
                              uint32_t *groups_per_crop, uint32_t *waves_per_group) {
  return slice_shape_entry(kSliceSetCrops, fr, ListCall(DecodeCall::kCrops, w, h, 0u, n_crops).over_set(), stream,
                           groups_per_crop, waves_per_group);
}

int mh_decode_set_crops_norm_planes(const mh_frame *fr, const mh_frame_geom *d_geoms, uint32_t total_blocks,
                                    const mh_norm_crop *d_crops, uint32_t n_crops, uint32_t w, uint32_t h,
                                    uint32_t format, uint32_t n_planes, uint32_t plane_frame_stride,
                                    const float *scale, const float *bias, const uint16_t *d_luts,
                                    uint64_t lut_stride_bytes, const int32_t *d_frame_status,
                                    int32_t *d_crop_status, void *d_out, size_t out_pitch, size_t out_plane_stride,
                                    size_t out_crop_stride, void *stream) {
  PlaneArgs pl;
  if (!plane_args(n_planes, plane_frame_stride, scale, bias, out_plane_stride, pl)) return MH_ERR_INVALID_ARG;
  ListCall c(DecodeCall::kNormCrops, w, h, 0u, n_crops, d_crops, d_luts, lut_stride_bytes);
  c.over_set(d_geoms, total_blocks).planes(format, n_planes, &pl);
  return decode_list<SetPlanesFn>(kSliceSetPlanes, fr, c, d_crops, d_frame_status, d_crop_status, d_out, out_pitch,
                                  out_crop_stride, stream, 1u + (n_planes - 1u) * pl.frame_stride,
                                  (w & 7u) ? 1u : 0u, pl, d_geoms);
}

int mh_decode_set_crops_norm_planes_shape(const mh_frame *fr, uint32_t n_crops, uint32_t w, uint32_t h,
                                          uint32_t format, uint32_t n_planes, void *stream,
                                          uint32_t *groups_per_plane, uint32_t *waves_per_group) {
  if (n_planes == 0 || n_planes > MH_MAX_PLANES) return MH_ERR_INVALID_ARG;
  return slice_shape_entry(kSliceSetPlanes, fr,
                           ListCall(DecodeCall::kNormCrops, w, h, 0u, n_crops).over_set().planes(format, n_planes),
                           stream, groups_per_plane, waves_per_group);
}

// The whole frames of a set: the checks are the set crops' (a prepared-table call over a set, with the
// records and the group map where the descriptors are and no pitch or stride to judge), and the grid
// is the caller's group map, one workgroup per word. dims carry the set's maxima and size nothing.
int mh_decode_set_frames(const mh_frame *fr, const mh_frame_geom *d_geoms, uint32_t total_blocks,
                         const mh_set_raster *d_rasters, const mh_set_share *d_shares, const uint32_t *d_group_frame,
                         uint32_t n_groups, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                         const int32_t *d_frame_status, int32_t *d_set_status, uint8_t *d_out, uint64_t out_bytes,
                         void *stream) {
  if (d_set_status && d_set_status == d_frame_status) return MH_ERR_INVALID_ARG;
  DecodeCall c{DecodeCall::kPrepared, d_luts, lut_stride_bytes};
  c.set = c.set_frames = true;
  c.geoms = d_geoms;
  c.total_blocks = total_blocks;
  c.rasters = d_rasters;
  c.shares = d_shares;
  c.group_frame = d_group_frame;
  c.n_groups = n_groups;
  c.out_bytes = out_bytes;
  const int rc = check_decode_args(fr, d_out, 0, 0, c);
  if (rc != MH_OK) return rc;
  DecodeArgs a{};
  a.offsets = fr->d_block_offsets;
  a.codes = fr->d_codes;
  a.frame_off = fr->d_frame_code_offsets;
  a.codes_bytes = fr->codes_bytes;
  a.block_init = fr->d_block_init;
  a.out = d_out;
  const bool delta = !(fr->flags & MH_FLAG_NO_DELTA), any_order = (fr->flags & MH_FLAG_ANY_ORDER) != 0;
  const SetFramesFn kernel = reinterpret_cast<SetFramesFn>(kSliceTable[kSliceSetFrames].fn[delta ? 1 : 0]);
  MH_LAUNCH(kernel, dim3(n_groups), dim3(kMaxWavesPerWG * 64), (hipStream_t)stream, any_order, a.offsets, a.frame_off,
            a.block_init, reinterpret_cast<const uint8_t *>(d_luts), d_frame_status, d_group_frame, total_blocks,
            fr->n_frames, lut_stride_bytes, d_set_status, d_geoms, d_rasters, d_shares, out_bytes, a);
  return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
}

// The planner's budget: the workgroups of the set-frames kernel resident on the device at once (CUs x
// its occupancy, groups_for's R) and the waves of one. No launch.
int mh_decode_set_frames_shape(const mh_frame *fr, void *stream, uint32_t *resident_groups,
                               uint32_t *waves_per_group) {
  if (!fr || !resident_groups || !waves_per_group) return MH_ERR_INVALID_ARG;
  if (fr->flags & ~(MH_FLAG_NO_DELTA | MH_FLAG_ANY_ORDER)) return MH_ERR_INVALID_ARG;
  const DeviceInfo *di = device_info((hipStream_t)stream);
  if (!di) return MH_ERR_HIP;
  const uint64_t r = (uint64_t)di->cus.load(std::memory_order_relaxed) *
                     (uint64_t)di->occ_slice[kSliceSetFrames][(fr->flags & MH_FLAG_NO_DELTA) ? 0 : 1];
  *resident_groups = (uint32_t)r;
  *waves_per_group = kMaxWavesPerWG;
  return MH_OK;
}

// mh_check's report, frame by frame under the frame's own table, and a verdict word per frame that
// the entries above take as d_frame_status (slice_walk).
int mh_check_frames(const mh_frame *fr, const uint16_t *d_luts, uint64_t lut_stride_bytes,
                    const int32_t *d_frame_status, uint32_t *d_report, int32_t *d_verdict, void *stream) {
  return check_walk(fr, false, d_luts, lut_stride_bytes, d_frame_status, nullptr, d_report, d_verdict, stream);
}

int mh_check_frames_shape(const mh_frame *fr, void *stream, uint32_t *groups_per_frame, uint32_t *waves_per_group) {
  return check_walk_shape(fr, false, stream, groups_per_frame, waves_per_group);
}

int mh_check_headers(const mh_frame *fr, const uint8_t *d_canon_headers, const int32_t *d_frame_status,
                     int32_t *d_header_status, uint32_t *d_report, int32_t *d_verdict, void *stream) {
  return check_walk(fr, true, d_canon_headers, 0, d_frame_status, d_header_status, d_report, d_verdict, stream);
}

int mh_check_headers_shape(const mh_frame *fr, void *stream, uint32_t *groups_per_frame, uint32_t *waves_per_group) {
  return check_walk_shape(fr, true, stream, groups_per_frame, waves_per_group);
}

int mh_header_luts_device(const uint8_t *d_canon_headers, uint32_t n_headers, uint16_t *d_luts,
                          uint64_t lut_stride_bytes, int32_t *d_status, void *stream) {
  if (!d_canon_headers || !d_luts || n_headers == 0 || n_headers > 65535u) return MH_ERR_INVALID_ARG;
  if (((uintptr_t)d_luts & 15u) || (lut_stride_bytes & 15u)) return MH_ERR_ALIGN;
  if (lut_stride_bytes < mh_lut_bytes()) return MH_ERR_CAPACITY;
  hipLaunchKernelGGL(mh_header_luts_kernel, dim3(n_headers), dim3(kMaxWavesPerWG * 64), 0, (hipStream_t)stream,
                     d_canon_headers, reinterpret_cast<uint8_t *>(d_luts), lut_stride_bytes, d_status);
  return hipGetLastError() == hipSuccess ? MH_OK : MH_ERR_HIP;
}
#endif  // !MH_LANE_PAIRS

}  // extern "C"
