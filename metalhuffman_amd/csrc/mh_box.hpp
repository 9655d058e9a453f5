// mh_box.hpp -- the rounding of the box filter (mh_decode_region_scaled, mh_box_reduce), compiled
// by the host codec (g++) and by the decode kernels (hipcc) alike: one definition, two callers.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MH_BOX_FN __host__ __device__ __forceinline__
#else
#define MH_BOX_FN inline
#endif

// The mean of n pixels whose sum is `sum`, halves rounded up: floor((2 sum + n) / (2 n)).
// sum <= 255 n and n <= 64, so 2 sum + n < 2^15. n = 0 (a cell wholly outside the frame) comes
// with sum = 0 and gives 0: the divisor is then 1, so no select is needed.
// (The masks state those ranges: a compiler that knows both operands fit 24 bits divides them
// through a float reciprocal plus one correction -- a third of the general 32-bit division's
// code. Both functions are minima and maxima, not selects: in the kernels every live comparison
// result is a pair of SGPRs, and the decode chain has none to spare.)
MH_BOX_FN uint32_t mh_box_round(uint32_t sum, uint32_t n) {
  sum &= 0x3FFFu;
  n &= 0x7Fu;
  const uint32_t d = 2u * n;
  return (2u * sum + n) / (d > 1u ? d : 1u);
}

// In-frame pixels of cell `i` (0 .. 8/s - 1) along one axis of a block that has `live` (0..8)
// in-frame pixels on that axis; cells are s = 1 << log2_scale pixels wide.
MH_BOX_FN uint32_t mh_box_cell_live(uint32_t live, uint32_t i, uint32_t log2_scale) {
  const int s = 1 << log2_scale;
  int d = (int)live - (int)(i << log2_scale);
  d = d > 0 ? d : 0;
  return (uint32_t)(d < s ? d : s);
}
