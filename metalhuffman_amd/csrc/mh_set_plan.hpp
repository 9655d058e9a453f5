// mh_set_plan.hpp -- what the set encoder's planner (mh_host.cpp, pure host C++) and its
// kernels and entry (mh_encode.hip) share: the tile sizes behind the plan's maps and the
// carve of the workspace, whose size the planner reports and the entry checks.
#ifndef MH_SET_PLAN_HPP
#define MH_SET_PLAN_HPP

#include <stdint.h>

#include "../../include/metalhuffman.h"

namespace mh_set {

constexpr uint32_t kTileBlocks = 256;  // mh_encode.hip: kBatchTile
constexpr uint32_t kPackTiles = 4;     // mh_encode.hip: kPackWaves (tiles of one frame per pack workgroup)
constexpr uint32_t kMetaWords = 32;    // mh_encode.hip: kMetaWords
constexpr uint32_t kByteMode = 0xFFu;  // mh_set_totals.fetch_mode: one byte load per sample (kBytePs)

constexpr uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
constexpr uint64_t align16(uint64_t x) { return (x + 15) & ~15ull; }

// The batched path's workspace parts (carve_batch) with per-frame parts indexed by the frame and
// per-tile parts by the plan's first-tile prefix: frame f's tile t is entry first_tile_f + t, and
// its ncode_f + 1 tile offsets start at entry first_tile_f + f.
struct Workspace {
  uint32_t *table;      // n x 256
  uint64_t *meta;       // n x kMetaWords
  uint16_t *tile_hist;  // tiles x 256
  uint32_t *tile_off;   // tiles + n
  uint64_t *tile_tail;  // tiles x 8
};

inline uint64_t carve(uint8_t *base, uint64_t n, uint64_t tiles, Workspace *w) {
  uint64_t o = 0;
  if (w) w->table = reinterpret_cast<uint32_t *>(base + o);
  o += align256(n * 256 * 4);
  if (w) w->meta = reinterpret_cast<uint64_t *>(base + o);
  o += align256(n * kMetaWords * 8);
  if (w) w->tile_hist = reinterpret_cast<uint16_t *>(base + o);
  o += align256(tiles * 256 * 2);
  if (w) w->tile_off = reinterpret_cast<uint32_t *>(base + o);
  o += align256((tiles + n) * 4);
  if (w) w->tile_tail = reinterpret_cast<uint64_t *>(base + o);
  o += align256(tiles * 64);
  return o;
}

}  // namespace mh_set

#endif
