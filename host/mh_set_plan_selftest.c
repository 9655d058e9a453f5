/* mh_set_plan_selftest.c -- the set encoder's host planner (mh_encode_set_plan, mh_host.cpp) as a
 * stand-alone program: seeded source lists go through the planner into blobs of exactly
 * mh_encode_set_plan_bytes() (at an odd host address every other round), and every record,
 * geometry record and map entry is checked against a straightforward recomputation. Built with the
 * host compiler's AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_set_plan_sanitize.py;
 * plain C, no HIP, no GPU.
 *   mh_set_plan_selftest [seed]   -> "set plan selftest ok" and exit status 0 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/metalhuffman.h"

static uint64_t rng_state;
static uint32_t rnd(void) { /* xorshift64* */
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 2685821237ull * 1000003ull) >> 32);
}
static uint32_t below(uint32_t n) { return rnd() % n; }

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                            \
    }                                                                     \
  } while (0)

static const uint32_t kEdge[][2] = {{1, 1}, {8, 8}, {65535, 8}, {8, 65535}, {2056, 8}, {128, 128}, {264, 256}, {40, 400}};

static void random_source(mh_set_source *s, uint32_t same_stride) {
  memset(s, 0, sizeof(*s));
  if (below(4) == 0) {
    const uint32_t e = below(sizeof(kEdge) / sizeof(kEdge[0]));
    s->width = kEdge[e][0];
    s->height = kEdge[e][1];
  } else {
    s->width = 1 + below(900);
    s->height = 1 + below(700);
  }
  s->pixel_stride = same_stride ? same_stride : 1 + below(below(3) ? 4 : 255);
  s->row_pitch = (uint64_t)s->width * s->pixel_stride + (below(2) ? 0 : below(4096));
  s->pixels = 0x700000000000ull + ((uint64_t)rnd() << 8) + (same_stride ? below(same_stride) : below(4));
  if (same_stride) s->row_pitch = (s->row_pitch + 3) & ~3ull;
  s->codes_cap = 16ull * (1 + below(1u << 16));
}

static void one_round(uint32_t n, uint32_t same_stride, int odd_address) {
  mh_set_source *src = (mh_set_source *)malloc(n * sizeof(*src));
  CHECK(src);
  for (uint32_t f = 0; f < n; ++f) random_source(&src[f], same_stride);
  const size_t bytes = mh_encode_set_plan_bytes(n, src);
  CHECK(bytes > 0);
  uint8_t *raw = (uint8_t *)malloc(bytes + (odd_address ? 1 : 0));  /* exactly: an overrun is a report */
  CHECK(raw);
  uint8_t *plan = raw + (odd_address ? 1 : 0);
  mh_set_totals t;
  CHECK(mh_encode_set_plan(n, src, 0, plan, bytes - 1, &t) == MH_ERR_CAPACITY);
  CHECK(mh_encode_set_plan(n, src, MH_FLAG_NO_DELTA | MH_ENCODE_LIMIT_LENGTHS, plan, bytes, &t) == MH_OK);
  CHECK(t.plan_bytes == bytes && t.n_frames == n);
  CHECK(t.geoms_offset % 16 == 0 && t.split_map_offset % 16 == 0 && t.pack_map_offset % 16 == 0);
  CHECK(t.geoms_offset == (uint64_t)n * sizeof(mh_set_frame));
  CHECK(t.split_map_offset >= t.geoms_offset + (uint64_t)n * sizeof(mh_frame_geom));
  CHECK(t.pack_map_offset >= t.split_map_offset + 8ull * t.split_grid && bytes >= t.pack_map_offset + 8ull * t.pack_grid);
  uint64_t slot = 0, blocks = 0, tiles = 0, units = 0;
  uint32_t wmax = 0, hmax = 0, dword = 1;
  for (uint32_t f = 0; f < n; ++f) {
    mh_set_frame r;
    mh_frame_geom g;
    memcpy(&r, plan + (size_t)f * sizeof(r), sizeof(r));
    memcpy(&g, plan + t.geoms_offset + (size_t)f * sizeof(g), sizeof(g));
    const uint32_t bw = (src[f].width + 7) / 8, nb = bw * ((src[f].height + 7) / 8);
    const uint32_t nt = (nb + MH_SET_TILE_BLOCKS - 1) / MH_SET_TILE_BLOCKS;
    CHECK(r.pixels == src[f].pixels && r.codes_cap == src[f].codes_cap && r.slot_offset == slot);
    CHECK(r.row_pitch == (src[f].height > 1 ? src[f].row_pitch : 0) && r.pixel_stride == src[f].pixel_stride);
    CHECK(r.width == src[f].width && r.height == src[f].height && r.block_width == bw && r.n_blocks == nb);
    CHECK(r.n_tiles == nt && r.first_tile == tiles && r.first_block == blocks && r.reserved == 0);
    CHECK(g.first_block == blocks && g.width == src[f].width && g.height == src[f].height && g.reserved == 0);
    for (uint32_t k = 0; k < nt; ++k) {
      uint32_t e[2];
      memcpy(e, plan + t.split_map_offset + (size_t)(tiles + k) * 8, 8);
      CHECK(e[0] == f && e[1] == k);
    }
    for (uint32_t k = 0; k < nt; k += MH_SET_PACK_TILES, ++units) {
      uint32_t e[2];
      CHECK(units < t.pack_grid);
      memcpy(e, plan + t.pack_map_offset + (size_t)units * 8, 8);
      CHECK(e[0] == f && e[1] == k);
    }
    slot += src[f].codes_cap;
    blocks += nb;
    tiles += nt;
    if (src[f].width > wmax) wmax = src[f].width;
    if (src[f].height > hmax) hmax = src[f].height;
    if (src[f].pixel_stride != src[0].pixel_stride || src[f].pixel_stride > 4 ||
        (src[f].pixels & 3) >= src[f].pixel_stride ||
        (src[f].height > 1 && (src[f].row_pitch & 3)))
      dword = 0;
  }
  CHECK(t.codes_bytes == slot && t.total_blocks == blocks && t.total_tiles == tiles && t.split_grid == tiles);
  CHECK(t.pack_grid == units && t.max_width == wmax && t.max_height == hmax);
  CHECK(t.fetch_mode == (dword ? src[0].pixel_stride : MH_SET_FETCH_BYTES));
  CHECK(t.workspace_bytes >= (uint64_t)n * (1024 + 256) + tiles * (512 + 64) + (tiles + n) * 4);
  /* the refusals leave the blob alone: one record spoilt per check, the earlier check wins */
  uint8_t *copy = (uint8_t *)malloc(bytes);
  CHECK(copy);
  memcpy(copy, plan, bytes);
  const uint32_t v = below(n), u = below(n);
  mh_set_source keep_v = src[v], keep_u = src[u];
  src[v].codes_cap += 8;
  CHECK(mh_encode_set_plan(n, src, 0, plan, bytes, &t) == MH_ERR_ALIGN);
  src[u].width = 0;
  CHECK(mh_encode_set_plan(n, src, 0, plan, bytes, &t) == MH_ERR_DIMS);
  src[v].reserved = 1;
  CHECK(mh_encode_set_plan(n, src, 0, plan, bytes, &t) == MH_ERR_INVALID_ARG);
  CHECK(mh_encode_set_plan_bytes(n, src) == 0);
  src[v] = keep_v;
  src[u] = keep_u;
  if (src[v].height > 1) {
    src[v].row_pitch = (uint64_t)src[v].width * src[v].pixel_stride - 1;
    CHECK(mh_encode_set_plan(n, src, 0, plan, bytes, &t) == MH_ERR_CAPACITY);
    src[v] = keep_v;
  }
  CHECK(mh_encode_set_plan(n, src, 0x40u, plan, bytes, &t) == MH_ERR_INVALID_ARG);
  CHECK(memcmp(copy, plan, bytes) == 0);
  free(copy);
  free(raw);
  free(src);
}

int main(int argc, char **argv) {
  rng_state = 0x9E3779B97F4A7C15ull ^ (argc > 1 ? strtoull(argv[1], NULL, 10) : 1);
  mh_set_totals t;
  mh_set_source one = {0x1000, 8, 1, 8, 8, 0, 16};
  uint8_t small[256];
  CHECK(mh_encode_set_plan(0, &one, 0, small, sizeof(small), &t) == MH_ERR_INVALID_ARG);
  CHECK(mh_encode_set_plan(1, NULL, 0, small, sizeof(small), &t) == MH_ERR_INVALID_ARG);
  CHECK(mh_encode_set_plan(1, &one, 0, NULL, sizeof(small), &t) == MH_ERR_INVALID_ARG);
  CHECK(mh_encode_set_plan(1, &one, 0, small, sizeof(small), NULL) == MH_ERR_INVALID_ARG);
  CHECK(mh_encode_set_plan_bytes(1, &one) == 64 + 16 + 16 + 16);
  CHECK(mh_encode_set_plan(1, &one, 0, small, sizeof(small), &t) == MH_OK && t.total_blocks == 1 && t.fetch_mode == 1);
  for (uint32_t round = 0; round < 200; ++round) {
    const uint32_t n = 1 + below(round % 10 == 0 ? 300 : 12);
    one_round(n, round % 3 == 0 ? 1 + below(4) : 0, (int)(round & 1));
  }
  printf("set plan selftest ok\n");
  return 0;
}
