/* mh_decode_set_plan_selftest.c -- the host planner of mh_decode_set_frames (mh_decode_set_plan,
 * mh_host.cpp) as a stand-alone program: seeded sets go through the sizing call and then the
 * planner into arrays of exactly the reported sizes, and every raster, share and map word is
 * checked against a straightforward recomputation and against the device's validation rules. Built
 * with the host compiler's AddressSanitizer and UndefinedBehaviorSanitizer by
 * tests/test_decode_set_plan_sanitize.py; plain C, no HIP, no GPU.
 *   mh_decode_set_plan_selftest [seed]   -> "decode set plan selftest ok" and exit status 0 */
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

static const uint32_t kEdge[][2] = {{1, 1},   {8, 8},     {9, 7},     {512, 8},     {520, 8},
                                    {8, 520}, {264, 40},  {65535, 1}, {1, 65535},   {4096, 4096}};
static const uint32_t kAlign[] = {0, 1, 8, 16, 64, 4096};
static const uint32_t kBudget[] = {1, 2, 31, 256, 1024, 2048, 65536, 0xFFFFFFFFu};

static uint64_t tiles_of(const mh_frame_geom *g) {
  return ((uint64_t)((g->width + 7) / 8) * ((g->height + 7) / 8) + 63) / 64;
}

static void one_round(uint32_t n) {
  mh_frame_geom *geo = (mh_frame_geom *)malloc(n * sizeof(*geo));
  CHECK(geo);
  uint64_t blocks = 0, sum = 0;
  for (uint32_t f = 0; f < n; ++f) {
    memset(&geo[f], 0, sizeof(geo[f]));
    if (below(4) == 0) {
      const uint32_t e = below(sizeof(kEdge) / sizeof(kEdge[0]));
      geo[f].width = kEdge[e][0];
      geo[f].height = kEdge[e][1];
    } else {
      geo[f].width = 1 + below(2100);
      geo[f].height = 1 + below(1600);
    }
    geo[f].first_block = (uint32_t)blocks;
    blocks += (uint64_t)((geo[f].width + 7) / 8) * ((geo[f].height + 7) / 8);
    sum += tiles_of(&geo[f]);
  }
  CHECK(blocks <= 0xFFFFFFFFull);
  const uint32_t align = kAlign[below(sizeof(kAlign) / sizeof(kAlign[0]))];
  const uint32_t budget = kBudget[below(sizeof(kBudget) / sizeof(kBudget[0]))];
  const uint64_t A = align > 8 ? align : 8;
  uint32_t n_groups = 0, again = 0;
  uint64_t out_bytes = 0, bytes_again = 0;
  CHECK(mh_decode_set_plan(n, geo, budget, align, NULL, NULL, NULL, 0, &n_groups, &out_bytes) == MH_ERR_CAPACITY);
  CHECK(n_groups >= n && out_bytes > 0);
  /* exactly the reported sizes: an overrun is a sanitizer report */
  mh_set_raster *ras = (mh_set_raster *)malloc(n * sizeof(*ras));
  mh_set_share *sh = (mh_set_share *)malloc(n * sizeof(*sh));
  uint32_t *map = (uint32_t *)malloc((size_t)n_groups * sizeof(*map));
  CHECK(ras && sh && map);
  memset(map, 0xEE, (size_t)n_groups * sizeof(*map));
  CHECK(mh_decode_set_plan(n, geo, budget, align, ras, sh, map, n_groups - 1, &again, &bytes_again) == MH_ERR_CAPACITY);
  CHECK(again == n_groups && bytes_again == out_bytes && map[0] == 0xEEEEEEEEu);
  CHECK(mh_decode_set_plan(n, geo, budget, align, ras, sh, map, n_groups, &again, &bytes_again) == MH_OK);
  CHECK(again == n_groups && bytes_again == out_bytes);
  uint64_t end = 0, first = 0;
  for (uint32_t f = 0; f < n; ++f) {
    const uint64_t W = geo[f].width, H = geo[f].height, rw = (W + 7) / 8 * 8, t = tiles_of(&geo[f]);
    const uint64_t cap = (t + MH_DECODE_GROUP_WAVES - 1) / MH_DECODE_GROUP_WAVES;
    uint64_t want = (2ull * budget * t + sum) / (2ull * sum);
    want = want < 1 ? 1 : want > cap ? cap : want;
    CHECK(ras[f].reserved == 0 && ras[f].pitch == (W + A - 1) / A * A && ras[f].offset == (end + A - 1) / A * A);
    /* the device's raster rules */
    CHECK(ras[f].offset % 8 == 0 && ras[f].pitch % 8 == 0 && ras[f].pitch >= rw && ras[f].pitch <= (1u << 20));
    CHECK(ras[f].offset + (H - 1) * ras[f].pitch + rw <= out_bytes);
    end = ras[f].offset + H * ras[f].pitch;
    CHECK(sh[f].reserved[0] == 0 && sh[f].reserved[1] == 0);
    CHECK(sh[f].first_group == first && sh[f].groups == want && sh[f].groups >= 1 && sh[f].groups <= (1u << 20));
    for (uint64_t k = 0; k < want; ++k) CHECK(map[first + k] == f);
    first += want;
  }
  CHECK(end == out_bytes && first == n_groups);
  /* the refusals write nothing: one record spoilt per check */
  uint32_t *copy = (uint32_t *)malloc((size_t)n_groups * sizeof(*map));
  CHECK(copy);
  memcpy(copy, map, (size_t)n_groups * sizeof(*map));
  const uint32_t v = below(n);
  const mh_frame_geom keep = geo[v];
  geo[v].width = 0;
  CHECK(mh_decode_set_plan(n, geo, budget, align, ras, sh, map, n_groups, &again, &bytes_again) == MH_ERR_DIMS);
  geo[v] = keep;
  geo[v].height = 65536;
  CHECK(mh_decode_set_plan(n, geo, budget, align, ras, sh, map, n_groups, &again, &bytes_again) == MH_ERR_DIMS);
  geo[v] = keep;
  geo[v].reserved = 1;
  CHECK(mh_decode_set_plan(n, geo, budget, align, ras, sh, map, n_groups, &again, &bytes_again) == MH_ERR_DIMS);
  geo[v] = keep;
  CHECK(mh_decode_set_plan(n, geo, 0, align, ras, sh, map, n_groups, &again, &bytes_again) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(n, geo, budget, 24, ras, sh, map, n_groups, &again, &bytes_again) == MH_ERR_INVALID_ARG);
  CHECK(memcmp(copy, map, (size_t)n_groups * sizeof(*map)) == 0);
  free(copy);
  free(map);
  free(sh);
  free(ras);
  free(geo);
}

int main(int argc, char **argv) {
  rng_state = 0x9E3779B97F4A7C15ull ^ (argc > 1 ? strtoull(argv[1], NULL, 10) : 1);
  const mh_frame_geom one = {0, 9, 7, 0};
  mh_set_raster r;
  mh_set_share s;
  uint32_t m[1], ng = 0;
  uint64_t ob = 0;
  CHECK(sizeof(mh_set_raster) == 16 && sizeof(mh_set_share) == 16);
  CHECK(mh_decode_set_plan(0, &one, 1, 0, &r, &s, m, 1, &ng, &ob) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(1, NULL, 1, 0, &r, &s, m, 1, &ng, &ob) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(1, &one, 1, 0, NULL, &s, m, 1, &ng, &ob) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(1, &one, 1, 0, &r, NULL, m, 1, &ng, &ob) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(1, &one, 1, 0, &r, &s, NULL, 1, &ng, &ob) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(1, &one, 1, 0, &r, &s, m, 1, NULL, &ob) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(1, &one, 1, 0, &r, &s, m, 1, &ng, NULL) == MH_ERR_INVALID_ARG);
  CHECK(mh_decode_set_plan(1, &one, 1, 0, &r, &s, m, 1, &ng, &ob) == MH_OK);
  CHECK(ng == 1 && ob == 7 * 16 && r.offset == 0 && r.pitch == 16 && s.first_group == 0 && s.groups == 1 && m[0] == 0);
  for (uint32_t round = 0; round < 200; ++round) one_round(1 + below(round % 10 == 0 ? 300 : 12));
  printf("decode set plan selftest ok\n");
  return 0;
}
