/* mh_mid_marks_selftest.c -- the two host functions of the mid-block marks (mh_host.cpp:
 * mh_encode_frame_marks, mh_mid_marks), meant to be built with the host compiler's
 * AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_mid_marks_sanitize.py). No GPU and
 * no HIP: it links mh_host.cpp only.
 *
 * Per case (size, picture kind, format):
 *   mh_encode_frame_marks writes the bytes mh_encode_frame writes (codes, offsets, header, init);
 *   its marks equal mh_mid_marks' over the frame's own tables, and equal the marks computed here
 *   from the picture and the code lengths (bits: the lengths of the block's first 32 symbols;
 *   prev: pixel 31 of the padded block, 0 without deltas); bits <= 512 and the top byte is 0.
 *   Then the code bytes and the offsets are scrambled and walked again: only memory safety and
 *   the two bounds are checked (bytes past codes_bytes read as zero).
 * Prints one line per failure and "selftest ok <cases>" at the end; exit status 0 iff ok. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/metalhuffman.h"

static uint64_t rng_state;
static uint32_t rnd(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 11);
}

/* kinds: 0 smooth gradient + small noise, 1 uniform random bytes, 2 constant, 3 two levels,
 * 4 Fibonacci-skewed noise (codes up to 16 bits; deeper trees take the limited lengths) */
static void make_picture(uint8_t *img, uint32_t w, uint32_t h, int kind) {
  for (uint32_t y = 0; y < h; ++y)
    for (uint32_t x = 0; x < w; ++x) {
      uint8_t v;
      switch (kind) {
        case 0: v = (uint8_t)((x * 3 + y * 5) / 7 + (rnd() % 5)); break;
        case 1: v = (uint8_t)rnd(); break;
        case 2: v = 77; break;
        case 3: v = (rnd() & 1) ? 10 : 200; break;
        default: {
          uint32_t r = rnd(), k = 0;
          while (k < 20 && (r & 1)) { r >>= 1; ++k; }
          v = (uint8_t)(k * 11);
        }
      }
      img[(size_t)y * w + x] = v;
    }
}

static int failures = 0;
#define FAIL(...)                      \
  do {                                 \
    fprintf(stderr, __VA_ARGS__);      \
    fputc('\n', stderr);               \
    ++failures;                        \
  } while (0)

static void check_bounds(const uint32_t *marks, uint64_t nb, const char *what) {
  for (uint64_t b = 0; b < nb; ++b)
    if ((marks[b] & 0xFFFFu) > 512u || (marks[b] >> 24) != 0u) {
      FAIL("%s: block %llu mark %08x out of bounds", what, (unsigned long long)b, marks[b]);
      return;
    }
}

static void one_case(uint32_t w, uint32_t h, int kind, uint32_t flags, int with_init) {
  const uint32_t bw = (w + 7) / 8, bh = (h + 7) / 8;
  const uint64_t nb = (uint64_t)bw * bh, n = nb * 64;
  const uint32_t enc_flags = flags | MH_ENCODE_LIMIT_LENGTHS;
  uint8_t *img = malloc((size_t)w * h);
  make_picture(img, w, h, kind);
  const uint64_t cap = mh_codes_bound(n) + 2;
  uint8_t *codes = malloc(cap), *codes0 = malloc(cap);
  uint32_t *offsets = malloc(nb * 4), *offsets0 = malloc(nb * 4);
  uint32_t *marks = malloc(nb * 4), *walked = malloc(nb * 4);
  uint8_t *init = with_init ? malloc(nb) : NULL, *init0 = with_init ? malloc(nb) : NULL;
  uint8_t *blocks = malloc(n);
  uint8_t canon[256], canon0[256];
  uint64_t len = 0, len0 = 0;
  mh_lookup_symbol t1[256];
  mh_lookup_symbol *t2 = malloc(sizeof(mh_lookup_symbol) * MH_TABLE2_MAX_ENTRIES);
  uint32_t t2e = 0;
  int rc = mh_encode_frame_marks(img, w, h, enc_flags, canon, codes, cap, &len, offsets, init, marks);
  const int rc0 = mh_encode_frame(img, w, h, enc_flags, canon0, codes0, cap, &len0, offsets0, init0);
  if (rc != MH_OK || rc0 != MH_OK) { FAIL("%ux%u kind %d: encode %d / %d", w, h, kind, rc, rc0); goto done; }
  if (len != len0 || memcmp(codes, codes0, len) || memcmp(offsets, offsets0, nb * 4) || memcmp(canon, canon0, 256) ||
      (with_init && memcmp(init, init0, nb)))
    FAIL("%ux%u kind %d flags %u init %d: the marks entry changed the frame's bytes", w, h, kind, flags, with_init);
  check_bounds(marks, nb, "encoder");
  /* the marks from the picture and the code lengths */
  if (mh_split_blocks(img, w, h, 8, 0, blocks, n) != MH_OK) { FAIL("split"); goto done; }
  for (uint64_t b = 0; b < nb; ++b) {
    const uint8_t *blk = blocks + b * 64;
    uint32_t bits = 0;
    for (int k = 0; k < 32; ++k) {
      uint8_t s = blk[k];
      if (!(flags & MH_FLAG_NO_DELTA)) s = (uint8_t)((k == 0 && with_init) ? 0 : blk[k] - (k ? blk[k - 1] : 0));
      bits += canon[s];
    }
    const uint32_t want = bits | ((flags & MH_FLAG_NO_DELTA) ? 0u : (uint32_t)blk[31] << 16);
    if (marks[b] != want) {
      FAIL("%ux%u kind %d flags %u init %d: block %llu mark %08x, computed %08x", w, h, kind, flags, with_init,
           (unsigned long long)b, marks[b], want);
      break;
    }
  }
  rc = mh_build_tables(canon, t1, t2, MH_TABLE2_MAX_ENTRIES, &t2e);
  if (rc != MH_OK) { FAIL("%ux%u kind %d: mh_build_tables %d", w, h, kind, rc); goto done; }
  rc = mh_mid_marks(codes, len, offsets, nb, t1, t2, t2e, init, flags, walked);
  if (rc != MH_OK || memcmp(walked, marks, nb * 4))
    FAIL("%ux%u kind %d flags %u init %d: the walk (rc %d) and the encoder disagree", w, h, kind, flags, with_init, rc);
  /* argument checks */
  if (mh_mid_marks(NULL, len, offsets, nb, t1, t2, t2e, init, flags, walked) != MH_ERR_INVALID_ARG ||
      mh_mid_marks(codes, len, offsets, 0, t1, t2, t2e, init, flags, walked) != MH_ERR_INVALID_ARG ||
      mh_mid_marks(codes, len, offsets, nb, t1, t2, t2e, init, flags | MH_FLAG_ANY_ORDER, walked) != MH_ERR_INVALID_ARG ||
      mh_mid_marks(codes, len, offsets, nb, t1, t2, 255, init, flags, walked) != MH_ERR_TABLE)
    FAIL("%ux%u: argument checks", w, h);
  /* garbage in: scrambled code bytes; offsets anywhere in the payload; offsets far past it; a
   * buffer declared shorter than the offsets reach; a truncated table2 */
  for (uint64_t i = 0; i + MH_CODES_PAD < len; ++i) codes[i] = (uint8_t)rnd();
  if (mh_mid_marks(codes, len, offsets, nb, t1, t2, t2e, init, flags, walked) == MH_OK) check_bounds(walked, nb, "noise");
  for (uint64_t b = 0; b < nb; ++b) offsets[b] = (uint32_t)(rnd() % (uint32_t)(len * 8));
  if (mh_mid_marks(codes, len, offsets, nb, t1, t2, t2e, init, flags, walked) == MH_OK) check_bounds(walked, nb, "offsets");
  for (uint64_t b = 0; b < nb; ++b) offsets[b] = 0xFFFFFFFFu - (uint32_t)b;
  if (mh_mid_marks(codes, len, offsets, nb, t1, t2, t2e, init, flags, walked) == MH_OK) check_bounds(walked, nb, "far");
  for (uint64_t b = 0; b < nb; ++b) offsets[b] = (uint32_t)(rnd() % (uint32_t)(len * 8));
  if (mh_mid_marks(codes, 1, offsets, nb, t1, t2, 256, init, flags, walked) == MH_OK) check_bounds(walked, nb, "short");
done:
  free(img);
  free(codes);
  free(codes0);
  free(offsets);
  free(offsets0);
  free(marks);
  free(walked);
  free(init);
  free(init0);
  free(blocks);
  free(t2);
}

int main(int argc, char **argv) {
  rng_state = argc > 1 ? strtoull(argv[1], NULL, 10) | 1u : 0x9E3779B97F4A7C15ull;
  static const uint32_t dims[][2] = {{1, 1}, {9, 9}, {8, 8}, {257, 17}, {64, 64}, {333, 117}, {1000, 8}, {3, 301}};
  int cases = 0;
  for (size_t d = 0; d < sizeof(dims) / sizeof(dims[0]); ++d)
    for (int kind = 0; kind < 5; ++kind) {
      one_case(dims[d][0], dims[d][1], kind, 0, 0);
      one_case(dims[d][0], dims[d][1], kind, MH_FLAG_NO_DELTA, 0);
      one_case(dims[d][0], dims[d][1], kind, 0, 1);
      cases += 3;
    }
  if (failures) {
    printf("selftest FAILED %d of %d\n", failures, cases);
    return 1;
  }
  printf("selftest ok %d\n", cases);
  return 0;
}
