/* mh_limit_selftest.c -- the length-limited code (mh_code_lengths_limited, mh_encode_frame
 * with MH_ENCODE_LIMIT_LENGTHS) through the host half of the C-ABI, meant to be built with
 * the host compiler's AddressSanitizer and UndefinedBehaviorSanitizer
 * (tests/test_limit_sanitize.py). No GPU and no HIP: it links mh_host.cpp and mh_cpu.cpp.
 *
 * Histograms: Fibonacci counts over 18..40 symbols dealt to random symbols, geometric tails
 * over all 256 symbols, heavy-tailed random counts, counts up to 2^40, and the 256-symbol
 * chain (239 symbols of count 1 and 17 whose counts follow a, b <- b, a + b from (239, 239)).
 * Each goes through mh_code_lengths_limited at 16, 13, 8 and ceil(log2 n) bits: every
 * present symbol has a length within the limit, no other has one, and the Kraft sum is
 * exactly 1; where mh_code_lengths fits the limit, the lengths are its own.
 * Frames: histograms that fit a frame become pictures in the delta, no-delta and init-byte
 * formats: mh_encode_frame without the flag says MH_ERR_CODE_TOO_LONG where the tree is too
 * deep, with it mh_encode_frame -> mh_build_tables -> mh_decode_frame_cpu == the picture.
 * Prints one line per failure and "limit selftest ok <cases>" at the end; exit status 0 iff ok. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../include/metalhuffman.h"

static uint64_t rng_state;
static uint64_t rnd64(void) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static uint32_t rnd(void) { return (uint32_t)(rnd64() >> 11); }

static int failures = 0, cases = 0, deep_cases = 0;
#define FAIL(...)                 \
  do {                            \
    fprintf(stderr, __VA_ARGS__); \
    fputc('\n', stderr);          \
    ++failures;                   \
  } while (0)

/* counts[0..n) onto n distinct random symbols, the first count on symbol 0 */
static void deal(const uint64_t *counts, uint32_t n, uint64_t freq[256]) {
  uint8_t perm[256];
  for (uint32_t i = 0; i < 256; ++i) perm[i] = (uint8_t)i;
  for (uint32_t i = 255; i > 1; --i) {  /* symbol 0 stays in place */
    const uint32_t j = 1 + rnd() % i;
    const uint8_t t = perm[i];
    perm[i] = perm[j];
    perm[j] = t;
  }
  memset(freq, 0, 256 * sizeof(uint64_t));
  for (uint32_t i = 0; i < n; ++i) freq[perm[i]] = counts[i];
}

static uint32_t ceil_log2(uint32_t n) {
  uint32_t b = 0;
  while ((1u << b) < n) ++b;
  return b ? b : 1;
}

static void check_lengths(const char *name, const uint64_t freq[256]) {
  uint32_t n = 0;
  for (int s = 0; s < 256; ++s) n += freq[s] != 0;
  uint8_t huff[256];
  const int hrc = mh_code_lengths(freq, huff);
  if (hrc == MH_ERR_CODE_TOO_LONG) ++deep_cases;
  const uint32_t limits[4] = {16, 13, 8, ceil_log2(n)};
  for (int k = 0; k < 4; ++k) {
    const uint32_t L = limits[k];
    uint8_t lens[256];
    memset(lens, 0xEE, sizeof lens);
    const int rc = mh_code_lengths_limited(freq, L, lens);
    ++cases;
    if ((1u << L) < n) {
      if (rc != MH_ERR_INVALID_ARG) FAIL("%s L=%u: %u symbols accepted (%d)", name, L, n, rc);
      continue;
    }
    if (rc != MH_OK) { FAIL("%s L=%u: status %d", name, L, rc); continue; }
    uint64_t kraft = 0;
    int fits = 1;
    for (int s = 0; s < 256; ++s) {
      if ((lens[s] != 0) != (freq[s] != 0) || lens[s] > L) { FAIL("%s L=%u: symbol %d length %u", name, L, s, lens[s]); break; }
      if (lens[s]) kraft += 1ull << (16 - lens[s]);
      if (huff[s] > L) fits = 0;
    }
    if (n >= 2 && kraft != 65536) FAIL("%s L=%u: Kraft sum %llu / 65536", name, L, (unsigned long long)kraft);
    if (fits && memcmp(lens, huff, 256) != 0) FAIL("%s L=%u: the tree fits but the lengths differ", name, L);
  }
}

/* a picture of w x h (multiples of 8) whose coded symbols have the histogram freq, the rest
 * of the frame filled with symbol 0, which also opens every block */
static uint8_t *picture(const uint64_t freq[256], uint32_t w, uint32_t h, int no_delta) {
  const uint32_t bw = w / 8, nb = bw * (h / 8);
  uint64_t total = 0;
  for (int s = 0; s < 256; ++s) total += freq[s];
  if (total > (uint64_t)nb * 64 || freq[0] + (uint64_t)nb * 64 - total < nb) return NULL;
  uint8_t *sym = malloc((size_t)nb * 64);
  size_t k = 0;
  for (int s = 1; s < 256; ++s)
    for (uint64_t c = 0; c < freq[s]; ++c) sym[k++] = (uint8_t)s;
  memset(sym + k, 0, (size_t)nb * 64 - k);
  for (size_t i = (size_t)nb * 64 - 1; i > 0; --i) {  /* shuffle, then open every block with 0 */
    const size_t j = rnd64() % (i + 1);
    const uint8_t t = sym[i];
    sym[i] = sym[j];
    sym[j] = t;
  }
  for (uint32_t b = 0, z = 0; b < nb; ++b) {
    if (sym[(size_t)b * 64] == 0) continue;
    while (z < nb * 64 && (sym[z] != 0 || z % 64 == 0)) ++z;  /* a zero that opens no block */
    if (z == nb * 64) break;                                   /* cannot happen: at least nb zeros */
    sym[z] = sym[(size_t)b * 64];
    sym[(size_t)b * 64] = 0;
  }
  uint8_t *img = malloc((size_t)w * h);
  for (uint32_t b = 0; b < nb; ++b) {
    uint8_t acc = 0;
    for (uint32_t i = 0; i < 64; ++i) {
      const uint8_t v = sym[(size_t)b * 64 + i];
      acc = no_delta ? v : (uint8_t)(acc + v);
      img[(size_t)((b / bw) * 8 + i / 8) * w + (b % bw) * 8 + i % 8] = acc;
    }
  }
  free(sym);
  return img;
}

static void check_frame(const char *name, const uint64_t freq[256], uint32_t w, uint32_t h) {
  for (int fmt = 0; fmt < 3; ++fmt) {  /* delta, no-delta, init byte */
    const uint32_t flags = fmt == 1 ? MH_FLAG_NO_DELTA : 0;
    uint8_t *img = picture(freq, w, h, fmt == 1);
    if (!img) { FAIL("%s: no %ux%u picture", name, w, h); return; }
    const uint64_t nb = (uint64_t)(w / 8) * (h / 8), cap = mh_codes_bound(nb * 64) + 2;
    uint8_t *codes = malloc(cap), *init = fmt == 2 ? malloc(nb) : NULL, *out = malloc((size_t)w * h);
    uint32_t *offsets = malloc(nb * 4);
    mh_lookup_symbol t1[256];
    mh_lookup_symbol *t2 = malloc(sizeof(mh_lookup_symbol) * MH_TABLE2_MAX_ENTRIES);
    uint8_t canon[256], huff[256];
    uint64_t len = 0;
    uint32_t t2e = 0;
    ++cases;
    uint64_t coded[256], total = 0;  /* the frame's histogram: the rest of the frame is symbol 0 */
    for (int s = 0; s < 256; ++s) total += (coded[s] = freq[s]);
    coded[0] += nb * 64 - total;
    const int deep = mh_code_lengths(coded, huff) == MH_ERR_CODE_TOO_LONG;
    int rc = mh_encode_frame(img, w, h, flags, canon, codes, cap, &len, offsets, init);
    if (rc != (deep ? MH_ERR_CODE_TOO_LONG : MH_OK)) FAIL("%s fmt %d: unflagged status %d", name, fmt, rc);
    rc = mh_encode_frame(img, w, h, flags | MH_ENCODE_LIMIT_LENGTHS, canon, codes, cap, &len, offsets, init);
    if (rc != MH_OK) { FAIL("%s fmt %d: mh_encode_frame %d", name, fmt, rc); goto done; }
    for (int s = 0; s < 256; ++s)
      if (canon[s] > 16) { FAIL("%s fmt %d: length %u", name, fmt, canon[s]); goto done; }
    rc = mh_build_tables(canon, t1, t2, MH_TABLE2_MAX_ENTRIES, &t2e);
    if (rc != MH_OK) { FAIL("%s fmt %d: mh_build_tables %d", name, fmt, rc); goto done; }
    for (uint32_t threads = 1; threads <= 3; threads += 2) {
      memset(out, 0xEE, (size_t)w * h);
      rc = mh_decode_frame_cpu(offsets, codes, len, t1, t2, t2e, init, w, h, flags, out, w, threads);
      if (rc != MH_OK || memcmp(out, img, (size_t)w * h) != 0)
        FAIL("%s fmt %d: decode on %u threads differs (%d)", name, fmt, threads, rc);
    }
  done:
    free(t2);
    free(offsets);
    free(out);
    free(init);
    free(codes);
    free(img);
  }
}

int main(int argc, char **argv) {
  rng_state = argc > 1 ? strtoull(argv[1], NULL, 10) * 0x9E3779B97F4A7C15ull + 1 : 88172645463325252ull;
  uint64_t counts[256], freq[256];
  char name[64];
  for (uint32_t n = 18; n <= 40; ++n) {  /* Fibonacci counts, the largest first */
    const uint64_t scale = 1 + rnd() % 40;
    uint64_t a = 1, b = 1;
    for (uint32_t i = 0; i < n; ++i) {
      counts[n - 1 - i] = a * scale;
      const uint64_t c = a + b;
      a = b;
      b = c;
    }
    deal(counts, n, freq);
    snprintf(name, sizeof name, "fib%u", n);
    check_lengths(name, freq);
    if (n <= 22) {
      for (uint32_t i = 0; i < n; ++i) counts[i] /= scale;
      deal(counts, n, freq);
      check_frame(name, freq, n == 18 ? 128 : 256, n == 18 ? 64 : 256);
    }
  }
  for (int k = 0; k < 30; ++k) {  /* geometric tails over all 256 symbols */
    const double ratio = 0.55 + 0.42 * (rnd() % 1000) / 1000.0;
    double top = (double)(1ull << (20 + rnd() % 25));
    for (int i = 0; i < 256; ++i) {
      counts[i] = (uint64_t)top + 1 + rnd() % 3;
      top *= ratio;
    }
    deal(counts, 256, freq);
    snprintf(name, sizeof name, "geo%d", k);
    check_lengths(name, freq);
  }
  for (int k = 0; k < 40; ++k) {  /* heavy tails: 2^(a random exponent, squared bias) */
    const uint32_t n = 2 + rnd() % 255;
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t e = (rnd() % 41) * (rnd() % 41) / 40;
      counts[i] = (1ull << e) + rnd64() % (1ull << e);
    }
    deal(counts, n, freq);
    snprintf(name, sizeof name, "heavy%d", k);
    check_lengths(name, freq);
  }
  for (int k = 0; k < 30; ++k) {  /* counts up to 2^40 */
    const uint32_t n = 2 + rnd() % 255;
    for (uint32_t i = 0; i < n; ++i) counts[i] = 1 + rnd64() % (1ull << (1 + rnd() % 40));
    deal(counts, n, freq);
    snprintf(name, sizeof name, "wide%d", k);
    check_lengths(name, freq);
  }
  {  /* the 256-symbol chain: level lists of 511 items */
    uint64_t a = 239, b = 239;
    for (int i = 0; i < 256; ++i) freq[i] = 1;
    for (int i = 16; i >= 0; --i) {
      freq[i] = a;
      const uint64_t c = a + b;
      a = b;
      b = c;
    }
    check_lengths("chain", freq);
    check_frame("chain", freq, 1024, 1024);
  }
  {  /* argument checks */
    uint8_t lens[256];
    memset(freq, 0, sizeof freq);
    if (mh_code_lengths_limited(freq, 16, lens) != MH_ERR_EMPTY) FAIL("empty histogram");
    freq[9] = 3;
    if (mh_code_lengths_limited(freq, 1, lens) != MH_OK || lens[9] != 1) FAIL("one symbol");
    freq[10] = 1ull << 59;
    if (mh_code_lengths_limited(freq, 16, lens) != MH_ERR_INVALID_ARG) FAIL("total of 2^59 accepted");
    freq[10] = ~0ull;
    freq[11] = ~0ull;
    if (mh_code_lengths_limited(freq, 16, lens) != MH_ERR_INVALID_ARG) FAIL("wrapping total accepted");
    freq[10] = freq[11] = 1;
    if (mh_code_lengths_limited(freq, 0, lens) != MH_ERR_INVALID_ARG ||
        mh_code_lengths_limited(freq, 17, lens) != MH_ERR_INVALID_ARG ||
        mh_code_lengths_limited(freq, 1, lens) != MH_ERR_INVALID_ARG ||
        mh_code_lengths_limited(NULL, 16, lens) != MH_ERR_INVALID_ARG ||
        mh_code_lengths_limited(freq, 16, NULL) != MH_ERR_INVALID_ARG)
      FAIL("argument checks");
    if (mh_code_lengths_limited(freq, 2, lens) != MH_OK) FAIL("three symbols in two bits");
  }
  if (deep_cases < 50) FAIL("only %d histograms deeper than 16", deep_cases);
  if (failures) {
    fprintf(stderr, "%d failure(s)\n", failures);
    return 1;
  }
  printf("limit selftest ok %d (%d deeper than 16)\n", cases, deep_cases);
  return 0;
}
