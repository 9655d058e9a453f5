// mh_host.cpp -- host-side producer of the MI355X Huffman block codec.
//
// Clean-room C++ re-derivation of the reference's CPU codec so that the frames
// the GPU decoder consumes are byte-identical to what mdejong/MetalHuffman's
// encoder emits:
//   * block split            Shared/Util.m:233-323
//   * per-block byte deltas  Shared/HuffmanUtil.cpp:21-85, :1133-1145
//   * Huffman code lengths   Shared/HuffmanEncoder.cpp:29-145 (node-array tie-breaking)
//   * canonical codes        Shared/huff_util.hpp:94-193
//   * MSB-first bit packing  Shared/HuffmanEncoder.cpp:211-381
//   * block bit offsets      Shared/HuffmanUtil.cpp:1103-1128
//   * split T1/T2 tables     Shared/HuffmanUtil.cpp:338-667
// No module statics (the reference keeps code tables in file statics,
// HuffmanUtil.cpp:87-102): every entry point is reentrant.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/metalhuffman.h"
#include "mh_set_plan.hpp"

namespace {

// Code lengths from symbol frequencies, reproducing the reference's tree
// shape exactly. The reference (HuffmanEncoder.cpp:81-102) keeps nodes in an
// array sorted by weight where a new node goes after every node whose weight
// is <= its own -- i.e. at std::upper_bound -- and build_tree (:69-79) merges
// the two front-most unconsumed entries. Leaves enter in symbol order.
int code_lengths(const uint64_t freq[256], uint8_t lens[256]) {
  std::memset(lens, 0, 256);
  struct Node { uint64_t w; int left, right; };
  std::vector<Node> nodes;
  nodes.reserve(512);
  std::vector<int> queue;  // node ids sorted by weight (stable)
  queue.reserve(512);
  auto push = [&](int id) {
    auto it = std::upper_bound(queue.begin(), queue.end(), nodes[id].w,
                               [&](uint64_t w, int other) { return w < nodes[other].w; });
    queue.insert(it, id);
  };
  int leaf_symbol[256];
  int nleaf = 0;
  for (int s = 0; s < 256; ++s) {
    if (!freq[s]) continue;
    leaf_symbol[nleaf++] = s;
    nodes.push_back({freq[s], -1, -1});
    push((int)nodes.size() - 1);
  }
  if (nleaf == 0) return MH_ERR_EMPTY;
  if (nleaf == 1) {  // single symbol -> 1-bit code "0" (HuffmanEncoder.cpp:118-121)
    lens[leaf_symbol[0]] = 1;
    return MH_OK;
  }
  size_t head = 0;
  while (head + 1 < queue.size()) {
    const int a = queue[head], b = queue[head + 1];
    head += 2;
    nodes.push_back({nodes[a].w + nodes[b].w, a, b});
    push((int)nodes.size() - 1);
  }
  // Depths top-down: internal nodes were created in order, the root last.
  std::vector<int> depth(nodes.size(), 0);
  for (int id = (int)nodes.size() - 1; id >= nleaf; --id) {
    depth[nodes[id].left] = depth[id] + 1;
    depth[nodes[id].right] = depth[id] + 1;
  }
  bool too_long = false;
  for (int i = 0; i < nleaf; ++i) {
    if (depth[i] > 16) too_long = true;
    lens[leaf_symbol[i]] = (uint8_t)std::min(depth[i], 255);
  }
  return too_long ? MH_ERR_CODE_TOO_LONG : MH_OK;
}

// Optimal code lengths of at most L bits (package-merge, the form that keeps only
// counts; DESIGN.md "Length-limited codes" states the rule). Leaves are the n >= 2
// present symbols sorted by (count, symbol); list_1 is the leaves; list_l is the merge
// of the leaves with the pairs of list_{l-1} (a trailing odd item dropped), the leaf
// first on equal weight. Backwards from t = 2n - 2 items of list_L, a_l is the number
// of leaves among the first t items of list_l and t becomes 2 (t - a_l); the leaf of
// rank r gets length #{l : a_l > r}. Weights are exact: a package is below L x the
// total, and the caller bounds the total by 2^59. Needs 2^L >= n.
void limited_lengths(const uint64_t freq[256], uint32_t L, uint8_t lens[256]) {
  std::memset(lens, 0, 256);
  int leaf_symbol[256];
  uint64_t lw[256];
  uint32_t n = 0;
  for (int s = 0; s < 256; ++s)
    if (freq[s]) leaf_symbol[n++] = s;
  std::stable_sort(leaf_symbol, leaf_symbol + n, [&](int a, int b) { return freq[a] < freq[b]; });
  for (uint32_t i = 0; i < n; ++i) lw[i] = freq[leaf_symbol[i]];
  // per level: which items of the merged list are leaves (a list has < 2n items)
  std::vector<uint8_t> is_leaf((size_t)(L + 1) * 512, 0);
  uint64_t list[2][512];
  uint32_t m = n, cur = 0;
  for (uint32_t i = 0; i < n; ++i) {
    list[0][i] = lw[i];
    is_leaf[512 + i] = 1;
  }
  for (uint32_t l = 2; l <= L; ++l) {
    const uint64_t *prev = list[cur];
    uint64_t *next = list[cur ^ 1];
    const uint32_t np = m / 2;
    uint32_t i = 0, j = 0, k = 0;
    while (i < n || j < np) {
      const uint64_t p = j < np ? prev[2 * j] + prev[2 * j + 1] : 0;
      if (i < n && (j >= np || lw[i] <= p)) {
        is_leaf[(size_t)l * 512 + k] = 1;
        next[k++] = lw[i++];
      } else {
        next[k++] = p;
        ++j;
      }
    }
    m = k;
    cur ^= 1;
  }
  uint32_t t = 2 * n - 2;
  for (uint32_t l = L; l >= 1; --l) {
    uint32_t a = 0;
    for (uint32_t k = 0; k < t; ++k) a += is_leaf[(size_t)l * 512 + k];
    for (uint32_t r = 0; r < a; ++r) ++lens[leaf_symbol[r]];
    t = 2 * (t - a);
  }
}

// huff_util.hpp:94-193: canonical order = (length, symbol); codes count up
// and are shifted left whenever the length grows; stored left-justified.
void canonical_codes(const uint8_t lens[256], uint16_t codes[256]) {
  std::memset(codes, 0, 256 * sizeof(uint16_t));
  int order[256];
  int n = 0;
  for (int s = 0; s < 256; ++s)
    if (lens[s]) order[n++] = s;
  std::stable_sort(order, order + n, [&](int a, int b) { return lens[a] < lens[b]; });
  uint32_t code = 0;
  for (int i = 0; i < n; ++i) {
    const int len = lens[order[i]];
    if (i > 0 && len > lens[order[i - 1]]) code <<= (len - lens[order[i - 1]]);
    codes[order[i]] = (uint16_t)(code << (16 - len));
    ++code;
  }
}

// MSB-first bit writer into a caller buffer.
struct BitWriter {
  uint8_t *out;
  uint64_t acc = 0;  // pending bits, right-aligned
  int nacc = 0;
  uint64_t nbytes = 0;
  uint64_t nbits = 0;
  explicit BitWriter(uint8_t *o) : out(o) {}
  inline void put(uint32_t code_lj16, int len) {
    acc = (acc << len) | (code_lj16 >> (16 - len));
    nacc += len;
    nbits += len;
    while (nacc >= 8) {
      nacc -= 8;
      out[nbytes++] = (uint8_t)(acc >> nacc);
    }
  }
  inline void flush() {  // zero-fill the last partial byte (HuffmanEncoder.cpp:279-306)
    if (nacc > 0) {
      out[nbytes++] = (uint8_t)(acc << (8 - nacc));
      nacc = 0;
    }
  }
};

int encode_symbols(const uint8_t *sym, uint64_t n, uint64_t stride, uint8_t canon[256],
                   uint8_t *codes, uint64_t codes_cap, uint64_t *codes_len, uint32_t *offsets,
                   bool limit = false, uint32_t *mid_bits = nullptr) {
  uint64_t freq[256] = {0};
  for (uint64_t i = 0; i < n; ++i) freq[sym[i]]++;
  int rc = code_lengths(freq, canon);
  // MH_ENCODE_LIMIT_LENGTHS: only a tree deeper than 16 is replaced (n < 2^59 symbols)
  if (rc == MH_ERR_CODE_TOO_LONG && limit && n < (1ull << 59)) {
    limited_lengths(freq, 16, canon);
    rc = MH_OK;
  }
  if (rc != MH_OK) return rc;
  uint16_t cc[256];
  canonical_codes(canon, cc);
  uint64_t total_bits = 0;
  for (int s = 0; s < 256; ++s) total_bits += freq[s] * canon[s];
  if (total_bits >= (1ull << 32)) return MH_ERR_CAPACITY;  // u32 block offsets
  const uint64_t need = (total_bits + 7) / 8 + 2;
  if (need > codes_cap) return MH_ERR_CAPACITY;
  BitWriter bw(codes);
  for (uint64_t i = 0; i < n; ++i) {
    if (offsets && (i % stride) == 0) offsets[i / stride] = (uint32_t)bw.nbits;
    // the packer passes a block's middle as it writes: code bits from the block's offset to the
    // symbol half a stride in (mh_encode_frame_marks; a block's first half is <= 32 x 16 bits)
    if (mid_bits && (i % stride) == stride / 2) mid_bits[i / stride] = (uint32_t)bw.nbits - offsets[i / stride];
    const uint8_t s = sym[i];
    bw.put(cc[s], canon[s]);
  }
  bw.flush();
  codes[bw.nbytes++] = 0;  // decoder read-ahead (HuffmanEncoder.cpp:371-378)
  codes[bw.nbytes++] = 0;
  *codes_len = bw.nbytes;
  return MH_OK;
}

void fill_range(mh_lookup_symbol *tab, uint32_t first, uint32_t count, uint8_t sym, uint8_t len) {
  for (uint32_t i = 0; i < count; ++i) tab[first + i] = mh_lookup_symbol{sym, len};
}

// binary32 bits -> binary16 / bfloat16 bits, round to nearest even (mh_norm_table). The input is
// finite or an infinity (a fused multiply-add of finite operands yields no NaN).
uint16_t f32_to_f16(uint32_t x) {
  const uint32_t sign = (x >> 16) & 0x8000u, mag = x & 0x7FFFFFFFu;
  if (mag >= 0x477FF000u) return (uint16_t)(sign | 0x7C00u);  // >= 65520 rounds to inf
  uint32_t q, rem, half;
  if (mag < 0x38800000u) {  // below 2^-14: a subnormal, in units of 2^-24
    const uint32_t e = mag >> 23, shift = 126u - e;
    if (e == 0u || shift > 24u) return (uint16_t)sign;  // below 2^-25: zero
    const uint32_t mant = (mag & 0x7FFFFFu) | 0x800000u;
    q = mant >> shift;
    rem = mant & ((1u << shift) - 1u);
    half = 1u << (shift - 1u);
  } else {
    const uint32_t v = mag - 0x38000000u;  // exponent rebiased from 127 to 15
    q = v >> 13;
    rem = v & 0x1FFFu;
    half = 0x1000u;
  }
  if (rem > half || (rem == half && (q & 1u))) ++q;  // a carry moves into the exponent, as it must
  return (uint16_t)(sign | q);
}

uint16_t f32_to_bf16(uint32_t x) { return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16); }

}  // namespace

extern "C" {

int mh_split_blocks(const uint8_t *img, uint32_t width, uint32_t height, uint32_t block_dim,
                    uint8_t zero_value, uint8_t *out, size_t out_bytes) {
  if (!img || !out || !width || !height || !block_dim) return MH_ERR_INVALID_ARG;
  const uint32_t bw = (width + block_dim - 1) / block_dim;
  const uint32_t bh = (height + block_dim - 1) / block_dim;
  const size_t bsz = (size_t)block_dim * block_dim;
  if (out_bytes < bsz * bw * bh) return MH_ERR_CAPACITY;
  std::memset(out, zero_value, bsz * bw * bh);
  for (uint32_t by = 0; by < bh; ++by) {
    for (uint32_t bx = 0; bx < bw; ++bx) {
      uint8_t *blk = out + ((size_t)by * bw + bx) * bsz;
      const uint32_t x0 = bx * block_dim;
      const uint32_t cols = std::min(block_dim, width - x0);
      for (uint32_t r = 0; r < block_dim; ++r) {
        const uint32_t y = by * block_dim + r;
        if (y >= height) break;
        std::memcpy(blk + (size_t)r * block_dim, img + (size_t)y * width + x0, cols);
      }
    }
  }
  return MH_OK;
}

int mh_merge_blocks(const uint8_t *blocks, uint32_t width, uint32_t height, uint32_t block_dim,
                    uint8_t *out, size_t out_pitch) {
  if (!blocks || !out || !width || !height || !block_dim || out_pitch < width)
    return MH_ERR_INVALID_ARG;
  const uint32_t bw = (width + block_dim - 1) / block_dim;
  const size_t bsz = (size_t)block_dim * block_dim;
  for (uint32_t y = 0; y < height; ++y) {
    const uint32_t by = y / block_dim, r = y % block_dim;
    for (uint32_t bx = 0; bx < bw; ++bx) {
      const uint32_t x0 = bx * block_dim;
      const uint32_t cols = std::min(block_dim, width - x0);
      std::memcpy(out + (size_t)y * out_pitch + x0,
                  blocks + ((size_t)by * bw + bx) * bsz + (size_t)r * block_dim, cols);
    }
  }
  return MH_OK;
}

int mh_encode_signed_byte_deltas(const uint8_t *in, uint8_t *out, size_t n) {
  if ((!in || !out) && n) return MH_ERR_INVALID_ARG;
  uint8_t prev = 0;
  for (size_t i = 0; i < n; ++i) {
    const uint8_t v = in[i];
    out[i] = (uint8_t)(v - prev);
    prev = v;
  }
  return MH_OK;
}

int mh_decode_signed_byte_deltas(const uint8_t *in, uint8_t *out, size_t n) {
  if ((!in || !out) && n) return MH_ERR_INVALID_ARG;
  uint8_t acc = 0;
  for (size_t i = 0; i < n; ++i) {
    acc = (uint8_t)(acc + in[i]);
    out[i] = acc;
  }
  return MH_OK;
}

uint64_t mh_codes_bound(uint64_t n_symbols) { return n_symbols * 2 + 2; }

int mh_encode_huffman(const uint8_t *symbols, uint64_t n_symbols, uint32_t block_dim,
                      uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                      uint64_t *codes_len, uint32_t *block_bit_offsets) {
  if (!symbols || !canon_header || !codes || !codes_len || !block_dim) return MH_ERR_INVALID_ARG;
  if (n_symbols == 0) return MH_ERR_EMPTY;
  const uint64_t stride = (uint64_t)block_dim * block_dim;
  // HuffmanUtil.cpp:1110-1115 queries offsets only for whole blocks.
  return encode_symbols(symbols, n_symbols, stride, canon_header, codes, codes_cap, codes_len,
                        block_bit_offsets);
}

int mh_encode_frame_marks(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                          uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                          uint64_t *codes_len, uint32_t *block_offsets, uint8_t *block_init,
                          uint32_t *mid_marks) {
  if (!gray || !canon_header || !codes || !codes_len || !block_offsets) return MH_ERR_INVALID_ARG;
  if (!width || !height || width > MH_MAX_DIM || height > MH_MAX_DIM) return MH_ERR_DIMS;
  const uint32_t bw = (width + 7) / 8, bh = (height + 7) / 8;
  const uint64_t nb = (uint64_t)bw * bh;
  std::vector<uint8_t> blocks(nb * 64);
  int rc = mh_split_blocks(gray, width, height, 8, 0, blocks.data(), blocks.size());
  if (rc != MH_OK) return rc;
  if (!(flags & MH_FLAG_NO_DELTA)) {
    for (uint64_t b = 0; b < nb; ++b) {
      uint8_t *blk = blocks.data() + b * 64;
      // the decoder's running sum when it begins symbol 32 is pixel 31 (block_init or not: the
      // first delta is in the sum either way); read before the deltas replace the pixels
      if (mid_marks) mid_marks[b] = (uint32_t)blk[31] << 16;
      mh_encode_signed_byte_deltas(blk, blk, 64);
      if (block_init) {  // AAPLRenderer.m:456-472
        block_init[b] = blk[0];
        blk[0] = 0;
      }
    }
  } else {
    if (block_init) std::memset(block_init, 0, nb);  // AAPLRenderer.m:517-523
    if (mid_marks) std::memset(mid_marks, 0, nb * sizeof(uint32_t));
  }
  if (codes_cap < 2) return MH_ERR_CAPACITY;
  std::vector<uint32_t> mid_bits(mid_marks ? nb : 0);
  rc = encode_symbols(blocks.data(), blocks.size(), 64, canon_header, codes, codes_cap - 2,
                      codes_len, block_offsets, (flags & MH_ENCODE_LIMIT_LENGTHS) != 0,
                      mid_marks ? mid_bits.data() : nullptr);
  if (rc != MH_OK) return rc;
  if (mid_marks)
    for (uint64_t b = 0; b < nb; ++b) mid_marks[b] |= mid_bits[b];
  codes[*codes_len] = 0;  // renderer read-ahead (AAPLRenderer.m:576-585)
  codes[*codes_len + 1] = 0;
  *codes_len += 2;
  return MH_OK;
}

int mh_encode_frame(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                    uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                    uint64_t *codes_len, uint32_t *block_offsets, uint8_t *block_init) {
  return mh_encode_frame_marks(gray, width, height, flags, canon_header, codes, codes_cap, codes_len,
                               block_offsets, block_init, nullptr);
}

int mh_mid_marks(const uint8_t *codes, uint64_t codes_bytes, const uint32_t *block_offsets,
                 uint64_t n_blocks, const mh_lookup_symbol *table1, const mh_lookup_symbol *table2,
                 uint32_t table2_entries, const uint8_t *block_init, uint32_t flags, uint32_t *mid_marks) {
  if (!codes || !block_offsets || !table1 || !table2 || !mid_marks || n_blocks == 0) return MH_ERR_INVALID_ARG;
  if (flags & ~MH_FLAG_NO_DELTA) return MH_ERR_INVALID_ARG;
  if (table2_entries < 256 || (table2_entries % 256) != 0 || table2_entries > MH_TABLE2_MAX_ENTRIES)
    return MH_ERR_TABLE;
  const bool delta = !(flags & MH_FLAG_NO_DELTA);
  const auto byte_at = [&](uint64_t i) -> uint32_t { return i < codes_bytes ? codes[i] : 0u; };
  for (uint64_t b = 0; b < n_blocks; ++b) {
    uint64_t bit = block_offsets[b];
    uint32_t prev = delta && block_init ? block_init[b] : 0u;
    for (int k = 0; k < 32; ++k) {
      const uint64_t by = bit >> 3;
      const uint32_t w24 = (byte_at(by) << 16) | (byte_at(by + 1) << 8) | byte_at(by + 2);
      const uint32_t pat = (w24 >> (8u - (uint32_t)(bit & 7u))) & 0xFFFFu;
      mh_lookup_symbol e = table1[pat >> 8];
      if (e.bitWidth == 0) {  // an escape; one past table2 is the all-zero entry, as in the kernels
        const uint32_t idx = (uint32_t)e.symbol * 256u + (pat & 0xFFu);
        e = idx < table2_entries ? table2[idx] : mh_lookup_symbol{0, 0};
      }
      if (e.bitWidth == 0) continue;  // a zero-width lookup repeats prev and does not advance
      bit += e.bitWidth > 16 ? 16 : e.bitWidth;
      prev = (prev + e.symbol) & 0xFFu;
    }
    mid_marks[b] = (uint32_t)(bit - block_offsets[b]) | ((delta ? prev : 0u) << 16);
  }
  return MH_OK;
}

// The symbols mh_encode_frame encodes for one frame: zero-padded 8x8 blocks, per-block
// deltas unless MH_FLAG_NO_DELTA, the first delta moved into init[b] and zeroed when the
// format has init bytes (init: nb bytes or NULL; all zero under MH_FLAG_NO_DELTA).
static int frame_symbols(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                         std::vector<uint8_t> &blocks, uint8_t *init) {
  const uint64_t nb = (uint64_t)((width + 7) / 8) * ((height + 7) / 8);
  blocks.resize(nb * 64);
  const int rc = mh_split_blocks(gray, width, height, 8, 0, blocks.data(), blocks.size());
  if (rc != MH_OK) return rc;
  if (!(flags & MH_FLAG_NO_DELTA)) {
    for (uint64_t b = 0; b < nb; ++b) {
      uint8_t *blk = blocks.data() + b * 64;
      mh_encode_signed_byte_deltas(blk, blk, 64);
      if (init) {
        init[b] = blk[0];
        blk[0] = 0;
      }
    }
  } else if (init) {
    std::memset(init, 0, nb);
  }
  return MH_OK;
}

int mh_frame_histogram(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                       int with_block_init, uint64_t freq[256]) {
  if (!gray || !freq) return MH_ERR_INVALID_ARG;
  if (flags & ~(MH_FLAG_NO_DELTA | MH_ENCODE_LIMIT_LENGTHS)) return MH_ERR_INVALID_ARG;
  if (!width || !height || width > MH_MAX_DIM || height > MH_MAX_DIM) return MH_ERR_DIMS;
  std::vector<uint8_t> blocks, init;
  if (with_block_init) init.resize((size_t)((width + 7) / 8) * ((height + 7) / 8));
  const int rc = frame_symbols(gray, width, height, flags, blocks, with_block_init ? init.data() : nullptr);
  if (rc != MH_OK) return rc;
  for (const uint8_t s : blocks) freq[s]++;
  return MH_OK;
}

int mh_encode_frame_with_header(const uint8_t *gray, uint32_t width, uint32_t height, uint32_t flags,
                                const uint8_t canon_header[256], uint8_t *codes, uint64_t codes_cap,
                                uint64_t *codes_len, uint32_t *block_offsets, uint8_t *block_init) {
  if (!gray || !canon_header || !codes || !codes_len || !block_offsets) return MH_ERR_INVALID_ARG;
  if (flags & ~(MH_FLAG_NO_DELTA | MH_ENCODE_LIMIT_LENGTHS)) return MH_ERR_INVALID_ARG;
  if (!width || !height || width > MH_MAX_DIM || height > MH_MAX_DIM) return MH_ERR_DIMS;
  // the header's verdict: a length over 16, then a Kraft sum over 1 (in units of 2^-16)
  uint64_t kraft = 0;
  for (int s = 0; s < 256; ++s) {
    if (canon_header[s] > 16) return MH_ERR_CODE_TOO_LONG;
    if (canon_header[s]) kraft += 1ull << (16 - canon_header[s]);
  }
  if (kraft > (1ull << 16)) return MH_ERR_TABLE;
  const uint64_t nb = (uint64_t)((width + 7) / 8) * ((height + 7) / 8);
  std::vector<uint8_t> blocks, init(block_init ? nb : 0);
  const int rc = frame_symbols(gray, width, height, flags, blocks, block_init ? init.data() : nullptr);
  if (rc != MH_OK) return rc;
  uint64_t freq[256] = {0};
  for (const uint8_t s : blocks) freq[s]++;
  uint64_t total_bits = 0;
  for (int s = 0; s < 256; ++s) {
    if (freq[s] && !canon_header[s]) return MH_ERR_TABLE;  // a symbol the header has no code for
    total_bits += freq[s] * canon_header[s];
  }
  if (total_bits >= (1ull << 32)) return MH_ERR_CAPACITY;  // u32 block offsets
  const uint64_t len = (total_bits + 7) / 8 + MH_CODES_PAD;
  if (len > codes_cap) return MH_ERR_CAPACITY;
  uint16_t cc[256];
  canonical_codes(canon_header, cc);
  BitWriter bw(codes);
  for (uint64_t i = 0; i < blocks.size(); ++i) {
    if (i % 64 == 0) block_offsets[i / 64] = (uint32_t)bw.nbits;
    bw.put(cc[blocks[i]], canon_header[blocks[i]]);
  }
  bw.flush();
  for (int k = 0; k < MH_CODES_PAD; ++k) codes[bw.nbytes++] = 0;
  *codes_len = bw.nbytes;
  if (block_init) std::memcpy(block_init, init.data(), nb);
  return MH_OK;
}

int mh_container_header(uint64_t n_symbols, uint8_t header[MH_CONTAINER_HEADER_BYTES]) {
  if (!header) return MH_ERR_INVALID_ARG;
  if (n_symbols > 0xFFFFFFFFull) return MH_ERR_CAPACITY;
  const uint32_t words[2] = {MH_CONTAINER_MAGIC, (uint32_t)n_symbols};
  for (int w = 0; w < 2; ++w)
    for (int k = 0; k < 4; ++k) header[4 * w + k] = (uint8_t)(words[w] >> (8 * k));
  return MH_OK;
}

int mh_parse_container_header(const uint8_t header[MH_CONTAINER_HEADER_BYTES], uint64_t *n_symbols) {
  if (!header || !n_symbols) return MH_ERR_INVALID_ARG;
  uint32_t words[2] = {0, 0};
  for (int w = 0; w < 2; ++w)
    for (int k = 0; k < 4; ++k) words[w] |= (uint32_t)header[4 * w + k] << (8 * k);
  if (words[0] != MH_CONTAINER_MAGIC) return MH_ERR_INVALID_ARG;
  *n_symbols = words[1];
  return MH_OK;
}

int mh_code_lengths(const uint64_t freq[256], uint8_t canon_header[256]) {
  if (!freq || !canon_header) return MH_ERR_INVALID_ARG;
  return code_lengths(freq, canon_header);
}

int mh_code_lengths_limited(const uint64_t freq[256], uint32_t max_bits, uint8_t canon_header[256]) {
  if (!freq || !canon_header || max_bits < 1 || max_bits > 16) return MH_ERR_INVALID_ARG;
  uint64_t total = 0;
  uint32_t n = 0;
  for (int s = 0; s < 256; ++s) {
    if (freq[s] >= (1ull << 59)) return MH_ERR_INVALID_ARG;
    total += freq[s];  // below 2^60: no wrap
    if (total >= (1ull << 59)) return MH_ERR_INVALID_ARG;
    n += freq[s] != 0;
  }
  if (n > (1u << max_bits)) return MH_ERR_INVALID_ARG;
  const int rc = code_lengths(freq, canon_header);
  if (rc == MH_ERR_EMPTY || n == 1) return rc;
  for (int s = 0; s < 256; ++s)
    if (canon_header[s] > max_bits) {
      limited_lengths(freq, max_bits, canon_header);
      break;
    }
  return MH_OK;
}

int mh_canonical_codes(const uint8_t canon_header[256], uint16_t codes[256]) {
  if (!canon_header || !codes) return MH_ERR_INVALID_ARG;
  for (int s = 0; s < 256; ++s)
    if (canon_header[s] > 16) return MH_ERR_CODE_TOO_LONG;
  canonical_codes(canon_header, codes);
  return MH_OK;
}

int mh_build_tables(const uint8_t canon_header[256], mh_lookup_symbol table1[256],
                    mh_lookup_symbol *table2, uint32_t table2_cap, uint32_t *table2_entries) {
  if (!canon_header || !table1 || !table2 || !table2_entries) return MH_ERR_INVALID_ARG;
  uint16_t cc[256];
  int rc = mh_canonical_codes(canon_header, cc);
  if (rc != MH_OK) return rc;
  std::memset(table1, 0, 256 * sizeof(mh_lookup_symbol));
  // Long codes grouped by their high byte; groups numbered in ascending
  // high-byte order starting at 1 (subtable 0 is the all-zero dummy the
  // shader may read unconditionally, HuffmanUtil.cpp:550-556).
  int16_t group_of_high[256];
  std::fill(group_of_high, group_of_high + 256, (int16_t)-1);
  for (int s = 0; s < 256; ++s)
    if (canon_header[s] > 8) group_of_high[cc[s] >> 8] = 0;
  uint32_t ngroups = 0;
  for (int hp = 0; hp < 256; ++hp)
    if (group_of_high[hp] == 0) group_of_high[hp] = (int16_t)(++ngroups);
  const uint32_t entries = (ngroups + 1) * 256;
  if (entries > table2_cap) return MH_ERR_CAPACITY;
  std::memset(table2, 0, entries * sizeof(mh_lookup_symbol));
  for (int s = 0; s < 256; ++s) {
    const int len = canon_header[s];
    if (!len) continue;
    if (len <= 8) {
      fill_range(table1, cc[s] >> 8, 1u << (8 - len), (uint8_t)s, (uint8_t)len);
    } else {
      const int g = group_of_high[cc[s] >> 8];
      fill_range(table2 + (size_t)g * 256, cc[s] & 0xFF, 1u << (16 - len), (uint8_t)s,
                 (uint8_t)len);
    }
  }
  for (int hp = 0; hp < 256; ++hp)
    if (group_of_high[hp] > 0) table1[hp] = mh_lookup_symbol{(uint8_t)group_of_high[hp], 0};
  *table2_entries = entries;
  return MH_OK;
}

int mh_build_single_table(const uint8_t canon_header[256], mh_lookup_symbol table[65536]) {
  if (!canon_header || !table) return MH_ERR_INVALID_ARG;
  uint16_t cc[256];
  int rc = mh_canonical_codes(canon_header, cc);
  if (rc != MH_OK) return rc;
  std::memset(table, 0, 65536 * sizeof(mh_lookup_symbol));
  for (int s = 0; s < 256; ++s) {
    const int len = canon_header[s];
    if (len) fill_range(table, cc[s], 1u << (16 - len), (uint8_t)s, (uint8_t)len);
  }
  return MH_OK;
}

// The 256 elements mh_decode_crops_norm can write: one std::fmaf per byte value, then the narrowing
// by integer arithmetic (round to nearest even, subnormals kept, overflow to inf).
int mh_norm_table(uint32_t format, float scale, float bias, void *table, size_t table_bytes) {
  if (!table || format > MH_NORM_F32 || !std::isfinite(scale) || !std::isfinite(bias)) return MH_ERR_INVALID_ARG;
  if (table_bytes < 256u * (format == MH_NORM_F32 ? 4u : 2u)) return MH_ERR_CAPACITY;
  for (uint32_t v = 0; v < 256u; ++v) {
    const float f = std::fmaf((float)v, scale, bias);
    uint32_t bits;
    std::memcpy(&bits, &f, 4);
    if (format == MH_NORM_F32)
      static_cast<uint32_t *>(table)[v] = bits;
    else
      static_cast<uint16_t *>(table)[v] = format == MH_NORM_F16 ? f32_to_f16(bits) : f32_to_bf16(bits);
  }
  return MH_OK;
}

// ---- the set encoder's planner (mh_encode_set_device_async, mh_encode.hip) ------------------
// Everything the set kernels read that does not depend on a pixel, computed once on the host:
// per-frame records, the decoders' geometry records, and the two workgroup maps.

// One record under the images entries' addressing rule for one image (image_layout_fits,
// mh_encode.hip): a row and the row pitch fit a tile's 32-bit descriptor, and so does the span
// from a tile's first row to the last row one of its blocks lies in.
static bool set_source_fits(const mh_set_source &s) {
  const uint64_t row = (uint64_t)s.width * s.pixel_stride;  // < 2^24
  if (s.height > 1 && (s.row_pitch < row || s.row_pitch > MH_IMAGE_TILE_SPAN_MAX)) return false;
  const uint64_t pitch = s.height > 1 ? s.row_pitch : 0;
  const uint64_t rows = std::min<uint64_t>(s.height, MH_IMAGE_TILE_ROWS(s.width));
  return (rows - 1) * pitch + row <= MH_IMAGE_TILE_SPAN_MAX;
}

// Checks 1-5 but the blob's size, and the totals.
static int set_plan_scan(uint32_t n, const mh_set_source *src, uint32_t flags, mh_set_totals *t) {
  if (!src || !t || !n) return MH_ERR_INVALID_ARG;
  if (flags & ~(MH_FLAG_NO_DELTA | MH_ENCODE_WORKSPACE_ZEROED | MH_ENCODE_LIMIT_LENGTHS)) return MH_ERR_INVALID_ARG;
  for (uint32_t f = 0; f < n; ++f)
    if (src[f].reserved) return MH_ERR_INVALID_ARG;
  for (uint32_t f = 0; f < n; ++f) {
    const mh_set_source &s = src[f];
    if (!s.width || !s.height || s.width > MH_MAX_DIM || s.height > MH_MAX_DIM || !s.pixel_stride ||
        s.pixel_stride > 255u)
      return MH_ERR_DIMS;
  }
  for (uint32_t f = 0; f < n; ++f)
    if (!src[f].codes_cap || (src[f].codes_cap & 15u)) return MH_ERR_ALIGN;
  uint64_t blocks = 0, tiles = 0, units = 0, codes = 0;
  uint32_t wmax = 0, hmax = 0;
  uint64_t align = 0;
  bool one_stride = true, in_pixel = true;
  for (uint32_t f = 0; f < n; ++f) {
    const mh_set_source &s = src[f];
    if (!set_source_fits(s)) return MH_ERR_CAPACITY;
    const uint64_t nb = (uint64_t)((s.width + 7) / 8) * ((s.height + 7) / 8);  // < 2^26
    const uint64_t nt = (nb + mh_set::kTileBlocks - 1) / mh_set::kTileBlocks;
    blocks += nb;
    tiles += nt;
    units += (nt + mh_set::kPackTiles - 1) / mh_set::kPackTiles;
    if (codes + s.codes_cap < codes) return MH_ERR_CAPACITY;
    codes += s.codes_cap;
    wmax = std::max(wmax, s.width);
    hmax = std::max(hmax, s.height);
    align |= s.height > 1 ? s.row_pitch : 0;
    one_stride = one_stride && s.pixel_stride == src[0].pixel_stride;
    in_pixel = in_pixel && (s.pixels & 3u) < s.pixel_stride;
  }
  if (blocks > 0xFFFFFFFFull || tiles > 0x7FFFFFFFull || n > 0x7FFFFFFFu) return MH_ERR_CAPACITY;
  std::memset(t, 0, sizeof(*t));
  t->codes_bytes = codes;
  t->workspace_bytes = mh_set::carve(nullptr, n, tiles, nullptr);
  t->geoms_offset = (uint64_t)n * sizeof(mh_set_frame);
  t->split_map_offset = t->geoms_offset + (uint64_t)n * sizeof(mh_frame_geom);
  t->pack_map_offset = t->split_map_offset + mh_set::align16(tiles * 8);
  t->plan_bytes = t->pack_map_offset + mh_set::align16(units * 8);
  t->n_frames = n;
  t->total_blocks = (uint32_t)blocks;
  t->total_tiles = (uint32_t)tiles;
  t->split_grid = (uint32_t)tiles;
  t->pack_grid = (uint32_t)units;
  t->max_width = wmax;
  t->max_height = hmax;
  t->fetch_mode = one_stride && in_pixel && src[0].pixel_stride <= 4u && !(align & 3u) ? src[0].pixel_stride : mh_set::kByteMode;
  return MH_OK;
}

size_t mh_encode_set_plan_bytes(uint32_t n_frames, const mh_set_source *sources) {
  mh_set_totals t;
  return set_plan_scan(n_frames, sources, 0, &t) == MH_OK ? (size_t)t.plan_bytes : 0;
}

int mh_encode_set_plan(uint32_t n_frames, const mh_set_source *sources, uint32_t flags, void *h_plan,
                       size_t plan_bytes, mh_set_totals *totals) {
  if (!h_plan) return MH_ERR_INVALID_ARG;
  mh_set_totals t;
  const int rc = set_plan_scan(n_frames, sources, flags, totals ? &t : nullptr);
  if (rc != MH_OK) return rc;
  if (plan_bytes < t.plan_bytes) return MH_ERR_CAPACITY;
  uint8_t *p = static_cast<uint8_t *>(h_plan);
  std::memset(p, 0, (size_t)t.plan_bytes);
  // the blob may sit at any host address: every record goes in by memcpy
  uint64_t slot = 0;
  uint32_t first_tile = 0, first_block = 0, unit = 0;
  for (uint32_t f = 0; f < n_frames; ++f) {
    const mh_set_source &s = sources[f];
    mh_set_frame r;
    std::memset(&r, 0, sizeof(r));
    r.pixels = s.pixels;
    r.slot_offset = slot;
    r.codes_cap = s.codes_cap;
    r.row_pitch = s.height > 1 ? (uint32_t)s.row_pitch : 0u;  // <= MH_IMAGE_TILE_SPAN_MAX
    r.pixel_stride = s.pixel_stride;
    r.width = s.width;
    r.height = s.height;
    r.block_width = (s.width + 7) / 8;
    r.n_blocks = r.block_width * ((s.height + 7) / 8);
    r.n_tiles = (r.n_blocks + mh_set::kTileBlocks - 1) / mh_set::kTileBlocks;
    r.first_tile = first_tile;
    r.first_block = first_block;
    std::memcpy(p + (size_t)f * sizeof(r), &r, sizeof(r));
    const mh_frame_geom g = {first_block, s.width, s.height, 0};
    std::memcpy(p + t.geoms_offset + (size_t)f * sizeof(g), &g, sizeof(g));
    for (uint32_t k = 0; k < r.n_tiles; ++k) {
      const uint32_t e[2] = {f, k};
      std::memcpy(p + t.split_map_offset + (size_t)(first_tile + k) * 8, e, 8);
    }
    for (uint32_t k = 0; k < r.n_tiles; k += mh_set::kPackTiles, ++unit) {
      const uint32_t e[2] = {f, k};
      std::memcpy(p + t.pack_map_offset + (size_t)unit * 8, e, 8);
    }
    slot += s.codes_cap;
    first_tile += r.n_tiles;
    first_block += r.n_blocks;
  }
  *totals = t;
  return MH_OK;
}

// mh_decode_set_frames' planner: the rasters laid out densely in frame order and the launch's
// workgroups shared out in proportion to the frames' tiles. Two passes over the records: the first
// judges them and counts, the second (only with room for the whole map) writes.
int mh_decode_set_plan(uint32_t n_frames, const mh_frame_geom *h_geoms, uint32_t group_budget, uint32_t pitch_align,
                       mh_set_raster *h_rasters, mh_set_share *h_shares, uint32_t *h_group_frame,
                       uint32_t group_capacity, uint32_t *n_groups, uint64_t *out_bytes) {
  if (!h_geoms || !n_groups || !out_bytes || n_frames == 0 || group_budget == 0) return MH_ERR_INVALID_ARG;
  if (pitch_align > 4096u || (pitch_align & (pitch_align - 1u))) return MH_ERR_INVALID_ARG;
  if (group_capacity != 0 && (!h_rasters || !h_shares || !h_group_frame)) return MH_ERR_INVALID_ARG;
  const uint64_t A = pitch_align > 8u ? pitch_align : 8u;
  const auto tiles_of = [](const mh_frame_geom &g) {
    return (uint64_t)(((g.width + 7u) / 8u) * ((g.height + 7u) / 8u) + 63u) / 64u;  // NB <= 2^26
  };
  uint64_t sum = 0;
  for (uint32_t f = 0; f < n_frames; ++f) {
    const mh_frame_geom &g = h_geoms[f];
    if (g.reserved || g.width - 1u > MH_MAX_DIM - 1u || g.height - 1u > MH_MAX_DIM - 1u) return MH_ERR_DIMS;
    const uint64_t nb = (uint64_t)((g.width + 7u) / 8u) * ((g.height + 7u) / 8u);
    if ((uint64_t)g.first_block + nb > (1ull << 32)) return MH_ERR_DIMS;
    sum += tiles_of(g);  // <= 2^32 * 2^20
  }
  // half rounds up: floor((2 budget tiles + sum) / (2 sum)), below 2^33 * 2^20 + 2^52
  const auto groups_of = [&](uint64_t tiles) {
    const uint64_t want = (2ull * group_budget * tiles + sum) / (2ull * sum);
    const uint64_t cap = (tiles + MH_DECODE_GROUP_WAVES - 1u) / MH_DECODE_GROUP_WAVES;
    return want < 1u ? 1ull : want > cap ? cap : want;
  };
  for (int pass = 0; pass < 2; ++pass) {
    uint64_t groups = 0, bytes = 0;
    for (uint32_t f = 0; f < n_frames; ++f) {
      const mh_frame_geom &g = h_geoms[f];
      const uint64_t pitch = (g.width + A - 1u) / A * A, offset = (bytes + A - 1u) / A * A;
      const uint64_t size = pitch * g.height, gf = groups_of(tiles_of(g));
      if (offset < bytes || offset + size < offset) return MH_ERR_DIMS;
      if (pass) {
        h_rasters[f] = mh_set_raster{offset, (uint32_t)pitch, 0u};
        h_shares[f] = mh_set_share{(uint32_t)groups, (uint32_t)gf, {0u, 0u}};
        for (uint64_t k = 0; k < gf; ++k) h_group_frame[groups + k] = f;
      }
      bytes = offset + size;
      groups += gf;
      if (groups > 0x7FFFFFFFull) return MH_ERR_DIMS;
    }
    if (pass) break;
    *n_groups = (uint32_t)groups;
    *out_bytes = bytes;
    if (group_capacity < groups) return MH_ERR_CAPACITY;
  }
  return MH_OK;
}

const char *mh_error_string(int status) {
  switch (status) {
    case MH_OK: return "ok";
    case MH_ERR_INVALID_ARG: return "invalid argument";
    case MH_ERR_DIMS: return "invalid dimensions";
    case MH_ERR_CODE_TOO_LONG: return "huffman code longer than 16 bits";
    case MH_ERR_CAPACITY: return "buffer too small";
    case MH_ERR_TABLE: return "invalid lookup table";
    case MH_ERR_ALIGN: return "misaligned buffer or pitch";
    case MH_ERR_HIP: return "HIP runtime error";
    case MH_ERR_EMPTY: return "no symbols";
    case MH_ERR_STREAM: return "code bits and block offsets disagree";
    default: return "unknown error";
  }
}

}  // extern "C"
