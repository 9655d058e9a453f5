// mh_cpu.cpp -- the product's CPU decoders (host, reentrant, no module state).
//
// The reference decodes on the CPU in two places: HuffmanUtil::decodeHuffmanBits
// (single 64K-entry table, Shared/HuffmanUtil.cpp:673-823) and
// HuffmanUtil::decodeHuffmanBitsFromTables (the T1/T2 pair the shaders use,
// :830-1046), both exposed through the ObjC facade (Shared/Huffman.mm:90-130) and run
// as the renderer's DEBUG self-check (Shared/AAPLRenderer.m:616-650). They decode
// the whole block-order symbol stream serially and optionally record each
// symbol's bit offset. mh_decode_frame_cpu is the CPU twin of mh_decode: the
// shader semantics per 8x8 block from its root bit offset (AAPLShaders.metal:
// 241-268, delta fold and init byte included) straight into the W x H raster,
// block rows spread over a persistent pool of host threads (started on first use,
// reused by every later call). None of these is called by the GPU path.
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include <pthread.h>

#include "../../include/metalhuffman.h"
#include "mh_box.hpp"

namespace {

// The 16-bit window at bit `pos` (MSB first), bytes past `n` read as zero. The
// reference reads 3 bytes at pos/8 (HuffmanUtil.cpp:700-770); 4 is the same bits.
inline uint32_t window16(const uint8_t *codes, uint64_t n, uint64_t pos) {
  const uint64_t b = pos >> 3;
  uint32_t w = 0;
  if (b + 4 <= n) {
    w = ((uint32_t)codes[b] << 24) | ((uint32_t)codes[b + 1] << 16) | ((uint32_t)codes[b + 2] << 8) |
        codes[b + 3];
  } else {
    for (uint64_t i = 0; i < 4; ++i) w = (w << 8) | (b + i < n ? codes[b + i] : 0u);
  }
  return (w << (pos & 7)) >> 16;
}

// T1/T2 lookup of a 16-bit window exactly as AAPLShaders.metal:159-170 /
// HuffmanUtil.cpp:961-995: T1 by the top 8 bits; bitWidth 0 escapes to subtable
// `symbol` of T2 indexed by the low 8 bits. An escape past T2 reads the zero entry.
inline mh_lookup_symbol split_lookup(const mh_lookup_symbol *t1, const mh_lookup_symbol *t2,
                                     uint32_t t2_entries, uint32_t pat) {
  mh_lookup_symbol e = t1[pat >> 8];
  if (e.bitWidth == 0) {
    const uint32_t idx = (uint32_t)e.symbol * MH_TABLE2_SIZE + (pat & 0xFFu);
    e = idx < t2_entries ? t2[idx] : mh_lookup_symbol{0, 0};
  }
  return e;
}

// Every window's {symbol, width} from T1/T2 as one u16 (symbol | width << 8):
// one lookup per symbol in the frame decoder, filled a T1 entry (256 windows) at a time:
// one value, or that entry's T2 subtable.
void flatten(const mh_lookup_symbol *t1, const mh_lookup_symbol *t2, uint32_t t2_entries,
             uint16_t *flat) {
  for (uint32_t h = 0; h < 256; ++h) {
    uint16_t *f = flat + h * 256u;
    const mh_lookup_symbol e = t1[h];
    if (e.bitWidth != 0) {
      std::fill(f, f + 256, (uint16_t)(e.symbol | (e.bitWidth << 8)));
    } else if ((uint32_t)e.symbol * MH_TABLE2_SIZE + 256u <= t2_entries) {
      const mh_lookup_symbol *s = t2 + (uint32_t)e.symbol * MH_TABLE2_SIZE;
      for (uint32_t l = 0; l < 256; ++l) f[l] = (uint16_t)(s[l].symbol | (s[l].bitWidth << 8));
    } else {
      std::fill(f, f + 256, (uint16_t)0);  // escape past T2: the zero entry (split_lookup)
    }
  }
}

// One block: 64 steps from `root` (the shader's per-fragment loop; its cursor is
// a 16-bit count of bits read), written as 8 rows of the raster.
inline void decode_block(const uint16_t *flat, const uint8_t *codes, uint64_t n, uint64_t root,
                         uint8_t init, bool delta, uint8_t blk[64]) {
  uint16_t nread = 0;
  uint8_t prev = init;
  if ((root >> 3) + 8 + 136 <= n) {
    // fast path: a 64-bit big-endian window, refilled when fewer than 16 bits remain
    // (a block's 64 codes span at most 128 bytes)
    const uint8_t *p = codes + (root >> 3);
    uint64_t pos = root & 7;  // bits consumed from p
    for (int k = 0; k < 64; ++k) {
      const uint64_t byte = pos >> 3;
      uint64_t w;
      std::memcpy(&w, p + byte, 8);
      w = __builtin_bswap64(w) << (pos & 7);
      const uint16_t e = flat[w >> 48];
      pos += e >> 8;
      nread = (uint16_t)(nread + (e >> 8));
      const uint8_t sym = (uint8_t)e;
      blk[k] = delta ? (prev = (uint8_t)(prev + sym)) : sym;
    }
    return;
  }
  for (int k = 0; k < 64; ++k) {
    const uint16_t e = flat[window16(codes, n, root + nread)];
    nread = (uint16_t)(nread + (e >> 8));
    const uint8_t sym = (uint8_t)e;
    blk[k] = delta ? (prev = (uint8_t)(prev + sym)) : sym;
  }
}

// kGroup neighbouring blocks of one block row decoded in lock-step: each block's
// 64-step chain (cursor -> window load -> table load -> cursor) is latency-bound on
// its own, so the blocks' independent chains are interleaved for the core to overlap.
// Same per-block semantics as decode_block's fast path; the caller checks that every
// block of the group takes that path. Writes the group's 8 x (8 * kGroup) pixels to
// `tile` (row pitch 8 * kGroup).
constexpr int kGroup = 8;
inline bool group_fast(const uint32_t *roots, uint64_t n) {
  uint32_t mx = 0;
  for (int g = 0; g < kGroup; ++g) mx = std::max(mx, roots[g]);
  return ((uint64_t)mx >> 3) + 8 + 136 <= n;
}
inline void decode_group(const uint16_t *flat, const uint8_t *codes, const uint32_t *roots,
                         const uint8_t *inits, bool delta, uint8_t *tile) {
  const uint8_t *p[kGroup];
  uint64_t pos[kGroup];
  uint8_t prev[kGroup];
  for (int g = 0; g < kGroup; ++g) {
    p[g] = codes + (roots[g] >> 3);
    pos[g] = roots[g] & 7u;
    prev[g] = inits ? inits[g] : 0;
  }
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) {
#pragma GCC unroll 8
      for (int g = 0; g < kGroup; ++g) {
        uint64_t w;
        std::memcpy(&w, p[g] + (pos[g] >> 3), 8);
        w = __builtin_bswap64(w) << (pos[g] & 7);
        const uint16_t e = flat[w >> 48];
        pos[g] += e >> 8;
        const uint8_t sym = (uint8_t)e;
        prev[g] = (uint8_t)(prev[g] + sym);
        tile[r * (8 * kGroup) + g * 8 + c] = delta ? prev[g] : sym;
      }
    }
}

// Persistent worker pool for mh_decode_frame_cpu. Round 3 started fresh threads on
// every call: 16 threads reached 5.6 x10^3 MB/s best-of but ~3.5-4.0 x10^3 per call in
// the bench line. Workers are started once (grown on demand up to the machine's
// hardware threads, never shrunk) and sleep on a condition variable between calls; a
// call hands out job indices from an atomic counter to its workers and the calling
// thread, so a call asking for more threads than the cap still runs every job, on
// fewer threads. One parallel call runs at a time (calls from several host threads
// queue on run_mutex_). No exception crosses the C ABI: a worker that cannot be
// started leaves its share to the others.
//
// fork(): the child inherits the pool's state but none of its threads. pthread_atfork
// handlers take both mutexes before the fork (so no call is half-way through), release
// them in the parent, and in the child forget the dead workers (their std::thread
// objects are leaked: neither joining nor destroying a joinable thread is possible
// there) and start from fresh mutexes and condition variables, so the child's first
// call starts its own workers.
class Pool {
 public:
  Pool() : cap_(std::max(1u, std::thread::hardware_concurrency())) {
    pthread_atfork(&Pool::prepare, &Pool::parent, &Pool::child);
  }
  ~Pool() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto &t : workers_) t.join();
  }

  // fn(j) for j in [0, njobs) on up to `threads` threads (the caller included).
  void run(uint32_t threads, uint32_t njobs, const std::function<void(uint32_t)> &fn) {
    std::lock_guard<std::mutex> call(run_mutex_);
    const uint32_t want = std::min(threads, cap_) > 1 ? std::min(threads, cap_) - 1 : 0;
    try {
      while (workers_.size() < want) {
        const uint32_t id = (uint32_t)workers_.size();
        workers_.emplace_back([this, id] { loop(id); });
      }
    } catch (...) {
    }
    {
      std::lock_guard<std::mutex> lk(m_);
      fn_ = &fn;
      njobs_ = njobs;
      next_.store(0, std::memory_order_relaxed);
      active_ = std::min<uint32_t>(want, (uint32_t)workers_.size());
      busy_ = active_;
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> lk(m_);
    done_cv_.wait(lk, [this] { return busy_ == 0; });
    fn_ = nullptr;
  }

  static Pool &get() {
    static Pool p;
    return p;
  }

 private:
  void work() {
    for (uint32_t j; (j = next_.fetch_add(1, std::memory_order_relaxed)) < njobs_;) (*fn_)(j);
  }
  void loop(uint32_t id) {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return stop_ || (gen_ != seen && id < active_); });
        if (stop_) return;
        seen = gen_;
      }
      work();
      std::lock_guard<std::mutex> lk(m_);
      if (--busy_ == 0) done_cv_.notify_one();
    }
  }
  static void prepare() {
    Pool &p = get();
    p.run_mutex_.lock();
    p.m_.lock();
  }
  static void parent() {
    Pool &p = get();
    p.m_.unlock();
    p.run_mutex_.unlock();
  }
  static void child() {
    Pool &p = get();
    // the workers do not exist here: drop their handles without touching them
    new std::vector<std::thread>(std::move(p.workers_));
    p.workers_.clear();
    p.active_ = p.busy_ = 0;
    // fresh synchronisation objects: the condition variables' internal state still
    // counts the parent's sleeping workers as waiters (a broadcast would wait for them
    // to leave), and both mutexes are held by prepare()
    new (&p.cv_) std::condition_variable();
    new (&p.done_cv_) std::condition_variable();
    new (&p.m_) std::mutex();
    new (&p.run_mutex_) std::mutex();
  }

  const uint32_t cap_;
  std::mutex run_mutex_, m_;
  std::condition_variable cv_, done_cv_;
  std::vector<std::thread> workers_;
  const std::function<void(uint32_t)> *fn_ = nullptr;
  uint32_t njobs_ = 0, active_ = 0, busy_ = 0;
  std::atomic<uint32_t> next_{0};
  uint64_t gen_ = 0;
  bool stop_ = false;
};

}  // namespace

extern "C" {

int mh_decode_huffman_bits(const mh_lookup_symbol *table, uint64_t n_symbols, const uint8_t *codes,
                           uint64_t codes_bytes, uint8_t *out, uint32_t *bit_offsets) {
  if (!table || !codes || !out) return MH_ERR_INVALID_ARG;
  uint64_t pos = 0;
  for (uint64_t i = 0; i < n_symbols; ++i) {
    if ((pos >> 3) + 2 >= codes_bytes) return MH_ERR_CAPACITY;  // the reference's DEBUG assert
    const mh_lookup_symbol e = table[window16(codes, codes_bytes, pos)];
    if (bit_offsets) bit_offsets[i] = (uint32_t)pos;
    pos += e.bitWidth;
    out[i] = e.symbol;
  }
  return MH_OK;
}

int mh_decode_huffman_bits_from_tables(const mh_lookup_symbol *table1, const mh_lookup_symbol *table2,
                                       uint32_t table2_entries, uint32_t table1_bits, uint32_t table2_bits,
                                       uint64_t n_symbols, const uint8_t *codes, uint64_t codes_bytes,
                                       uint8_t *out, uint32_t *bit_offsets) {
  if (!table1 || !table2 || !codes || !out) return MH_ERR_INVALID_ARG;
  // the reference's tables are built for 8 + 8 bits (HUFF_TABLE1/2_NUM_BITS,
  // AAPLShaderTypes.h:109-123; T2 subtables are HUFF_TABLE2_SIZE = 256 entries)
  if (table1_bits != MH_TABLE1_NUM_BITS || table2_bits != MH_TABLE2_NUM_BITS) return MH_ERR_INVALID_ARG;
  if (table2_entries < 256 || table2_entries % 256 || table2_entries > MH_TABLE2_MAX_ENTRIES)
    return MH_ERR_TABLE;
  uint64_t pos = 0;
  for (uint64_t i = 0; i < n_symbols; ++i) {
    if ((pos >> 3) + 2 >= codes_bytes) return MH_ERR_CAPACITY;
    const mh_lookup_symbol e = split_lookup(table1, table2, table2_entries, window16(codes, codes_bytes, pos));
    if (bit_offsets) bit_offsets[i] = (uint32_t)pos;
    pos += e.bitWidth;
    out[i] = e.symbol;
  }
  return MH_OK;
}

int mh_decode_frame_cpu(const uint32_t *block_offsets, const uint8_t *codes, uint64_t codes_bytes,
                        const mh_lookup_symbol *table1, const mh_lookup_symbol *table2,
                        uint32_t table2_entries, const uint8_t *block_init, uint32_t width,
                        uint32_t height, uint32_t flags, uint8_t *out, size_t out_pitch,
                        uint32_t n_threads) {
  if (!block_offsets || !codes || !table1 || !table2 || !out) return MH_ERR_INVALID_ARG;
  if (flags & ~MH_FLAG_NO_DELTA) return MH_ERR_INVALID_ARG;
  if (!width || !height || width > MH_MAX_DIM || height > MH_MAX_DIM) return MH_ERR_DIMS;
  if (table2_entries < 256 || table2_entries % 256 || table2_entries > MH_TABLE2_MAX_ENTRIES)
    return MH_ERR_TABLE;
  if (out_pitch < width) return MH_ERR_CAPACITY;
  const uint32_t bw = (width + 7) / 8, bh = (height + 7) / 8;
  const bool delta = !(flags & MH_FLAG_NO_DELTA);
  std::vector<uint16_t> flat;
  try {
    flat.resize(65536);
  } catch (...) {
    return MH_ERR_CAPACITY;  // no exception crosses the C ABI
  }
  flatten(table1, table2, table2_entries, flat.data());
  const auto rows = [&](uint32_t by0, uint32_t by1) {
    uint8_t blk[64];
    alignas(64) uint8_t tile[8 * 8 * kGroup];
    const uint32_t gw = width / (8 * kGroup);  // whole groups of full-width blocks per block row
    for (uint32_t by = by0; by < by1; ++by)
      for (uint32_t bx = 0; bx < bw; ++bx) {
        const uint32_t b = by * bw + bx;
        if (bx % kGroup == 0 && bx / kGroup < gw && group_fast(block_offsets + b, codes_bytes)) {
          decode_group(flat.data(), codes, block_offsets + b, block_init ? block_init + b : nullptr, delta,
                       tile);
          for (uint32_t r = 0; r < 8 && by * 8 + r < height; ++r)
            std::memcpy(out + (size_t)(by * 8 + r) * out_pitch + bx * 8, tile + r * 8 * kGroup, 8 * kGroup);
          bx += kGroup - 1;
          continue;
        }
        decode_block(flat.data(), codes, codes_bytes, block_offsets[b], block_init ? block_init[b] : 0,
                     delta, blk);
        const uint32_t nx = std::min(8u, width - bx * 8);
        for (uint32_t r = 0; r < 8 && by * 8 + r < height; ++r)
          std::memcpy(out + (size_t)(by * 8 + r) * out_pitch + bx * 8, blk + r * 8, nx);
      }
  };
  const uint32_t nt = std::max(1u, std::min(n_threads ? n_threads : 1u, bh));
  if (nt == 1) {
    rows(0, bh);
    return MH_OK;
  }
  // nt contiguous shares of block rows on the persistent pool (the caller takes one)
  try {
    const std::function<void(uint32_t)> job = [&](uint32_t j) {
      rows((uint32_t)((uint64_t)bh * j / nt), (uint32_t)((uint64_t)bh * (j + 1) / nt));
    };
    Pool::get().run(nt, nt, job);
  } catch (...) {
    return MH_ERR_CAPACITY;  // no exception crosses the C ABI
  }
  return MH_OK;
}

// The CPU twin of mh_check_headers for one frame: the header's verdict by the device builder's rule
// (a length over 16, then a Kraft sum over 1; an incomplete code is valid), each 16-bit window's code
// length from the canonical order -- the codes of length l fill [F, F + count[l] << (16 - l)) of the
// window space in (length, symbol) order, windows no code reaches are width 0 -- and the reference
// walk of every block: 64 steps from its offset, bytes at or past codes_bytes zero, a zero-width
// lookup not advancing, 64-bit positions.
int mh_check_frame_cpu(const uint32_t *block_offsets, uint32_t n_blocks, const uint8_t *codes,
                       uint64_t codes_bytes, const uint8_t canon_header[256], uint32_t report[4]) {
  if (!block_offsets || !n_blocks || !codes || !canon_header || !report) return MH_ERR_INVALID_ARG;
  report[0] = report[1] = report[2] = 0u;
  report[3] = 0xFFFFFFFFu;
  uint64_t kraft = 0;
  for (int s = 0; s < 256; ++s) {
    if (canon_header[s] > 16) return MH_ERR_CODE_TOO_LONG;
    if (canon_header[s]) kraft += 1ull << (16 - canon_header[s]);
  }
  if (kraft > 65536u) return MH_ERR_TABLE;
  std::vector<uint8_t> width;
  try {
    width.assign(65536, 0);
  } catch (...) {
    return MH_ERR_CAPACITY;  // no exception crosses the C ABI
  }
  uint32_t first = 0;
  for (uint32_t l = 1; l <= 16; ++l)
    for (int s = 0; s < 256; ++s)
      if (canon_header[s] == l) {
        std::memset(width.data() + first, (int)l, 1u << (16 - l));
        first += 1u << (16 - l);
      }
  for (uint32_t b = 0; b < n_blocks; ++b) {
    uint64_t pos = block_offsets[b];
    uint32_t zero = 0;
    for (int k = 0; k < 64; ++k) {
      const uint32_t len = width[window16(codes, codes_bytes, pos)];
      zero += len == 0;
      pos += len;
    }
    // the last block's end is not recorded: it must lie inside the slot
    const bool bad = b + 1 < n_blocks ? pos != block_offsets[b + 1] : pos > 8 * codes_bytes;
    report[0] += zero;
    report[2] += bad;
    if ((zero || bad) && report[3] == 0xFFFFFFFFu) report[3] = b;
  }
  return MH_OK;
}

// The CPU twin of mh_decode_region_scaled's output stage: every s x s cell's in-frame mean,
// rounded by the function the kernels round an edge cell with (mh_box.hpp).
int mh_box_reduce(const uint8_t *raster, uint32_t width, uint32_t height, size_t pitch, uint32_t log2_scale,
                  uint8_t *out, size_t out_pitch) {
  if (!raster || !out || !width || !height || log2_scale > 3) return MH_ERR_INVALID_ARG;
  const uint32_t s = 1u << log2_scale;
  const uint32_t sw = (width + s - 1) >> log2_scale, sh = (height + s - 1) >> log2_scale;
  if (pitch < width || out_pitch < sw) return MH_ERR_CAPACITY;
  for (uint32_t Y = 0; Y < sh; ++Y) {
    const uint32_t nh = std::min(s, height - Y * s);
    for (uint32_t X = 0; X < sw; ++X) {
      const uint32_t nw = std::min(s, width - X * s);
      uint32_t sum = 0;
      for (uint32_t y = 0; y < nh; ++y)
        for (uint32_t x = 0; x < nw; ++x) sum += raster[(size_t)(Y * s + y) * pitch + X * s + x];
      out[(size_t)Y * out_pitch + X] = (uint8_t)mh_box_round(sum, nw * nh);
    }
  }
  return MH_OK;
}

}  // extern "C"
