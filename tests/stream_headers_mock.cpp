// stream_headers_mock.cpp -- CPU test harness for the stream's table-per-frame mode
// (metalhuffman_amd/csrc/mh_stream_headers.cpp and mh_stream.cpp, compiled unchanged beside
// this file with g++). The HIP runtime calls they make are fakes over host memory that record
// every copy (destination, size, stream) and every decode; mh_decode and mh_decode_headers are
// fakes too. The fake mh_decode_headers gives the verdict -3 for a header whose first length is
// over 16 and 0 otherwise, writes it to the status word, and stamps the raster's first byte
// with the header's second byte unless it rejected the header. A captured graph
// (MH_STREAM_GRAPHS=1) replays the fake decode it recorded. The program checks what
// tests/test_stream_headers_host.py asks of it and exits 0.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/metalhuffman.h"

namespace {
struct FakeStream {
  int id;
};
struct Op {
  char kind;  // 'c' copy, 'd' mh_decode, 'h' mh_decode_headers (eager), 'g' graph launch
  const void *dst;
  size_t bytes;
  hipStream_t stream;
};
struct Captured {
  const uint8_t *header;
  int32_t *status;
  uint8_t *out;
  bool table_mode;
  hipStream_t stream;
};
std::vector<Op> g_ops;
int g_next_stream = 0;
bool g_capturing = false;
Captured g_capture{};
int g_fail = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); \
      ++g_fail;                                                       \
    }                                                                 \
  } while (0)

void run_headers(const uint8_t *header, int32_t *status, uint8_t *out) {
  const int32_t v = header[0] > 16 ? MH_ERR_CODE_TOO_LONG : MH_OK;
  if (status) *status = v;
  if (v == MH_OK) out[0] = header[1];
}
}  // namespace

extern "C" {
hipError_t hipGetDevice(int *d) {
  *d = 0;
  return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetDeviceCount(int *n) {
  *n = 1;
  return hipSuccess;
}
hipError_t hipMalloc(void **p, size_t n) {
  *p = std::calloc(1, n ? n : 1);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *p) {
  std::free(p);
  return hipSuccess;
}
hipError_t hipMemset(void *p, int v, size_t n) {
  std::memset(p, v, n);
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t s) {
  std::memcpy(dst, src, n);
  if (kind == hipMemcpyHostToDevice) g_ops.push_back({'c', dst, n, s});
  return hipSuccess;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned int) {
  *s = reinterpret_cast<hipStream_t>(new FakeStream{g_next_stream++});
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  delete reinterpret_cast<FakeStream *>(s);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipEventCreate(hipEvent_t *e) {
  *e = reinterpret_cast<hipEvent_t>(new int(0));
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  delete reinterpret_cast<int *>(e);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) {
  *ms = 1.f;
  return hipSuccess;
}
hipError_t hipStreamBeginCapture(hipStream_t, hipStreamCaptureMode) {
  g_capturing = true;
  g_capture = Captured{};
  return hipSuccess;
}
hipError_t hipStreamEndCapture(hipStream_t, hipGraph_t *g) {
  g_capturing = false;
  *g = reinterpret_cast<hipGraph_t>(new Captured(g_capture));
  return hipSuccess;
}
hipError_t hipGraphInstantiate(hipGraphExec_t *x, hipGraph_t g, hipGraphNode_t *, char *, size_t) {
  *x = reinterpret_cast<hipGraphExec_t>(new Captured(*reinterpret_cast<Captured *>(g)));
  return hipSuccess;
}
hipError_t hipGraphLaunch(hipGraphExec_t x, hipStream_t s) {
  const Captured &c = *reinterpret_cast<Captured *>(x);
  CHECK(c.stream == s);  // the slot's graph on the slot's stream
  if (!c.table_mode) run_headers(c.header, c.status, c.out);
  g_ops.push_back({'g', c.out, 0, s});
  return hipSuccess;
}
hipError_t hipGraphDestroy(hipGraph_t g) {
  delete reinterpret_cast<Captured *>(g);
  return hipSuccess;
}
hipError_t hipGraphExecDestroy(hipGraphExec_t x) {
  delete reinterpret_cast<Captured *>(x);
  return hipSuccess;
}
int mh_decode(const mh_frame *f, uint8_t *out, size_t, size_t, void *s) {
  CHECK(f && out && f->n_frames == 1 && f->d_table1 && f->d_table2);
  if (g_capturing)
    g_capture = Captured{nullptr, nullptr, out, true, (hipStream_t)s};
  else
    g_ops.push_back({'d', out, 0, (hipStream_t)s});
  return MH_OK;
}
int mh_decode_headers(const mh_frame *f, const uint8_t *hdr, const int32_t *fst, int32_t *hst, uint8_t *out,
                      size_t pitch, size_t, void *s) {
  CHECK(f && hdr && out && hst && !fst && f->n_frames == 1 && !f->d_frame_code_offsets);
  CHECK(!f->d_table1 && !f->d_table2 && !f->d_lut);
  CHECK(pitch == ((f->dims.width + 7) & ~7u));
  // the slot layout: [status, 16 B][header, 256 B][offsets, padded to 16 B][codes]
  const uint64_t nb = (uint64_t)f->dims.block_width * f->dims.block_height;
  CHECK(reinterpret_cast<const uint8_t *>(hst) + 16 == hdr);
  CHECK(reinterpret_cast<const uint8_t *>(f->d_block_offsets) == hdr + 256);
  CHECK(f->d_codes == hdr + 256 + ((nb * 4 + 15) & ~15ull));
  if (g_capturing) {
    g_capture = Captured{hdr, hst, out, false, (hipStream_t)s};
  } else {
    run_headers(hdr, hst, out);
    g_ops.push_back({'h', out, 0, (hipStream_t)s});
  }
  return MH_OK;
}
}  // extern "C"

namespace {

constexpr uint32_t W = 64, H = 24, NB = (W / 8) * (H / 8), OFFB = (NB * 4 + 15) & ~15u, CAP = 1024;

// one host frame, in slot layout (header | offsets | codes) or in three separate buffers
struct HostFrame {
  std::vector<uint8_t> packed, hdr, offs, codes;
  explicit HostFrame(uint8_t len0, uint8_t tag) : packed(256 + OFFB + CAP, 0), hdr(256, 0), offs(OFFB, 0), codes(CAP, 0) {
    packed[0] = hdr[0] = len0;
    packed[1] = hdr[1] = tag;
  }
};

int submit(mh_stream *s, const HostFrame &f, bool packed, const uint8_t *init, uint32_t *slot, uint64_t bytes = 64) {
  if (packed)
    return mh_stream_submit_header(s, f.packed.data(), f.packed.data() + 256 + OFFB, bytes,
                                   reinterpret_cast<const uint32_t *>(f.packed.data() + 256), init, slot);
  return mh_stream_submit_header(s, f.hdr.data(), f.codes.data(), bytes,
                                 reinterpret_cast<const uint32_t *>(f.offs.data()), init, slot);
}

void run_mode(bool graphs, bool unset = false) {
  if (unset)
    unsetenv("MH_STREAM_GRAPHS");  // header mode: direct launches by default
  else
    setenv("MH_STREAM_GRAPHS", graphs ? "1" : "0", 1);
  mh_frame proto{};
  proto.dims = {W, H, W / 8, H / 8};
  proto.n_frames = 1;
  std::vector<uint8_t> r0(W * H, 0xA5), r1(W * H, 0xA5), r2(W * H, 0xA5);
  uint8_t *outs[3] = {r0.data(), r1.data(), r2.data()};
  mh_stream *s = nullptr;
  g_ops.clear();
  CHECK(mh_stream_create_headers(&proto, CAP, 3, outs, &s) == MH_OK && s);
  // creating the stream stores nothing into the rasters, and an unused slot reports MH_OK
  CHECK(r0[0] == 0xA5 && r1[0] == 0xA5 && r2[0] == 0xA5);
  int32_t st = 99;
  for (uint32_t k = 0; k < 3; ++k) CHECK(mh_stream_slot_status(s, k, &st) == MH_OK && st == MH_OK);
  CHECK(mh_stream_slot_status(s, 3, &st) == MH_ERR_INVALID_ARG);
  CHECK(mh_stream_slot_status(s, 0, nullptr) == MH_ERR_INVALID_ARG);
  for (const Op &o : g_ops) CHECK(o.kind != 'c');  // no frame copies at creation

  // slot rotation, copies per submit, and everything on the slot's stream
  for (uint32_t i = 0; i < 8; ++i) {
    const bool packed = (i & 1) == 0;
    HostFrame f(3, (uint8_t)(10 + i));
    uint32_t slot = 99;
    const size_t before = g_ops.size();
    CHECK(submit(s, f, packed, nullptr, &slot) == MH_OK);
    CHECK(slot == i % 3);
    hipStream_t want = (hipStream_t)mh_stream_slot_stream(s, slot);
    CHECK(want && mh_stream_compute_stream(s) == (void *)want);
    size_t copies = 0, launches = 0;
    for (size_t k = before; k < g_ops.size(); ++k) {
      CHECK(g_ops[k].stream == want);
      if (g_ops[k].kind == 'c') {
        ++copies;
        CHECK(launches == 0);  // the copies come before the decode
      } else {
        ++launches;
        CHECK(g_ops[k].kind == (graphs ? 'g' : 'h'));
        CHECK(g_ops[k].dst == outs[slot]);
      }
    }
    CHECK(copies == (packed ? 1u : 3u) && launches == 1);
    if (packed) CHECK(g_ops[before].bytes == 256 + OFFB + 64);
    CHECK(mh_stream_wait(s, slot) == MH_OK);
    CHECK(mh_stream_slot_status(s, slot, &st) == MH_OK && st == MH_OK);
    size_t pitch = 0;
    CHECK(mh_stream_output(s, slot, &pitch) == outs[slot] && pitch == W);
    CHECK(outs[slot][0] == 10 + i);  // this frame's header reached this slot's decode
    float ms = 0;
    CHECK(mh_stream_slot_time(s, slot, &ms) == MH_OK && ms > 0);
  }
  // a rejected header: status -3, raster as it was; the next frame into that slot decodes
  {
    uint32_t slot = 99;
    HostFrame bad(17, 77), good(5, 78);
    CHECK(submit(s, bad, true, nullptr, &slot) == MH_OK && slot == 2);
    const uint8_t was = 10 + 5;  // frame 5 was the last into slot 2
    CHECK(mh_stream_slot_status(s, 2, &st) == MH_OK && st == MH_ERR_CODE_TOO_LONG);
    CHECK(outs[2][0] == was);
    CHECK(submit(s, good, false, nullptr, &slot) == MH_OK && slot == 0);
    CHECK(submit(s, good, false, nullptr, &slot) == MH_OK && slot == 1);
    CHECK(submit(s, good, true, nullptr, &slot) == MH_OK && slot == 2);
    CHECK(mh_stream_slot_status(s, 2, &st) == MH_OK && st == MH_OK && outs[2][0] == 78);
  }
  // capacity and argument errors; a refused submit does not advance the rotation
  {
    HostFrame f(3, 1);
    uint32_t slot = 99;
    const size_t before = g_ops.size();
    CHECK(submit(s, f, true, nullptr, &slot, 2) == MH_ERR_CAPACITY);         // below MH_CODES_PAD
    CHECK(submit(s, f, true, nullptr, &slot, CAP + 16) == MH_ERR_CAPACITY);  // above the slot capacity
    const uint8_t init[NB] = {};
    CHECK(submit(s, f, true, init, &slot) == MH_ERR_INVALID_ARG);            // created without init bytes
    CHECK(mh_stream_submit_header(s, nullptr, f.codes.data(), 64, reinterpret_cast<const uint32_t *>(f.offs.data()),
                                  nullptr, &slot) == MH_ERR_INVALID_ARG);
    // the table-mode submit on a header-mode stream
    CHECK(mh_stream_submit(s, f.codes.data(), 64, reinterpret_cast<const uint32_t *>(f.offs.data()), nullptr, &slot) ==
          MH_ERR_INVALID_ARG);
    CHECK(g_ops.size() == before);
    CHECK(submit(s, f, true, nullptr, &slot) == MH_OK && slot == 0);
  }
  CHECK(mh_stream_synchronize(s) == MH_OK);
  CHECK(mh_stream_destroy(s) == MH_OK);

  // with init bytes: four copies from separate buffers, two from the slot layout
  proto.d_block_init = r0.data();
  CHECK(mh_stream_create_headers(&proto, CAP, 2, nullptr, &s) == MH_OK && s);
  {
    HostFrame f(3, 1);
    const uint8_t init[NB] = {};
    uint32_t slot = 99;
    size_t before = g_ops.size(), copies = 0;
    CHECK(submit(s, f, false, init, &slot) == MH_OK && slot == 0);
    for (size_t k = before; k < g_ops.size(); ++k) copies += g_ops[k].kind == 'c';
    CHECK(copies == 4);
    before = g_ops.size(), copies = 0;
    CHECK(submit(s, f, true, init, &slot) == MH_OK && slot == 1);
    for (size_t k = before; k < g_ops.size(); ++k) copies += g_ops[k].kind == 'c';
    CHECK(copies == 2);
    CHECK(submit(s, f, true, nullptr, &slot) == MH_ERR_INVALID_ARG);  // created with init bytes
  }
  CHECK(mh_stream_destroy(s) == MH_OK);
  proto.d_block_init = nullptr;

  // a table-mode stream: mh_stream_submit_header is refused, slot_status reports MH_OK
  uint8_t t1[512] = {}, t2[512] = {};
  proto.d_table1 = reinterpret_cast<const mh_lookup_symbol *>(t1);
  proto.d_table2 = reinterpret_cast<const mh_lookup_symbol *>(t2);
  proto.table2_entries = 256;
  CHECK(mh_stream_create(&proto, CAP, 2, nullptr, &s) == MH_OK && s);
  {
    HostFrame f(3, 1);
    uint32_t slot = 99;
    const size_t before = g_ops.size();
    CHECK(submit(s, f, true, nullptr, &slot) == MH_ERR_INVALID_ARG);
    CHECK(g_ops.size() == before);
    CHECK(mh_stream_submit(s, f.codes.data(), 64, reinterpret_cast<const uint32_t *>(f.offs.data()), nullptr, &slot) ==
              MH_OK && slot == 0);
    st = 99;
    CHECK(mh_stream_slot_status(s, 0, &st) == MH_OK && st == MH_OK);
  }
  CHECK(mh_stream_destroy(s) == MH_OK);
}

}  // namespace

int main() {
  run_mode(true);
  run_mode(false);
  run_mode(false, true);
  std::printf("ops %zu failures %d\n", g_ops.size(), g_fail);
  return g_fail ? 1 : 0;
}
