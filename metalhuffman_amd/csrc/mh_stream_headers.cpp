// mh_stream_headers.cpp -- the stream in table-per-frame mode: every frame brings its
// own 256-byte canonical header, as every producer here writes one (mh_encode_frame, the
// GPU encoders) and as the reference builds its tables per image
// (Shared/AAPLRenderer.m:608). mh_stream.cpp's slots, streams, events and graphs, with
//   * a slot of one allocation [status, 16 B][header, 256 B][block offsets, padded to
//     16 B][codes], so a host buffer laid out header | offsets | codes moves in one DMA;
//   * one mh_decode_headers launch per frame (n_frames = 1), which builds the frame's
//     table in LDS from the header and writes the header's verdict into the slot's status
//     word: no table launch, no prepared table in memory.
// The launch is direct by default. Replayed from a captured graph (MH_STREAM_GRAPHS=1) the
// same launch measured 76.1 us of device latency per 2048x1536 frame against 68.8 us direct,
// and a graph of mh_build_luts_device + mh_decode_frames 78.6 us; the two launches issued
// directly take 72.4 us (profiles/stream_headers_ab*.txt).
// Every other mh_stream_* call works on such a stream unchanged (mh_stream.cpp).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <new>

#include "../../include/metalhuffman.h"
#include "mh_stream_internal.hpp"

namespace {

constexpr uint64_t kStatusBytes = 16, kHeaderBytes = 256;

int decode_slot(mh_stream *s, mh_stream::Slot &sl) {
  mh_frame f = s->proto;
  f.d_codes = sl.codes;
  f.codes_bytes = s->cap;
  f.d_block_offsets = sl.offsets;
  f.d_block_init = sl.init;
  return mh_decode_headers(&f, sl.header, nullptr, sl.status, sl.out, s->pitch, s->out_bytes, sl.stream);
}

}  // namespace

extern "C" {

int mh_stream_create_headers(const mh_frame *proto, uint64_t codes_capacity, uint32_t n_slots,
                             uint8_t *const *d_outputs, mh_stream **out) {
  if (!proto || !out || n_slots < 1 || n_slots > 64 || codes_capacity < MH_CODES_PAD) return MH_ERR_INVALID_ARG;
  if (proto->flags & ~MH_FLAG_NO_DELTA) return MH_ERR_INVALID_ARG;  // as mh_stream_create
  const mh_dims &d = proto->dims;
  if (!d.width || !d.height || d.width > MH_MAX_DIM || d.height > MH_MAX_DIM ||
      d.block_width != (d.width + 7) / 8 || d.block_height != (d.height + 7) / 8)
    return MH_ERR_DIMS;
  *out = nullptr;
  mh_stream *s = new (std::nothrow) mh_stream();
  if (!s) return MH_ERR_CAPACITY;
  s->headers = true;
  s->proto = *proto;
  s->proto.n_frames = 1;
  s->proto.d_frame_code_offsets = nullptr;
  s->proto.d_table1 = s->proto.d_table2 = nullptr;  // ignored by mh_decode_headers
  s->proto.table2_entries = 0;
  s->proto.d_lut = nullptr;
  s->cap = (codes_capacity + 15) & ~15ull;
  s->nb = (uint64_t)d.block_width * d.block_height;
  s->off_bytes = (s->nb * 4 + 15) & ~15ull;
  s->pitch = ((size_t)d.width + 7) & ~(size_t)7;
  s->out_bytes = s->pitch * d.height;
  s->slots.resize(n_slots);
  const bool want_init = proto->d_block_init != nullptr;
  // direct launches unless MH_STREAM_GRAPHS=1 asks for per-slot graph replays (A/B; 0 = direct, as
  // in table mode)
  const char *ge = std::getenv("MH_STREAM_GRAPHS");
  s->graphs = ge && ge[0] == '1';
  const uint64_t slot_bytes = kStatusBytes + kHeaderBytes + s->off_bytes + s->cap;
  int rc = MH_OK;
  if (hipGetDevice(&s->device) != hipSuccess) rc = MH_ERR_HIP;
  for (uint32_t i = 0; i < n_slots && rc == MH_OK; ++i) {
    mh_stream::Slot &sl = s->slots[i];
    if (d_outputs) {
      sl.out = d_outputs[i];
      sl.own_out = false;
      if (!sl.out || ((uintptr_t)sl.out & 7u)) {
        rc = MH_ERR_ALIGN;
        break;
      }
    }
    if (hipMalloc(&sl.base, slot_bytes) != hipSuccess ||
        (want_init && hipMalloc(&sl.init, s->nb) != hipSuccess) ||
        (!d_outputs && hipMalloc(&sl.out, s->out_bytes) != hipSuccess) ||
        hipMemset(sl.base, 0, slot_bytes) != hipSuccess ||
        (want_init && hipMemset(sl.init, 0, s->nb) != hipSuccess) ||
        hipEventCreate(&sl.start) != hipSuccess || hipEventCreate(&sl.done) != hipSuccess ||
        hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking) != hipSuccess) {
      rc = MH_ERR_HIP;
      break;
    }
    sl.status = reinterpret_cast<int32_t *>(sl.base);
    sl.header = sl.base + kStatusBytes;
    sl.offsets = reinterpret_cast<uint32_t *>(sl.header + kHeaderBytes);
    sl.codes = sl.header + kHeaderBytes + s->off_bytes;
    // The warm-up decode and the capture run on a header of 17-bit lengths, which the
    // kernel rejects: creating a stream stores nothing into the slots' rasters.
    if (hipMemset(sl.header, 17, kHeaderBytes) != hipSuccess) {
      rc = MH_ERR_HIP;
      break;
    }
    // one eager decode first: validates the arguments and caches the launch geometry
    // queries outside the capture
    rc = decode_slot(s, sl);
    if (rc != MH_OK) break;
    if (s->graphs) {
      if (hipStreamBeginCapture(sl.stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
        rc = MH_ERR_HIP;
        break;
      }
      const int drc = decode_slot(s, sl);
      hipGraph_t g = nullptr;
      const hipError_t e = hipStreamEndCapture(sl.stream, &g);
      sl.graph = g;
      if (drc != MH_OK || e != hipSuccess) {
        rc = drc != MH_OK ? drc : MH_ERR_HIP;
        break;
      }
      if (hipGraphInstantiate(&sl.exec, sl.graph, nullptr, nullptr, 0) != hipSuccess) {
        rc = MH_ERR_HIP;
        break;
      }
    }
    // behind the warm-up on the slot's stream: an unused slot reports MH_OK
    if (hipStreamSynchronize(sl.stream) != hipSuccess || hipMemset(sl.base, 0, kStatusBytes) != hipSuccess)
      rc = MH_ERR_HIP;
  }
  if (rc == MH_OK && hipDeviceSynchronize() != hipSuccess) rc = MH_ERR_HIP;
  if (rc != MH_OK) {
    (void)mh_stream_destroy(s);
    return rc;
  }
  *out = s;
  return MH_OK;
}

int mh_stream_submit_header(mh_stream *s, const uint8_t *h_canon_header, const uint8_t *h_codes,
                            uint64_t codes_bytes, const uint32_t *h_block_offsets,
                            const uint8_t *h_block_init, uint32_t *slot_out) {
  if (!s || !h_canon_header || !h_codes || !h_block_offsets) return MH_ERR_INVALID_ARG;
  if (!s->headers) return MH_ERR_INVALID_ARG;  // a table-mode stream: mh_stream_submit
  if (codes_bytes < MH_CODES_PAD || codes_bytes > s->cap) return MH_ERR_CAPACITY;
  if (!h_block_init != !s->slots[0].init) return MH_ERR_INVALID_ARG;
  const uint32_t k = s->next;
  mh_stream::Slot &sl = s->slots[k];
  DeviceGuard dg(s->device);
  if (!dg.ok) return MH_ERR_HIP;
  if (hipEventRecord(sl.start, sl.stream) != hipSuccess) return MH_ERR_HIP;
  // copies then decode on the slot's own stream (its previous decode is ahead in it). Host
  // buffers laid out like the slot ([header][offsets, padded to 16 B][codes]): one DMA;
  // otherwise one per part
  const uint8_t *h_off8 = reinterpret_cast<const uint8_t *>(h_block_offsets);
  const bool packed = h_off8 == h_canon_header + kHeaderBytes && h_codes == h_off8 + s->off_bytes;
  if ((packed ? hipMemcpyAsync(sl.header, h_canon_header, kHeaderBytes + s->off_bytes + codes_bytes,
                               hipMemcpyHostToDevice, sl.stream) != hipSuccess
              : (hipMemcpyAsync(sl.header, h_canon_header, kHeaderBytes, hipMemcpyHostToDevice, sl.stream) !=
                     hipSuccess ||
                 hipMemcpyAsync(sl.codes, h_codes, codes_bytes, hipMemcpyHostToDevice, sl.stream) != hipSuccess ||
                 hipMemcpyAsync(sl.offsets, h_block_offsets, s->nb * 4, hipMemcpyHostToDevice, sl.stream) !=
                     hipSuccess)) ||
      (h_block_init &&
       hipMemcpyAsync(sl.init, h_block_init, s->nb, hipMemcpyHostToDevice, sl.stream) != hipSuccess) ||
      (s->graphs ? hipGraphLaunch(sl.exec, sl.stream) != hipSuccess : decode_slot(s, sl) != MH_OK) ||
      hipEventRecord(sl.done, sl.stream) != hipSuccess)
    return MH_ERR_HIP;
  sl.used = true;
  s->last = k;
  s->next = (k + 1) % (uint32_t)s->slots.size();
  if (slot_out) *slot_out = k;
  return MH_OK;
}

int mh_stream_slot_status(mh_stream *s, uint32_t slot, int32_t *status) {
  if (!s || !status || slot >= s->slots.size()) return MH_ERR_INVALID_ARG;
  *status = MH_OK;
  mh_stream::Slot &sl = s->slots[slot];
  if (!s->headers || !sl.used) return MH_OK;
  DeviceGuard dg(s->device);
  if (!dg.ok) return MH_ERR_HIP;
  // behind the slot's decode on its own stream
  int32_t v = 0;
  if (hipMemcpyAsync(&v, sl.status, sizeof v, hipMemcpyDeviceToHost, sl.stream) != hipSuccess ||
      hipStreamSynchronize(sl.stream) != hipSuccess)
    return MH_ERR_HIP;
  *status = v;
  return MH_OK;
}

}  // extern "C"
