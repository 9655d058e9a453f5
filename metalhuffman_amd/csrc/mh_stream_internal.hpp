// mh_stream_internal.hpp -- struct mh_stream, shared by mh_stream.cpp (streams whose
// frames share the table pair fixed at mh_stream_create) and mh_stream_headers.cpp
// (streams whose frames bring a canonical header each). Not part of the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/metalhuffman.h"

struct mh_stream {
  struct Slot {
    // one allocation. Table mode: [block offsets, padded to 16 B][codes];
    // header mode: [status, 16 B][header, 256 B][block offsets, padded to 16 B][codes]
    uint8_t *base = nullptr;
    uint8_t *codes = nullptr;
    uint32_t *offsets = nullptr;
    uint8_t *init = nullptr;
    uint8_t *out = nullptr;
    bool own_out = true;
    hipEvent_t start = nullptr;  // before the slot's copy (timing event)
    hipEvent_t done = nullptr;   // after the slot's decode (timing event)
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipStream_t stream = nullptr;  // this slot's copies + decode, in order
    bool used = false;
    int32_t *status = nullptr;   // header mode: the header's verdict, written by the decode
    uint8_t *header = nullptr;   // header mode: the frame's 256 code lengths
  };
  int device = 0;
  uint32_t last = 0;  // slot of the most recent submit
  mh_frame proto{};
  uint64_t cap = 0;
  uint64_t nb = 0;
  uint64_t off_bytes = 0;  // nb * 4 rounded up to 16
  size_t pitch = 0, out_bytes = 0;
  uint32_t next = 0;
  bool graphs = true;
  bool headers = false;  // header mode (mh_stream_create_headers)
  std::vector<Slot> slots;
};

namespace {

// Makes `dev` current for the scope (and restores the caller's device): every
// stream call may come from any host thread with any current device.
struct DeviceGuard {
  int prev = -1;
  bool ok = true;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) {
      ok = false;
      return;
    }
    if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

}  // namespace
