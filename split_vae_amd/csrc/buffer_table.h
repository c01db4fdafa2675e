// Workspace buffer table of the objects that sequence launches over one caller-owned workspace (lgvae_plan.hip, gm_encoder.hip).
//
// The owner declares ONE list of buffers: an enum of ids and, in the same order, their public names.  That order is also the order of
// the buffers in the workspace: layout() walks the ids, so a buffer's position cannot drift from its id and "b follows a" is a fact of
// the list, not of the order of some calls.  Offsets and sizes are kept by id; the pointers are resolved once, in bind().  Only
// lookup() -- the body of the public sv_*_buffer queries -- compares names.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "../../include/splitvae.h"

template <int N>
struct BufTable {
  const char* const* names;      // N public names, in id (= layout) order
  int64_t off[N], bytes[N];      // off < 0: this object has no such buffer (its mode or dtype lacks it)
  void* ptr[N];                  // workspace + off after bind(); NULL for an absent buffer, by declaration and never by a misspelt name
  int64_t ws_bytes = 0;

  explicit BufTable(const char* const* names_) : names(names_) {
    for (int i = 0; i < N; ++i) { off[i] = -1; bytes[i] = 0; ptr[i] = nullptr; }
  }
  // size[id] < 0: absent.  Every buffer starts on a 256-byte boundary.
  void layout(const int64_t (&size)[N]) {
    ws_bytes = 0;
    for (int i = 0; i < N; ++i) {
      if (size[i] < 0) continue;
      off[i] = ws_bytes; bytes[i] = size[i];
      ws_bytes += (size[i] + 255) / 256 * 256;
    }
  }
  bool has(int id) const { return off[id] >= 0; }
  // first .. last (by id) are all there: what zero() then clears is exactly those buffers.  Checked once, when the object is created.
  bool run(int first, int last) const {
    for (int i = first; i <= last; ++i)
      if (!has(i)) return false;
    return first <= last;
  }
  // one memset from the start of `first` to the end of `last`
  int zero(int first, int last, hipStream_t st) const {
    const hipError_t e = hipMemsetAsync(ptr[first], 0, (size_t)(off[last] + bytes[last] - off[first]), st);
    return e == hipSuccess ? SV_OK : (int)e;
  }
  int lookup(const char* name, int64_t* offset, int64_t* nbytes) const {
    if (!name) return SV_E_BADARG;
    for (int i = 0; i < N; ++i)
      if (has(i) && !strcmp(names[i], name)) {
        if (offset) *offset = off[i];
        if (nbytes) *nbytes = bytes[i];
        return SV_OK;
      }
    return SV_E_BADARG;
  }
  // The whole workspace starts from ZERO: pad channels / pad rows of the activation, gradient and weight-image buffers that no kernel ever writes are read as
  // zeros by the MFMA kernels, and a few accumulators (metric_acc, the polyphase head's dbias') count up from zero.  The Python mirror used to hand in a zeroed
  // tensor; a C caller's hipMalloc'd block is garbage (scripts/ws_poison_probe.py: with 0xFF bytes every loss was NaN), so the bind does it itself.
  // Then the owner's job table (host memory that may go away) is copied into buffer `jobs_id`, and the copy finished.
  int bind(void* workspace, int64_t nbytes, hipStream_t st, int jobs_id, const void* jobs, size_t jobs_bytes) {
    if (!workspace) return SV_E_BADARG;
    if (nbytes < ws_bytes) return SV_E_WORKSPACE;
    if ((uintptr_t)workspace & 255) return SV_E_BADARG;
    for (int i = 0; i < N; ++i) ptr[i] = has(i) ? (char*)workspace + off[i] : nullptr;
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)ws_bytes, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ptr[jobs_id], jobs, jobs_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? SV_OK : (int)e;
  }
};
