// hpgq_accum.h — what every accumulator handle does on the host (internal; the
// entry points of include/hpgq.h keep their own argument checks and return
// codes).
#pragma once
#include "hpgq_common.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace hpgq {
namespace accum {

// Every *_open: HPGQ_E_NO_DEVICE when no device is visible, HPGQ_E_INVALID for
// an index out of range, then the device is made current.
inline int use_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return HPGQ_E_NO_DEVICE;
  if (device < 0 || device >= ndev) return HPGQ_E_INVALID;
  HPGQ_HIP_TRY(hipSetDevice(device));
  return HPGQ_OK;
}

// The caller's stream, borrowed, or a non-blocking one of the handle's own.
struct Stream {
  hipStream_t s = nullptr;
  bool own = false;
  int open(void *callers) {
    if (callers) {
      s = (hipStream_t)callers;
      return HPGQ_OK;
    }
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return HPGQ_E_HIP;
    own = true;
    return HPGQ_OK;
  }
  void close() {   // (destroys only what it created)
    if (own && s) (void)hipStreamDestroy(s);
    s = nullptr;
    own = false;
  }
  operator hipStream_t() const { return s; }
};

// Device buffers replaced or lent to a kernel while the stream may still read
// them: freed when the stream is next known idle, and at close.
struct Retired {
  std::vector<void *> bufs;
  void add(void *p) { bufs.push_back(p); }
  void free_all() {   // the stream is idle
    for (void *p : bufs) (void)hipFree(p);
    bufs.clear();
  }
};

// a grid under hpgq_*_debug_set_max_workgroups (0: no limit)
inline int64_t capped(int64_t grid, int max_wg) { return max_wg > 0 ? std::min<int64_t>(grid, max_wg) : grid; }

// A batch in launches of at most kPart reads (32-bit offsets into idx; u32
// cells): launch(idx, mask, n) with the idx and mask pointers advanced.
constexpr int64_t kPart = (int64_t)1 << 28;
template <class Launch>
int for_parts(const hpgq_batch_t *b, const uint8_t *mask, Launch launch) {
  for (int64_t lo = 0; lo < b->num_reads; lo += kPart) {
    launch(b->data_indices + lo, mask ? mask + lo : nullptr, std::min(kPart, b->num_reads - lo));
    HPGQ_HIP_TRY(hipGetLastError());
  }
  return HPGQ_OK;
}

// What every handle that runs per-read kernels on one stream owns (hpgq_qdist,
// hpgq_adapt, and through hpgq_cut.h hpgq_clip and hpgq_ovl): the device, the
// stream, the buffers it replaced, the grid limits, and nscal u64 sums the
// kernels add to, with their pinned copy.
struct Handle {
  int device = 0;
  Stream stream;
  Retired retired;                          // owned buffers replaced by larger ones
  int nscal = 0;
  unsigned long long *d_scal = nullptr;     // [nscal]
  unsigned long long *h_scal = nullptr;     // pinned: the scalars, then one word that is the derived handle's (h_extra)
  int cus = 0, max_wg = 0;

  void *h_extra() const { return h_scal + nscal; }

  // After use_device.  The scalars allocated and zeroed; on an error close() frees what there is.
  int open(int dev, void *callers_stream, int scalars) {
    device = dev;
    nscal = scalars;
    const int rc = stream.open(callers_stream);
    if (rc) return rc;
    if ((nscal && hipMalloc(&d_scal, (size_t)nscal * 8) != hipSuccess) ||
        hipHostMalloc(reinterpret_cast<void **>(&h_scal), (size_t)nscal * 8 + 8, hipHostMallocDefault) != hipSuccess)
      return HPGQ_E_NOMEM;
    for (int i = 0; i <= nscal; ++i) h_scal[i] = 0;
    if (zero() != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
      return HPGQ_E_HIP;
    return HPGQ_OK;
  }

  // Waits for the stream.  The derived handle frees its own buffers after it.
  void close() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    retired.free_all();
    (void)hipFree(d_scal);
    if (h_scal) (void)hipHostFree(h_scal);
    stream.close();
  }

  hipError_t zero() { return nscal ? hipMemsetAsync(d_scal, 0, (size_t)nscal * 8, stream) : hipSuccess; }

  int reset() {
    HPGQ_HIP_TRY(hipSetDevice(device));
    HPGQ_HIP_TRY(zero());
    return HPGQ_OK;
  }

  // fetch the scalars, wait for the stream, free the replaced buffers
  int settle() {
    HPGQ_HIP_TRY(hipSetDevice(device));
    if (nscal) HPGQ_HIP_TRY(hipMemcpyAsync(h_scal, d_scal, (size_t)nscal * 8, hipMemcpyDeviceToHost, stream));
    HPGQ_HIP_TRY(hipStreamSynchronize(stream));
    retired.free_all();
    return HPGQ_OK;
  }

  // persistent grid: per_cu workgroups per CU, no more than there are read groups
  unsigned grid(int64_t per_cu, int64_t groups) const {
    return (unsigned)capped(std::min<int64_t>(per_cu * (int64_t)std::max(1, cus), groups), max_wg);
  }

  int set_max_workgroups(int n) {
    if (n < 0) return HPGQ_E_INVALID;
    max_wg = n;
    return HPGQ_OK;
  }
};

// A counter per read position (hpgq_qdist, hpgq_adapt): a table of `rows` rows
// of row_bytes of u64 on the device, position-major so that growing appends
// rows; the handle's sums beside it; and two flags the kernel keeps, [the
// longest counted read, the counted reads longer than the rows].
struct Positions : Handle {
  unsigned long long *d_table = nullptr;    // [rows][row_bytes / 8]
  int64_t rows = 0;
  size_t row_bytes = 0;
  uint32_t *d_flags = nullptr;              // (their pinned copy: h_extra)

  const uint32_t *h_flags() const { return static_cast<const uint32_t *>(h_extra()); }

  // After use_device.  Everything allocated and zeroed; on an error close() frees what there is.
  int open(int dev, void *callers_stream, int64_t nrows, size_t nrow_bytes, int scalars) {
    rows = nrows;
    row_bytes = nrow_bytes;
    const int rc = Handle::open(dev, callers_stream, scalars);
    if (rc) return rc;
    if (hipMalloc(&d_table, (size_t)rows * row_bytes) != hipSuccess || hipMalloc(&d_flags, 8) != hipSuccess)
      return HPGQ_E_NOMEM;
    return zero_table() == hipSuccess ? HPGQ_OK : HPGQ_E_HIP;
  }

  void close() {
    Handle::close();
    (void)hipFree(d_table);
    (void)hipFree(d_flags);
  }

  hipError_t zero_table() {
    const hipError_t e = hipMemsetAsync(d_table, 0, (size_t)rows * row_bytes, stream);
    return e == hipSuccess ? hipMemsetAsync(d_flags, 0, 8, stream) : e;
  }

  int reset() {
    const int rc = Handle::reset();
    if (rc) return rc;
    HPGQ_HIP_TRY(zero_table());
    return HPGQ_OK;
  }

  // Rows for reads of up to max_len: half as much again at least (a file whose
  // units grow slowly reallocates rarely), the old rows copied, the new ones
  // zeroed, the old table retired.  HPGQ_E_NOMEM: nothing changed.
  int reserve_length(int64_t max_len) {
    if (max_len < 0 || max_len > INT32_MAX) return HPGQ_E_INVALID;
    if (max_len <= rows) return HPGQ_OK;
    HPGQ_HIP_TRY(hipSetDevice(device));
    const int64_t nr = std::min<int64_t>(std::max<int64_t>(max_len, rows + rows / 2), INT32_MAX);
    unsigned long long *d = nullptr;
    if (hipMalloc(&d, (size_t)nr * row_bytes) != hipSuccess) return HPGQ_E_NOMEM;
    const size_t old = (size_t)rows * row_bytes;
    if (hipMemcpyAsync(d, d_table, old, hipMemcpyDeviceToDevice, stream) != hipSuccess ||
        hipMemsetAsync(reinterpret_cast<char *>(d) + old, 0, (size_t)nr * row_bytes - old, stream) != hipSuccess) {
      (void)hipStreamSynchronize(stream);
      (void)hipFree(d);
      return HPGQ_E_HIP;
    }
    retired.add(d_table);   // the copy above still reads it
    d_table = d;
    rows = nr;
    return HPGQ_OK;
  }

  // the handle's, with the flags fetched before the wait
  int settle() {
    HPGQ_HIP_TRY(hipSetDevice(device));
    HPGQ_HIP_TRY(hipMemcpyAsync(h_extra(), d_flags, 8, hipMemcpyDeviceToHost, stream));
    const int rc = Handle::settle();
    if (rc) return rc;
    return h_flags()[1] ? HPGQ_E_READ_TOO_LONG : HPGQ_OK;
  }

  // the first np rows to the host (after settle)
  int read_rows(void *host, size_t np) {
    if (np) HPGQ_HIP_TRY(hipMemcpy(host, d_table, np * row_bytes, hipMemcpyDeviceToHost));
    return HPGQ_OK;
  }
};

}  // namespace accum
}  // namespace hpgq
