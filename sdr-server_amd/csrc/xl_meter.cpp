// xl_meter.cpp -- the power meter (include/xlating_meter.h): the mean power of many device rows by one launch, one table copy and one
// copy back.  The rule is xl_meter_rule.h's; the kernels xl_meter.hip.
//
// One measurement = one table of runs written into pinned memory and uploaded by one copy, the ragged launch, which leaves one
// partial of 8 bytes per workgroup in a device table, and one copy of those partials into pinned memory, all on the caller's stream,
// with the event `done` behind them.  The ring of pinned tables and the single device table are xl_bank_host.h's.  ONE measurement is
// outstanding: the next is refused until this one has been seen done, so the device tables and the pinned partials are never replaced
// or rewritten under work that still uses them, and nothing here waits on the host but xlating_meter_wait.
#include "../../include/xlating_meter.h"

#include <errno.h>

#include <algorithm>
#include <new>
#include <vector>

#include "xl_bank_host.h"
#include "xl_common.h"
#include "xl_meter.h"
#include "xl_meter_rule.h"

namespace {

struct XlMeterRow {
  uint64_t cnt = 0;
  size_t first = 0, pieces = 0;  // its partials
};

}  // namespace

struct xlating_meter {
  int device = 0;
  hipEvent_t done = nullptr;  // behind the latest measurement's copy back
  bool issued = false;        // `done` has been recorded ...
  bool seen_done = true;      // ... and has been seen passed
  bool broken = false;
  bool cs16 = false;
  std::vector<XlMeterRow> rows;  // of the latest measurement
  XlTableRing ring;              // the measurements' tables of runs
  uint64_t *d_part = nullptr, *h_part = nullptr;  // a partial per workgroup: device, pinned
  size_t part_cap = 0;
  unsigned launches = 0, copies = 0;
};

// 1 done, 0 not yet, -EIO
static int xl_meter_done(xlating_meter *m) {
  if (!m->issued || m->seen_done) return 1;
  const hipError_t e = hipEventQuery(m->done);
  if (e == hipErrorNotReady) {
    (void)hipGetLastError();  // (not an error: clear the sticky code)
    return 0;
  }
  if (e != hipSuccess) {
    m->broken = true;
    return -EIO;
  }
  m->seen_done = true;
  return 1;
}

static int xl_meter_measure(xlating_meter *m, bool cs16, size_t n, const void *const *dev_rows, const size_t *counts, hipStream_t st) {
  size_t nruns = 0;
  uint64_t W = 0;
  for (size_t i = 0; i < n; ++i) {
    if (counts[i] > XL_METER_COUNT_MAX) return -EINVAL;
    if (counts[i] == 0) continue;
    if (dev_rows[i] == nullptr || ((uintptr_t)dev_rows[i] & (cs16 ? 3u : 7u)) != 0u) return -EINVAL;
    W += xl_meter_pieces(counts[i]);
    ++nruns;
  }
  if (W >= ((uint64_t)1 << 31)) return -ENOMEM;  // (the ragged launch counts its workgroups in 32 bits)
  m->rows.resize(n);  // (bad_alloc: the caller's)
  const size_t bytes = nruns * sizeof(XlMeterRun);
  XlRingTable *t = nullptr;
  if (nruns > 0) {
    XL_TRY_RET(hipSetDevice(m->device));
    if (W > m->part_cap) {  // (nothing of this object's is in flight: the previous measurement has been seen done)
      if (m->d_part) (void)hipFree(m->d_part);
      if (m->h_part) (void)hipHostFree(m->h_part);
      m->d_part = m->h_part = nullptr, m->part_cap = 0;
      const size_t cap = std::max<size_t>((size_t)(W + W / 2), 1024);
      hipError_t e = hipMalloc(reinterpret_cast<void **>(&m->d_part), cap * sizeof(uint64_t));
      if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void **>(&m->h_part), cap * sizeof(uint64_t), hipHostMallocDefault);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        XL_LOG_ERR("meter: partials of %zu pieces: %s", cap, hipGetErrorString(e));
        if (m->d_part) (void)hipFree(m->d_part);
        m->d_part = m->h_part = nullptr;
        m->rows.clear();
        return -ENOMEM;
      }
      m->part_cap = cap;
    }
    const hipError_t e = xl_ring_acquire(&m->ring, bytes, &t);
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      m->rows.clear();
      return -ENOMEM;
    }
    XL_TRY_RET(e);
    if (m->ring.d_cap < bytes) {
      if (xl_ring_dev_grow(&m->ring, bytes) != hipSuccess) {
        (void)hipGetLastError();
        m->rows.clear();
        return -ENOMEM;  // (the ring holds no device table now; the next measurement allocates one)
      }
    }
  }
  // from here on the measurement exists
  m->cs16 = cs16, m->issued = false, m->seen_done = true;
  XlMeterRun *runs = nruns > 0 ? static_cast<XlMeterRun *>(t->h) : nullptr;
  uint32_t w = 0;
  size_t k = 0;
  for (size_t i = 0; i < n; ++i) {
    XlMeterRow &row = m->rows[i];
    row.cnt = counts[i], row.first = w, row.pieces = (size_t)xl_meter_pieces(counts[i]);
    if (counts[i] == 0) continue;
    XlMeterRun &r = runs[k++];
    r.src = dev_rows[i], r.cnt = (uint32_t)counts[i], r.wsum = w;
    w += (uint32_t)row.pieces;
  }
  if (nruns == 0) return 0;
  XL_TRY_RET(xl_ring_upload(&m->ring, t, bytes, st));
  m->copies += 1;
  XL_TRY_RET(xl_meter_launch(cs16, static_cast<const XlMeterRun *>(m->ring.d_tab), (uint32_t)nruns, w, m->d_part, st));
  m->launches += 1;
  XL_TRY_RET(hipMemcpyAsync(m->h_part, m->d_part, (size_t)w * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  m->copies += 1;
  XL_TRY_RET(hipEventRecord(m->done, st));
  m->issued = true, m->seen_done = false;
  return 0;
}

extern "C" int xlating_meter_create(xlating_meter **out) {
  if (out == nullptr) return -EINVAL;
  *out = nullptr;
  const int device = xl_hip_select_device(-1);
  if (device < 0) {
    XL_LOG_ERR("xlating_meter_create: no usable HIP device (%s); there is no CPU path", xlating_hip_device_info());
    return -ENODEV;
  }
  xlating_meter *m = new (std::nothrow) xlating_meter();
  if (m == nullptr) return -ENOMEM;
  m->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&m->done, hipEventDisableTiming);
  if (e == hipSuccess) e = xl_ring_init(&m->ring);
  if (e != hipSuccess) {
    xl_last_hip_error = e;
    XL_LOG_ERR("xlating_meter_create: %s", hipGetErrorString(e));
    const int rc = xl_errno_of_last_hip_error();
    xlating_meter_destroy(m);
    return rc;
  }
  *out = m;
  return 0;
}

extern "C" int xlating_meter_measure_device(xlating_meter *m, int fmt, size_t n, const void *const *dev_rows, const size_t *counts,
                                            void *hip_stream) {
  if (m == nullptr || (fmt != XL_METER_CF32 && fmt != XL_METER_CS16) || (n > 0 && (dev_rows == nullptr || counts == nullptr))) return -EINVAL;
  if (m->broken) return -EIO;
  m->launches = m->copies = 0;  // (a refused measurement issued nothing)
  const int done = xl_meter_done(m);
  if (done <= 0) return done < 0 ? done : -EBUSY;
  int rc;
  try {
    rc = xl_meter_measure(m, fmt == XL_METER_CS16, n, dev_rows, counts, static_cast<hipStream_t>(hip_stream));
  } catch (const std::bad_alloc &) {  // (the rows are sized before anything is enqueued)
    rc = -ENOMEM;
  }
  if (rc != 0 && rc != -EINVAL && rc != -ENOMEM) m->broken = true;  // (-EINVAL and -ENOMEM are decided before anything is issued)
  return rc;
}

extern "C" int xlating_meter_query(xlating_meter *m) {
  if (m == nullptr) return -EINVAL;
  if (m->broken) return -EIO;
  return xl_meter_done(m);
}

extern "C" int xlating_meter_wait(xlating_meter *m) {
  if (m == nullptr) return -EINVAL;
  if (m->broken) return -EIO;
  if (!m->issued || m->seen_done) return 0;
  if (hipEventSynchronize(m->done) != hipSuccess) {
    m->broken = true;
    return -EIO;
  }
  m->seen_done = true;
  return 0;
}

extern "C" int xlating_meter_power(xlating_meter *m, size_t i, double *mean_power, uint64_t *samples) {
  if (m == nullptr || i >= m->rows.size()) return -EINVAL;
  if (m->broken) return -EIO;
  const int done = xl_meter_done(m);
  if (done <= 0) return done < 0 ? done : -EBUSY;
  const XlMeterRow &r = m->rows[i];
  const uint64_t *p = r.pieces > 0 ? m->h_part + r.first : nullptr;
  if (mean_power) *mean_power = m->cs16 ? xl_meter_mean_cs16(p, r.pieces, r.cnt) : xl_meter_mean_cf32(p, r.pieces, r.cnt);
  if (samples) *samples = r.cnt;
  return 0;
}

extern "C" int xlating_meter_partials(xlating_meter *m, size_t i, size_t cap, uint64_t *partials) {
  if (m == nullptr || i >= m->rows.size() || (cap > 0 && partials == nullptr)) return -EINVAL;
  if (m->broken) return -EIO;
  const int done = xl_meter_done(m);
  if (done <= 0) return done < 0 ? done : -EBUSY;
  const XlMeterRow &r = m->rows[i];
  const size_t k = std::min(cap, r.pieces);
  if (k > 0) std::copy(m->h_part + r.first, m->h_part + r.first + k, partials);
  return (int)r.pieces;
}

extern "C" int xlating_meter_last_ops(const xlating_meter *m, unsigned *launches, unsigned *copies) {
  if (m == nullptr) return -EINVAL;
  if (launches) *launches = m->launches;
  if (copies) *copies = m->copies;
  return 0;
}

extern "C" unsigned xlating_meter_piece_samples(void) { return XL_METER_PIECE; }

extern "C" void xlating_meter_destroy(xlating_meter *m) {
  if (m == nullptr) return;
  (void)hipSetDevice(m->device);
  if (m->issued) (void)hipEventSynchronize(m->done);
  xl_ring_destroy(&m->ring);
  if (m->d_part) (void)hipFree(m->d_part);
  if (m->h_part) (void)hipHostFree(m->h_part);
  if (m->done) (void)hipEventDestroy(m->done);
  delete m;
}
