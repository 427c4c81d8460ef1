// libgprx C ABI, the numerics of the diagnostic plots (gprx_dg_*): performance_cdf, performance_scatterplot and
// map_detection_categories of gpras/utils/plotting.py.
#include "abi_common.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "diag.h"
#include "gprx_common.h"

using namespace gprx;

extern "C" {

// ---- diagnostics (gpras/utils/plotting.py:155-233, 716-859) -------------------------------------------------
struct gprx_dg_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  Buf keys2, tab, fixed, aux;  // the second sort buffer | counts and offsets of a pass | histograms and results | partials, events, ranks
  hipEvent_t ev[3] = {};       // around the histogram sweep and the passes of the last sort
  bool timed = false;
  int last_mask = 0;           // bit p: pass p of the last sort was executed
  std::string err;
};

int gprx_dg_destroy(gprx_dg_handle h) {
  if (!h) return GPRX_OK;
  release_handle(h->device, h->stream, {h->keys2.p, h->tab.p, h->fixed.p, h->aux.p}, h->ev, 3);
  delete h;
  return GPRX_OK;
}

}  // extern "C"

namespace {
constexpr int64_t DG_MAX_N = (int64_t)1 << 40;                          // 32-bit LDS counters of the histogram sweep hold a workgroup's share
constexpr size_t DG_HIST_BYTES = sizeof(unsigned long long) * DG_PASSES * DG_BINS;
constexpr size_t DG_FIXED_BYTES = DG_HIST_BYTES + 64;                   // + res[4] doubles, the first negative event

// (n <= 2^40: every size here fits a size_t; ensure() answers GPRX_ENOMEM before it allocates what does not fit the device)
int dg_ensure(gprx_dg_handle h, Buf& b, double bytes, const char* what) { return ensure(h, b, (size_t)bytes, what); }

template <bool PAIR>
int dg_pass(gprx_dg_handle h, const void* s0, const void* s1, int64_t n, int pass, int64_t tiles, uint64_t* dst) {
  unsigned int* counts = reinterpret_cast<unsigned int*>(h->tab.p);
  // the offsets behind the counts, on an 8-byte boundary
  unsigned long long* offs = reinterpret_cast<unsigned long long*>(h->tab.p) + (DG_BINS * tiles + 1) / 2;
  const unsigned long long* hist = reinterpret_cast<const unsigned long long*>(h->fixed.p) + pass * DG_BINS;
  hipStream_t st = h->stream;
  hipLaunchKernelGGL(dg_count_kernel<PAIR>, dim3((unsigned)tiles), dim3(DG_NT), 0, st, s0, s1, n, 8 * pass, tiles, counts);
  hipLaunchKernelGGL(dg_scan_kernel, dim3(DG_BINS), dim3(DG_NT), 0, st, counts, tiles, hist, offs);
  hipLaunchKernelGGL(dg_scatter_kernel<PAIR>, dim3((unsigned)tiles), dim3(DG_NT), 0, st, s0, s1, n, 8 * pass, tiles, offs, dst);
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

// s1 null: raw keys in s0
template <bool PAIR>
int dg_sort(gprx_dg_handle h, const void* s0, const void* s1, int64_t n, void* out_dev) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  if (!s0 || (PAIR && !s1) || !out_dev) return fail(h, GPRX_EINVAL, "null argument");
  if (n < 1 || n > DG_MAX_N) return fail(h, GPRX_EINVAL, "need 1 <= n <= 2^40 keys");
  HIPCHK(h, hipSetDevice(h->device));
  const int64_t tiles = (n + DG_TILE - 1) / DG_TILE;
  int rc;
  if ((rc = dg_ensure(h, h->keys2, 8.0 * (double)n, "the second buffer of the sort"))) return rc;
  if ((rc = dg_ensure(h, h->tab, 8.0 * ((double)((DG_BINS * tiles + 1) / 2) + (double)(DG_BINS * tiles)), "the tile counts and offsets of the sort"))) return rc;
  hipStream_t st = h->stream;
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(h->fixed.p);
  HIPCHK(h, hipMemsetAsync(hist, 0, DG_HIST_BYTES, st));
  HIPCHK(h, hipEventRecord(h->ev[0], st));
  const int64_t per_block = (int64_t)DG_NT * DG_HIST_PT;
  const unsigned hist_grid = (unsigned)std::min<int64_t>((n + per_block - 1) / per_block, 2048);
  hipLaunchKernelGGL(dg_hist_kernel<PAIR>, dim3(hist_grid), dim3(DG_NT), 0, st, s0, s1, n, hist);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], st));
  static thread_local unsigned long long host_hist[DG_PASSES * DG_BINS];
  HIPCHK(h, hipMemcpyAsync(host_hist, hist, DG_HIST_BYTES, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  int mask = 0, executed = 0;
  for (int p = 0; p < DG_PASSES; ++p) {
    int bins = 0;
    unsigned long long total = 0;
    for (int d = 0; d < DG_BINS; ++d) {
      bins += host_hist[p * DG_BINS + d] != 0;
      total += host_hist[p * DG_BINS + d];
    }
    if (total != (unsigned long long)n) return fail(h, GPRX_EHIP, "the digit histogram of pass " + std::to_string(p) + " does not sum to n");
    if (bins > 1) {
      mask |= 1 << p;
      ++executed;
    }
  }
  uint64_t *out = static_cast<uint64_t*>(out_dev), *other = reinterpret_cast<uint64_t*>(h->keys2.p);
  if (!executed) {
    if (PAIR) {
      hipLaunchKernelGGL(dg_build_kernel, dim3((unsigned)std::min<int64_t>((n + DG_NT - 1) / DG_NT, 4096)), dim3(DG_NT), 0, st, s0, s1, n, out);
      HIPCHK(h, hipGetLastError());
    } else {
      HIPCHK(h, hipMemcpyAsync(out, s0, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToDevice, st));
    }
  } else {
    uint64_t* dst = (executed & 1) ? out : other;  // the last executed pass lands in out
    const uint64_t* cur = nullptr;
    for (int p = 0; p < DG_PASSES; ++p) {
      if (!(mask >> p & 1)) continue;
      rc = cur ? dg_pass<false>(h, cur, nullptr, n, p, tiles, dst) : dg_pass<PAIR>(h, s0, s1, n, p, tiles, dst);
      if (rc) return rc;
      cur = dst;
      dst = dst == out ? other : out;
    }
  }
  HIPCHK(h, hipEventRecord(h->ev[2], st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->timed = true;
  h->last_mask = mask;
  return GPRX_OK;
}
}  // namespace

extern "C" {

int gprx_dg_create(int device, gprx_dg_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  gprx_dg_handle h = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    h = new gprx_dg_ctx();
    const int rc = open_handle(h, device, h->ev, 3);
    return rc ? rc : ensure(nullptr, h->fixed, DG_FIXED_BYTES);
  });
  if (rc) gprx_dg_destroy(h);
  else *out = h;
  return rc;
}

// np.sort of n unsigned 64-bit keys: out_dev (n) <- keys_dev (n), which is left unchanged.  The buffers must not overlap.
int gprx_dg_sort_u64_dev(gprx_dg_handle h, const uint64_t* keys_dev, int64_t n, uint64_t* out_dev) {
  return guarded(h, [&]() -> int { return dg_sort<false>(h, keys_dev, nullptr, n, out_dev); });
}

// np.sort(np.abs(a - b).flatten()) (plotting.py:221-222): out_dev (n) doubles; a_dev and b_dev are left unchanged.
int gprx_dg_sort_abs_residual_dev(gprx_dg_handle h, const double* a_dev, const double* b_dev, int64_t n, double* out_dev) {
  return guarded(h, [&]() -> int { return dg_sort<true>(h, a_dev, b_dev, n, out_dev); });
}

int gprx_dg_sort_info(gprx_dg_handle h, int* executed_mask, double* ms) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (executed_mask) *executed_mask = h->last_mask;
    if (ms)
      for (int i = 0; i < 2; ++i) {
        float v = 0.f;
        if (h->timed) HIPCHK(h, hipEventElapsedTime(&v, h->ev[i], h->ev[i + 1]));
        ms[i] = v;
      }
    return GPRX_OK;
  });
}

// out[j] = sorted_dev[ranks[j]], j < m: ranks and out on the host, only m numbers cross the link each way
int gprx_dg_gather_dev(gprx_dg_handle h, const double* sorted_dev, int64_t n, const int64_t* ranks, int64_t m, double* out) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!sorted_dev || !ranks || !out) return fail(h, GPRX_EINVAL, "null argument");
    if (n < 1 || n > DG_MAX_N) return fail(h, GPRX_EINVAL, "need 1 <= n <= 2^40");
    if (m < 1 || m > ((int64_t)1 << 31)) return fail(h, GPRX_EINVAL, "need 1 <= m <= 2^31 ranks");
    for (int64_t j = 0; j < m; ++j)
      if (ranks[j] < 0 || ranks[j] >= n) return fail(h, GPRX_EINVAL, "rank " + std::to_string((long long)j) + " is outside [0, n)");
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = dg_ensure(h, h->aux, 16.0 * (double)m, "the ranks of the gather"))) return rc;
    int64_t* ranks_dev = reinterpret_cast<int64_t*>(h->aux.p);
    double* out_dev = h->aux.p + m;
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(ranks_dev, ranks, sizeof(int64_t) * (size_t)m, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dg_gather_kernel, dim3((unsigned)((m + DG_NT - 1) / DG_NT)), dim3(DG_NT), 0, st, sorted_dev, ranks_dev, m, out_dev);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, out_dev, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

// out[0] = min over both arrays, out[1] = max (plotting.py:183, 191), out[2] = sum (p - hf)^2 in the order of csrc/diag.h, out[3] = n
int gprx_dg_scatter_summary_dev(gprx_dg_handle h, const double* p_dev, const double* hf_dev, int64_t n, double* out) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!p_dev || !hf_dev || !out) return fail(h, GPRX_EINVAL, "null argument");
    if (n < 1 || n > DG_MAX_N) return fail(h, GPRX_EINVAL, "need 1 <= n <= 2^40 values");
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t chunks = (n + DG_SUM_CHUNK - 1) / DG_SUM_CHUNK;
    int rc;
    if ((rc = dg_ensure(h, h->aux, 32.0 * (double)chunks, "the chunk sums of the scatter summary"))) return rc;
    double* res = reinterpret_cast<double*>(reinterpret_cast<char*>(h->fixed.p) + DG_HIST_BYTES);
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(dg_summary_kernel, dim3((unsigned)chunks), dim3(DG_NT), 0, st, p_dev, hf_dev, n, h->aux.p);
    hipLaunchKernelGGL(dg_summary_final_kernel, dim3(1), dim3(DG_NT), 0, st, h->aux.p, chunks, res);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, res, 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    out[3] = (double)n;
    return GPRX_OK;
  });
}

// map_detection_categories (plotting.py:758-802) without the drawing: codes_dev (E, cells) bytes.  ev_lo / ev_hi: host arrays, event e
// is rows [ev_lo[e], ev_hi[e]).  *first_negative_event: the first event with a negative maximum (the reference's ValueError,
// :776-777; the codes are written all the same), -1 when there is none.
int gprx_dg_detect_dev(gprx_dg_handle h, const double* truth_dev, const double* pred_dev, int64_t rows, int64_t cells, const int64_t* ev_lo,
                       const int64_t* ev_hi, int64_t E, double thr, int include_cn, unsigned char* codes_dev, int64_t* first_negative_event) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!truth_dev || !pred_dev || !ev_lo || !ev_hi || !codes_dev || !first_negative_event) return fail(h, GPRX_EINVAL, "null argument");
    if (E < 1 || E > 65535) return fail(h, GPRX_EINVAL, "need 1 <= E <= 65535 events");
    if (rows < 1 || cells < 1 || (double)rows * (double)cells > (double)DG_MAX_N) return fail(h, GPRX_EINVAL, "need rows >= 1, cells >= 1 and rows x cells <= 2^40");
    if (std::isnan(thr)) return fail(h, GPRX_EINVAL, "the wet threshold is NaN");
    for (int64_t e = 0; e < E; ++e)
      if (ev_lo[e] < 0 || ev_lo[e] >= ev_hi[e] || ev_hi[e] > rows)
        return fail(h, GPRX_EINVAL, "event " + std::to_string((long long)e) + ": need 0 <= lo < hi <= rows");
    HIPCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = dg_ensure(h, h->aux, 16.0 * (double)E, "the event ranges"))) return rc;
    int64_t* ev_dev = reinterpret_cast<int64_t*>(h->aux.p);
    int* first = reinterpret_cast<int*>(reinterpret_cast<char*>(h->fixed.p) + DG_HIST_BYTES + 32);
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(ev_dev, ev_lo, sizeof(int64_t) * (size_t)E, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(ev_dev + E, ev_hi, sizeof(int64_t) * (size_t)E, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dg_detect_init_kernel, dim3(1), dim3(1), 0, st, first);
    hipLaunchKernelGGL(dg_detect_kernel, dim3((unsigned)((cells + DG_NT - 1) / DG_NT), (unsigned)E), dim3(DG_NT), 0, st, truth_dev, pred_dev, cells, ev_dev,
                       (int)E, thr, include_cn, codes_dev, first);
    HIPCHK(h, hipGetLastError());
    int host_first = 0;
    HIPCHK(h, hipMemcpyAsync(&host_first, first, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    *first_negative_event = host_first == 0x7fffffff ? -1 : host_first;
    return GPRX_OK;
  });
}

int gprx_dg_synchronize(gprx_dg_handle h) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  return guarded(h, [&]() -> int { HIPCHK(h, hipStreamSynchronize(h->stream)); return GPRX_OK; });
}

const char* gprx_dg_last_error(gprx_dg_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

}  // extern "C"
