// libgprx C ABI, per-event temporal clipping (gprx_al_*): DataBuilder.get_cutoff and the row slices of _align_datasets.
#include "abi_common.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "align.h"
#include "gprx_common.h"

using namespace gprx;

extern "C" {

// ---- temporal clipping (gpras/preprocess.py:89-155) ---------------------------------------------------------
struct gprx_al_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  Buf ws, up;             // the workspace of a cutoff call; the uploaded matrix of gprx_al_cutoff
  hipEvent_t ev[5] = {};  // around the four stages of the last cutoff call
  bool timed = false;
  std::string err;
};

int gprx_al_destroy(gprx_al_handle h) {
  if (!h) return GPRX_OK;
  release_handle(h->device, h->stream, {h->ws.p, h->up.p}, h->ev, 5);
  delete h;
  return GPRX_OK;
}

int gprx_al_create(int device, gprx_al_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  gprx_al_handle h = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    h = new gprx_al_ctx();
    return open_handle(h, device, h->ev, 5);
  });
  if (rc) gprx_al_destroy(h);
  else *out = h;
  return rc;
}

namespace {
constexpr int64_t AL_MAX = ((int64_t)1 << 31) - 1024;  // rows and columns: the first NaN row is a 32-bit integer on the device

// the arguments of a cutoff call, judged without the device (and before the handle, so that a host without one can test them)
int al_check(gprx_al_handle h, int n_blocks, const double* const* blocks, const int64_t* cols, const int64_t* ld, int64_t rows, double threshold,
             int64_t* start, int64_t* stop, int64_t* total_cols) {
  if (n_blocks < 1 || n_blocks > AL_MAX_BLOCKS) return fail(h, GPRX_EINVAL, "n_blocks must be 1 to 4");
  if (!blocks || !cols || !ld || !start || !stop) return fail(h, GPRX_EINVAL, "null argument");
  int64_t C = 0;
  for (int b = 0; b < n_blocks; ++b) {
    const std::string which = "block " + std::to_string(b) + ": ";
    if (!blocks[b]) return fail(h, GPRX_EINVAL, which + "null pointer");
    if (cols[b] < 1) return fail(h, GPRX_EINVAL, which + "cols must be at least 1");
    if (ld[b] < cols[b]) return fail(h, GPRX_EINVAL, which + "ld is smaller than cols");
    C += cols[b];
    if (C > AL_MAX) return fail(h, GPRX_EINVAL, "need fewer than 2^31 - 1024 columns in all");
  }
  if (rows < 1 || rows > AL_MAX) return fail(h, GPRX_EINVAL, "need 1 <= rows < 2^31 - 1024");
  if (!std::isfinite(threshold)) return fail(h, GPRX_EINVAL, "the threshold is not finite");
  if (rows < 2) return fail(h, GPRX_EINVAL, "fewer than 2 rows: no difference row to judge (the reference raises ValueError from argmax)");
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  *total_cols = C;
  return GPRX_OK;
}
}  // namespace

// DataBuilder.get_cutoff (:135-147) with _delta_cols_norm (:149-155) over device blocks.
int gprx_al_cutoff_dev(gprx_al_handle h, int n_blocks, const double* const* blocks_dev, const int64_t* cols, const int64_t* ld, int64_t rows,
                       double threshold, int64_t* start, int64_t* stop, int64_t* rows_used, double* curve) {
  return guarded(h, [&]() -> int {
    int64_t C = 0;
    int rc;
    if ((rc = al_check(h, n_blocks, blocks_dev, cols, ld, rows, threshold, start, stop, &C))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t strips = (C + AL_NT - 1) / AL_NT, pitch = rows - 1;
    // doubles: 4 of integers (start, stop, T', first NaN row) | n_c (C) | strip sums (strips, pitch) | r (pitch) | curve (pitch)
    const double want = 8.0 * (4.0 + (double)C + (double)strips * (double)pitch + 2.0 * (double)pitch);
    if ((rc = ensure(h, h->ws, (size_t)want, "the workspace of the cutoff"))) return rc;
    int64_t* res = reinterpret_cast<int64_t*>(h->ws.p);
    int* first = reinterpret_cast<int*>(res + 3);
    double *nrm = h->ws.p + 4, *part = nrm + C, *r = part + strips * pitch, *cum = r + pitch;
    AlBlocks B{};
    for (int b = 0; b <= AL_MAX_BLOCKS; ++b) B.c0[b] = C;
    for (int64_t b = 0, c = 0; b < n_blocks; c += cols[b], ++b) {
      B.p[b] = blocks_dev[b];
      B.ld[b] = ld[b];
      B.c0[b] = c;
    }
    B.rows = rows;
    hipStream_t st = h->stream;
    const dim3 scan_grid((unsigned)strips, (unsigned)std::min<int64_t>((rows + AL_RT - 1) / AL_RT, 65535));
    const dim3 sum_grid((unsigned)strips, (unsigned)std::min<int64_t>((pitch + AL_RT - 1) / AL_RT, 65535));
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(al_init_kernel, dim3(1), dim3(1), 0, st, first, (int)rows);
    hipLaunchKernelGGL(al_scan_kernel, scan_grid, dim3(AL_NT), 0, st, B, first);
    HIPCHK(h, hipEventRecord(h->ev[1], st));
    hipLaunchKernelGGL(al_norm_kernel, dim3((unsigned)strips), dim3(AL_NT), 0, st, B, first, nrm);
    HIPCHK(h, hipEventRecord(h->ev[2], st));
    hipLaunchKernelGGL(al_rowsum_kernel, sum_grid, dim3(AL_NT), 0, st, B, first, nrm, part, pitch);
    hipLaunchKernelGGL(al_combine_kernel, dim3((unsigned)((pitch + AL_NT - 1) / AL_NT)), dim3(AL_NT), 0, st, first, part, pitch, strips, r);
    HIPCHK(h, hipEventRecord(h->ev[3], st));
    hipLaunchKernelGGL(al_finish_kernel, dim3(1), dim3(AL_NT), 0, st, first, r, threshold, cum, res);
    HIPCHK(h, hipEventRecord(h->ev[4], st));
    HIPCHK(h, hipGetLastError());
    h->timed = true;
    int64_t host[3] = {0, 0, 0};
    HIPCHK(h, hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    if (rows_used) *rows_used = host[2];
    if (host[2] < 2)
      return fail(h, GPRX_EINVAL, "fewer than 2 rows are left after the NaN trim: the first NaN is in row " + std::to_string((long long)host[2]));
    *start = host[0];
    *stop = host[1];
    if (curve) {
      HIPCHK(h, hipMemcpyAsync(curve, cum, sizeof(double) * (size_t)(host[2] - 1), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipStreamSynchronize(st));
    }
    return GPRX_OK;
  });
}

// The same from one host matrix x (rows, cols): uploaded, then one device block.
int gprx_al_cutoff(gprx_al_handle h, const double* x, int64_t rows, int64_t cols, double threshold, int64_t* start, int64_t* stop,
                   int64_t* rows_used, double* curve) {
  return guarded(h, [&]() -> int {
    int64_t C = 0;
    int rc;
    const int64_t ld = cols;
    if ((rc = al_check(h, 1, &x, &cols, &ld, rows, threshold, start, stop, &C))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    // the size in double first: rows x cols of the allowed ranges can exceed what a size_t holds, and must end as GPRX_ENOMEM
    const double want = 8.0 * (double)rows * (double)cols;
    if (want > (double)h->up.bytes && (rc = need_device_bytes(h, want, "the uploaded matrix of the cutoff"))) return rc;
    const size_t bytes = sizeof(double) * (size_t)rows * (size_t)cols;
    if ((rc = ensure(h, h->up, bytes, "the uploaded matrix of the cutoff"))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->up.p, x, bytes, hipMemcpyHostToDevice, h->stream));
    const double* dev = h->up.p;
    return gprx_al_cutoff_dev(h, 1, &dev, &cols, &ld, rows, threshold, start, stop, rows_used, curve);
  });
}

// Rows [start, stop) of one block (_align_datasets, :110-112; aligned_ref_line_df, :132) into a destination with its own pitch.
int gprx_al_clip_dev(gprx_al_handle h, const double* src_dev, int64_t lds, int64_t cols, int64_t start, int64_t stop, double* dst_dev, int64_t ldd) {
  return guarded(h, [&]() -> int {
    if (cols < 1 || cols > AL_MAX) return fail(h, GPRX_EINVAL, "need 1 <= cols < 2^31 - 1024");
    if (lds < cols) return fail(h, GPRX_EINVAL, "lds is smaller than cols");
    if (ldd < cols || ldd > AL_MAX) return fail(h, GPRX_EINVAL, "ldd is smaller than cols (or not below 2^31 - 1024)");
    if (start < 0 || stop < 0 || stop > AL_MAX) return fail(h, GPRX_EINVAL, "need 0 <= start and 0 <= stop < 2^31 - 1024");
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (stop <= start) return GPRX_OK;  // an empty slice, as in numpy
    if (!src_dev || !dst_dev) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t n = stop - start;
    const dim3 grid((unsigned)((ldd + AL_NT - 1) / AL_NT), (unsigned)std::min<int64_t>((n + 7) / 8, 65535));
    hipLaunchKernelGGL(al_clip_kernel, grid, dim3(AL_NT), 0, h->stream, src_dev, lds, cols, start, n, dst_dev, ldd);
    HIPCHK(h, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_al_timings(gprx_al_handle h, double* ms) {
  return guarded(h, [&]() -> int {
    if (!h || !ms) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < 4; ++i) {
      float v = 0.f;
      if (h->timed) HIPCHK(h, hipEventElapsedTime(&v, h->ev[i], h->ev[i + 1]));
      ms[i] = v;
    }
    return GPRX_OK;
  });
}

int gprx_al_synchronize(gprx_al_handle h) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  return guarded(h, [&]() -> int { HIPCHK(h, hipStreamSynchronize(h->stream)); return GPRX_OK; });
}

const char* gprx_al_last_error(gprx_al_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

}  // extern "C"
