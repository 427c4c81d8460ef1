// libgprx C ABI, handle-less entry points over fields: the fused error metrics (gprx_metrics*), the k-means inducing-point
// initialisation (gprx_kmeans_*) and gprx_gather_rows.  All of them run on the library's utility stream.
#include "abi_common.h"

#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "gprx_common.h"
#include "kmeans.h"
#include "metrics.h"

using namespace gprx;

extern "C" {

// ---- fused error metrics over reconstructed fields ----------------------------
int gprx_metrics_dev(int device, const double* x_dev, const double* y_dev, const double* conf_dev, int64_t rows, int64_t cells, int t_tol,
                     double v_tol, double* row_sums_dev, double* cell_sums_dev, int* cell_arg_dev, unsigned long long* matches) {
  return guarded(nullptr, [&]() -> int {
    if (!x_dev || !y_dev || !row_sums_dev || !cell_sums_dev || !cell_arg_dev || !matches) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (rows <= 0 || cells <= 0 || rows > (1 << 30)) return fail(nullptr, GPRX_EINVAL, "rows and cells must be positive");
    if (t_tol < 0 || t_tol > MET_TMAX) return fail(nullptr, GPRX_EINVAL, "t_tol must be between 0 and 8");
    HIPCHK(nullptr, hipSetDevice(device));
    const int nwg = (int)((cells + 255) / 256);
    unsigned long long* match_partial = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&match_partial, sizeof(unsigned long long) * nwg));
    MetricsArgs a{x_dev, y_dev, conf_dev, rows, cells, v_tol, t_tol, cell_sums_dev, cell_sums_dev + cells, cell_sums_dev + 2 * cells,
                  cell_sums_dev + 3 * cells, cell_sums_dev + 4 * cells, cell_arg_dev, cell_arg_dev + cells, match_partial};
    hipLaunchKernelGGL(metrics_cells_kernel, dim3(nwg), dim3(256), 0, util_stream(), a);
    hipLaunchKernelGGL(metrics_rows_kernel, dim3((unsigned)rows), dim3(256), 0, util_stream(), x_dev, y_dev, conf_dev, cells, row_sums_dev);
    std::vector<unsigned long long> hm(nwg);
    hipError_t e = copy_sync(hm.data(), match_partial, sizeof(unsigned long long) * nwg, hipMemcpyDeviceToHost);  // synchronises
    hipFree(match_partial);
    HIPCHK(nullptr, e);
    unsigned long long total = 0;
    for (auto v : hm) total += v;
    *matches = total;
    return GPRX_OK;
  });
}

int gprx_metrics(int device, const double* x, const double* y, const double* conf, int64_t rows, int64_t cells, int t_tol, double v_tol,
                 double* row_sums, double* cell_sums, int* cell_arg, unsigned long long* matches) {
  return guarded(nullptr, [&]() -> int {
    if (!x || !y || !row_sums || !cell_sums || !cell_arg || !matches) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (rows <= 0 || cells <= 0) return fail(nullptr, GPRX_EINVAL, "rows and cells must be positive");
    HIPCHK(nullptr, hipSetDevice(device));
    const size_t fb = sizeof(double) * (size_t)rows * cells;
    double *dx = nullptr, *dy = nullptr, *dc = nullptr, *drow = nullptr, *dcell = nullptr;
    int* darg = nullptr;
    DevTemps tmp(util_stream(), {(void**)&dx, (void**)&dy, (void**)&dc, (void**)&drow, (void**)&dcell, (void**)&darg});
    hipError_t e = hipMalloc((void**)&dx, fb);
    if (e == hipSuccess) e = hipMalloc((void**)&dy, fb);
    if (e == hipSuccess && conf) e = hipMalloc((void**)&dc, fb);
    if (e == hipSuccess) e = hipMalloc((void**)&drow, sizeof(double) * rows * 4);
    if (e == hipSuccess) e = hipMalloc((void**)&dcell, sizeof(double) * cells * 5);
    if (e == hipSuccess) e = hipMalloc((void**)&darg, sizeof(int) * cells * 2);
    if (e == hipSuccess) e = copy_sync(dx, x, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = copy_sync(dy, y, fb, hipMemcpyHostToDevice);
    if (e == hipSuccess && conf) e = copy_sync(dc, conf, fb, hipMemcpyHostToDevice);
    if (e != hipSuccess)
      return fail(nullptr, e == hipErrorOutOfMemory ? GPRX_ENOMEM : GPRX_EHIP, std::string("gprx_metrics staging: ") + hipGetErrorString(e));
    int rc = gprx_metrics_dev(device, dx, dy, dc, rows, cells, t_tol, v_tol, drow, dcell, darg, matches);
    if (rc == GPRX_OK) {
      e = copy_sync(row_sums, drow, sizeof(double) * rows * 4, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = copy_sync(cell_sums, dcell, sizeof(double) * cells * 5, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = copy_sync(cell_arg, darg, sizeof(int) * cells * 2, hipMemcpyDeviceToHost);
      if (e != hipSuccess) rc = fail(nullptr, GPRX_EHIP, std::string("gprx_metrics copy back: ") + hipGetErrorString(e));
    }
    return rc;
  });
}

// ---- k-means inducing-point initialisation: Lloyd iterations on the device ---------------
int gprx_kmeans_lloyd(int device, const double* x, int64_t n, int d, double* centers, int m, double tol, int max_iter, int32_t* labels,
                      int* n_iter, int* empty) {
  return guarded(nullptr, [&]() -> int {
    if (!x || !centers || !labels || !n_iter || !empty) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (n <= 0 || d <= 0 || d > 64 || m <= 0 || m > n || max_iter <= 0 || n > (1 << 30)) return fail(nullptr, GPRX_EINVAL, "need 0 < m <= n, 0 < d <= 64, max_iter > 0");
    HIPCHK(nullptr, hipSetDevice(device));
    double *dx = nullptr, *dc[2] = {nullptr, nullptr}, *dstat = nullptr;
    int* dlab = nullptr;
    DevTemps tmp(util_stream(), {(void**)&dx, (void**)&dc[0], (void**)&dc[1], (void**)&dstat, (void**)&dlab});
    const size_t cb = sizeof(double) * (size_t)m * d;
    hipError_t e = hipMalloc((void**)&dx, sizeof(double) * (size_t)n * d);
    if (e == hipSuccess) e = hipMalloc((void**)&dc[0], cb);
    if (e == hipSuccess) e = hipMalloc((void**)&dc[1], cb);
    if (e == hipSuccess) e = hipMalloc((void**)&dstat, sizeof(double) * (2 + m));
    if (e == hipSuccess) e = hipMalloc((void**)&dlab, sizeof(int) * n);
    if (e == hipSuccess) e = copy_sync(dx, x, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = copy_sync(dc[0], centers, cb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = memset_sync(dlab, 0xff, sizeof(int) * n);  // labels_old = -1 (_kmeans_single_lloyd)
    if (e != hipSuccess)
      return fail(nullptr, e == hipErrorOutOfMemory ? GPRX_ENOMEM : GPRX_EHIP, std::string("gprx_kmeans_lloyd staging: ") + hipGetErrorString(e));
    std::vector<double> stat(2 + m);
    const dim3 pgrid((unsigned)((n + 255) / 256));
    int cur = 0, it = 0;
    bool strict = false;
    *empty = 0;
    for (it = 0; it < max_iter; ++it) {
      // one iteration of lloyd_iter_chunked_dense: labels from the current centres, then the new centres and their shifts
      // the flags are cleared on the stream the two kernels run on (a non-blocking stream has no ordering with the legacy stream)
      e = hipMemsetAsync(dstat, 0, sizeof(double) * 2, util_stream());
      if (e != hipSuccess) break;
      hipLaunchKernelGGL(kmeans_assign_kernel, pgrid, dim3(256), 0, util_stream(), (const double*)dx, (int)n, d, (const double*)dc[cur], m, dlab, dstat);
      hipLaunchKernelGGL(kmeans_update_kernel, dim3(m), dim3(256), 0, util_stream(), (const double*)dx, (int)n, d, (const int*)dlab, (const double*)dc[cur],
                         dc[cur ^ 1], dstat);
      e = copy_sync(stat.data(), dstat, sizeof(double) * (2 + m), hipMemcpyDeviceToHost);  // synchronises
      if (e != hipSuccess) break;
      if (stat[1] != 0.0) {  // scikit-learn relocates empty clusters to far points; the caller falls back to it
        *empty = 1;
        break;
      }
      cur ^= 1;  // centers, centers_new = centers_new, centers
      if (stat[0] == 0.0) {  // labels equal labels_old: strict convergence
        strict = true;
        ++it;
        break;
      }
      double shift_tot = 0.0;
      for (int j = 0; j < m; ++j) shift_tot += stat[2 + j];
      if (shift_tot <= tol) {
        ++it;
        break;
      }
    }
    if (e == hipSuccess && !*empty && !strict) {
      // rerun the E-step so that the labels match the final centres
      hipLaunchKernelGGL(kmeans_assign_kernel, pgrid, dim3(256), 0, util_stream(), (const double*)dx, (int)n, d, (const double*)dc[cur], m, dlab, dstat);
    }
    if (e == hipSuccess) e = copy_sync(centers, dc[cur], cb, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = copy_sync(labels, dlab, sizeof(int) * n, hipMemcpyDeviceToHost);
    HIPCHK(nullptr, e);
    *n_iter = it > max_iter ? max_iter : it;
    return GPRX_OK;
  });
}

// k-means++ seeding on the device (kmeans.h): x (n, d) host, centred as scikit-learn centres it; xsq = row_norms(x, squared=True);
// first_id and uniforms ((m - 1) x trials) are the host's RandomState draws.  indices_out: m chosen point indices.
int gprx_kmeans_pp(int device, const double* x, int64_t n, int d, const double* xsq, int m, int trials, int64_t first_id, const double* uniforms,
                   int64_t* indices_out) {
  return guarded(nullptr, [&]() -> int {
    if (!x || !xsq || !indices_out || (m > 1 && !uniforms)) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (n <= 0 || d <= 0 || d > 64 || m <= 0 || m > n || trials <= 0 || trials > KPP_MAX_TRIALS || first_id < 0 || first_id >= n || n > (1 << 30))
      return fail(nullptr, GPRX_EINVAL, "need 0 < m <= n, 0 < d <= 64, 0 < trials <= 16, 0 <= first_id < n");
    HIPCHK(nullptr, hipSetDevice(device));
    hipStream_t us = util_stream();
    if (!us) return fail(nullptr, GPRX_EHIP, "no utility stream");
    const int nblocks = (int)((n + 255) / 256);
    double *dx = nullptr, *dsq = nullptr, *dbuf = nullptr, *dpart = nullptr, *duni = nullptr;
    KppState* dst = nullptr;
    long long* didx = nullptr;
    DevTemps tmp(util_stream(), {(void**)&dx, (void**)&dsq, (void**)&dbuf, (void**)&dpart, (void**)&duni, (void**)&dst, (void**)&didx});
    const size_t slab = sizeof(double) * (size_t)trials * n;  // one generation of candidate distance arrays
    hipError_t e = hipMalloc((void**)&dx, sizeof(double) * (size_t)n * d);
    if (e == hipSuccess) e = hipMalloc((void**)&dsq, sizeof(double) * n);
    if (e == hipSuccess) e = hipMalloc((void**)&dbuf, 2 * slab);
    if (e == hipSuccess) e = hipMalloc((void**)&dpart, sizeof(double) * (size_t)trials * nblocks);
    if (e == hipSuccess) e = hipMalloc((void**)&duni, sizeof(double) * (size_t)std::max(1, (m - 1) * trials));
    if (e == hipSuccess) e = hipMalloc((void**)&dst, 2 * sizeof(KppState));
    if (e == hipSuccess) e = hipMalloc((void**)&didx, sizeof(long long) * m);
    if (e == hipSuccess) e = hipMemcpyAsync(dx, x, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, us);
    if (e == hipSuccess) e = hipMemcpyAsync(dsq, xsq, sizeof(double) * n, hipMemcpyHostToDevice, us);
    if (e == hipSuccess && m > 1) e = hipMemcpyAsync(duni, uniforms, sizeof(double) * (size_t)(m - 1) * trials, hipMemcpyHostToDevice, us);
    if (e != hipSuccess)
      return fail(nullptr, e == hipErrorOutOfMemory ? GPRX_ENOMEM : GPRX_EHIP, std::string("gprx_kmeans_pp staging: ") + hipGetErrorString(e));
    double* gen[2] = {dbuf, dbuf + (size_t)trials * n};
    // distances to the first centre: generation 0, one "candidate"
    hipLaunchKernelGGL(kpp_dist_kernel, dim3(nblocks, 1), dim3(256), 0, us, (const double*)dx, (int)n, d, (const double*)dsq, (const KppState*)nullptr,
                       (const double*)nullptr, (int)first_id, gen[0], dpart, nblocks);
    int cur = 0, prev_trials = 1;
    for (int c = 1; c <= m; ++c) {
      // choose among the candidates of centre c - 1 (c == 1: the first centre itself); c < m: candidates of centre c
      const bool more = c < m;
      hipLaunchKernelGGL(kpp_select_kernel, dim3(1), dim3(256), 0, us, (int)n, (const double*)gen[cur], (const double*)dpart, nblocks, prev_trials,
                         c == 1 ? (const KppState*)nullptr : (const KppState*)(dst + ((c - 1) & 1)), (int)first_id, dst + (c & 1),
                         more ? (const double*)(duni + (size_t)(c - 1) * trials) : (const double*)nullptr, trials, didx + (c - 1));
      if (!more) break;
      hipLaunchKernelGGL(kpp_dist_kernel, dim3(nblocks, trials), dim3(256), 0, us, (const double*)dx, (int)n, d, (const double*)dsq,
                         (const KppState*)(dst + (c & 1)), (const double*)gen[cur], (int)first_id, gen[cur ^ 1], dpart, nblocks);
      cur ^= 1;
      prev_trials = trials;
    }
    std::vector<long long> idx(m);
    e = hipMemcpyAsync(idx.data(), didx, sizeof(long long) * m, hipMemcpyDeviceToHost, us);
    hipError_t e2 = hipStreamSynchronize(us);
    HIPCHK(nullptr, e);
    HIPCHK(nullptr, e2);
    for (int c = 0; c < m; ++c) indices_out[c] = idx[c];
    return GPRX_OK;
  });
}

int gprx_gather_rows(int device, const double* field_dev, int64_t rows, int64_t cells, const int64_t* idx, double* out) {
  return guarded(nullptr, [&]() -> int {
    if (!field_dev || !idx || !out) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (rows <= 0 || cells <= 0) return fail(nullptr, GPRX_EINVAL, "rows and cells must be positive");
    std::vector<int64_t> wrapped(idx, idx + cells);
    for (int64_t c = 0; c < cells; ++c) {
      if (wrapped[c] < -rows || wrapped[c] >= rows) {
        char msg[160];
        snprintf(msg, sizeof msg, "index %lld is out of bounds for axis 0 with size %lld", (long long)idx[c], (long long)rows);
        return fail(nullptr, GPRX_EINVAL, msg);
      }
      if (wrapped[c] < 0) wrapped[c] += rows;
    }
    HIPCHK(nullptr, hipSetDevice(device));
    int64_t* didx = nullptr;
    double* dout = nullptr;
    DevTemps tmp(util_stream(), {(void**)&didx, (void**)&dout});
    hipError_t e = hipMalloc((void**)&didx, sizeof(int64_t) * cells);
    if (e == hipSuccess) e = hipMalloc((void**)&dout, sizeof(double) * cells);
    if (e == hipSuccess) e = copy_sync(didx, wrapped.data(), sizeof(int64_t) * cells, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, util_stream(), field_dev, cells, (const int64_t*)didx, dout);
      e = copy_sync(out, dout, sizeof(double) * cells, hipMemcpyDeviceToHost);  // synchronises
    }
    HIPCHK(nullptr, e);
    return GPRX_OK;
  });
}

}  // extern "C"
