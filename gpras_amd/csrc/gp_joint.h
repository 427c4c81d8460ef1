// GP path: the JOINT predictive distribution of a batch of sparse models over one event's test points -- the mean of the batched
// predict and the lower Cholesky factor of the predictive covariance with the diagonal kept joint (oracle/sgpr.py:187-197):
//   C = Kss - tmp1^T tmp1 + tmp2^T tmp2 (+ noise I, or + JITTER variance I without the noise),  tmp1 = L^-1 Kus,  tmp2 = LB^-1 tmp1.
// After gp_predict.h.  The mean equals gprx_predict_batch_dev's bit for bit (a tested equality).  The launches are those of
// sgpr_predict_batch on one tile for all ns columns at once, with tmp1 copied beside tmp2 in the cell's Kus tile (columns [JOINT_T1_COL, ...) of its SGPR_PRED_TILE: ns <= 1024 leaves room), launch_kmat in its symmetric mode for Kss,
// two (1, 0) GEMMs with beta = 1 and the batched Cholesky by the route its pickers take for (Tp, count).  New kernels: the diagonal
// term and the copy of the factor's lower triangle into the caller's (count, Tp, Tp) block.
#pragma once

namespace gprx {
// C[c][i, i] += include_noise ? noise_c : jitter * variance_c  for i < ns (row c of the cell-parameter table: [0] variance, [1] noise)
__global__ __launch_bounds__(256) void joint_diag_kernel(double* __restrict__ C, int64_t ld, int64_t cs, int ns, const double* __restrict__ cell_par,
                                                         int include_noise, double jitter) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  const double* par = cell_par + (int64_t)blockIdx.y * CELL_PAR;
  double* cp = C + (int64_t)blockIdx.y * cs + (int64_t)i * ld + i;
  const double add = include_noise ? par[1] : jitter * par[0];
  *cp = *cp + add;
}
// Lc[c] (tp, tp) <- the lower triangle of the factorised C[c] (leading dimension ld, cells cs apart), zeros above the diagonal
__global__ __launch_bounds__(256) void joint_tril_kernel(const double* __restrict__ C, int64_t ld, int64_t cs, int tp, double* __restrict__ Lc) {
  const int64_t total = (int64_t)tp * tp;
  const double* src = C + (int64_t)blockIdx.y * cs;
  double* dst = Lc + (int64_t)blockIdx.y * total;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t i = e / tp, j = e - i * tp;
    dst[e] = j <= i ? src[i * ld + j] : 0.0;
  }
}
}  // namespace gprx

namespace {
constexpr int JOINT_MAX_NS = 1024;
constexpr int JOINT_T1_COL = SGPR_PRED_TILE / 2;  // tmp1's copy starts at this column of the cell's Kus tile

int predict_joint_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                        double* means_dev, double* lc_dev, int include_noise) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !thetas || !xs_dev || !means_dev || !lc_dev) return fail(h, GPRX_EINVAL, "null argument");
  if (h->m == 0) return fail(h, GPRX_EINVAL, "gprx_predict_joint_batch_dev: exact model (the joint prediction serves sparse models)");
  if (h->mp > LOEO_BLOCKED_MAX_MP) return fail(h, GPRX_EINVAL, "gprx_predict_joint_batch_dev: more than 320 inducing points");
  if (h->d > CELL_PAR - CELL_PAR_LS) return fail(h, GPRX_EINVAL, "gprx_predict_joint_batch_dev: d > 64");
  if (ns < 1 || ns > JOINT_MAX_NS) return fail(h, GPRX_EINVAL, "gprx_predict_joint_batch_dev: an event has between 1 and 1024 test points");
  if (!z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
  hipStream_t st = h->stream;
  // the batched factorisation of the cells, as gprx_predict_batch_dev runs it (ENOTPD included)
  std::vector<Theta> ts;
  if ((rc = decode_cells(h, count, units, thetas, z, ts))) return rc;
  std::vector<double> elbo(count);
  std::vector<int> stv(count);
  if ((rc = sgpr_objective_batch(h, count, units, ts.data(), z, elbo.data(), nullptr, nullptr, stv.data()))) return rc;
  const SgprLayout L = sgpr_batch_layout(h);
  const int mp = (int)h->mp, m = (int)h->m, tile = SGPR_PRED_TILE;
  const int nsi = (int)ns, tp = (int)round_up(ns, NB);
  const int64_t ss = L.ss;
  double* A0 = h->sarena.p;
  const SgprParSrc ps = sgpr_par_src(h, h->variance, h->noise);
  const double* cpar = ps.table;
  // workspace, one block per cell: C (tp, tp) | inverse diagonal blocks | staged diagonal blocks | info
  const int64_t oInvD = (int64_t)tp * tp, oStage = oInvD + (int64_t)tp * NB, oInfo = oStage + round_up((int64_t)tp * STAGE_LD, 2);
  const int64_t cs = round_up(oInfo + 2, 64);
  if ((rc = ensure(h, h->joint_ws, sizeof(double) * (size_t)cs * count, "gprx_predict_joint_batch_dev workspace"))) return rc;
  double* W0 = h->joint_ws.p;
  int* info0 = reinterpret_cast<int*>(W0 + oInfo);
  HIPCHK(h, hipMemset2DAsync(W0 + oInfo, sizeof(double) * cs, 0, 2 * sizeof(double), count, st));
  // the head of sgpr_predict_batch for all ns columns: Kus, tmp1 = L^-1 Kus (copied aside), tmp2 = LB^-1 tmp1, mean = tmp2^T c
  const int rows_per_chunk = 256;
  const int nchunks = (mp + rows_per_chunk - 1) / rows_per_chunk;
  const double* cvec = A0 + L.oBm + (int64_t)mp * mp;
  double* T2 = A0 + L.oKs;
  double* T1 = T2 + JOINT_T1_COL;
  KmatArgs ka{A0 + L.oZ, xs_dev, nullptr, T2, tile, m, nsi, h->d, mp, tp, 0.0, 0.0, 0, 0.0, nullptr, 0};
  ps.stamp(ka);
  ka.out_stride = ss;
  ka.a_stride = ss;
  ka.diag_const = 1;
  HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h), count));
  HIPCHK(h, trsm_lower_left(st, A0 + L.oQm, mp, A0 + L.oInvDL, T2, tile, mp, tp, count, ss));
  for (int c = 0; c < count; ++c)
    HIPCHK(h, hipMemcpy2DAsync(T1 + (int64_t)c * ss, sizeof(double) * tile, T2 + (int64_t)c * ss, sizeof(double) * tile, sizeof(double) * tp, (size_t)mp,
                               hipMemcpyDeviceToDevice, st));
  HIPCHK(h, trsm_lower_left(st, A0 + L.oBm, mp, A0 + L.oInvDB, T2, tile, mp, tp, count, ss));
  const dim3 pgrid((nsi + 255) / 256, nchunks, count), fgrid((nsi + 255) / 256, count);
  hipLaunchKernelGGL(colreduce_partial, pgrid, dim3(256), 0, st, (const double*)T2, (int64_t)tile, cvec, mp, nsi, rows_per_chunk, A0 + L.oPred, ss, ss, ss);
  hipLaunchKernelGGL(colreduce_final, fgrid, dim3(256), 0, st, (const double*)(A0 + L.oPred), nchunks, nsi, 0.0, 1.0, 0, means_dev, ss, ns);
  HIPCHK(h, hipGetLastError());
  // C = Kss (identity on the padding) + the diagonal term - tmp1^T tmp1 + tmp2^T tmp2, lower tiles only
  KmatArgs ks{xs_dev, xs_dev, nullptr, W0, tp, nsi, nsi, h->d, tp, tp, 0.0, 0.0, 1, 1.0, nullptr, 0};
  ps.stamp(ks);
  ks.out_stride = cs;
  ks.diag_const = 1;
  HIPCHK(h, launch_kmat(st, h->kid, with_form(ks, h), count));
  hipLaunchKernelGGL(joint_diag_kernel, dim3((nsi + 255) / 256, count), dim3(256), 0, st, W0, (int64_t)tp, cs, nsi, cpar, include_noise ? 1 : 0, JITTER);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, launch_gemm(st, 1, 0, tp, tp, mp, -1.0, T1, tile, T1, tile, 1.0, W0, tp, GEMM_C_LOWER, 64, 1, 0, 0, 0, count, ss, ss, cs));
  HIPCHK(h, launch_gemm(st, 1, 0, tp, tp, mp, 1.0, T2, tile, T2, tile, 1.0, W0, tp, GEMM_C_LOWER, 64, 1, 0, 0, 0, count, ss, ss, cs));
  // the batched Cholesky by the route the pickers of the exact path take for this size and count
  if (use_cell_kernel(h->tune, tp, count))
    HIPCHK(h, potrf_cells(st, W0, tp, tp, 0, W0 + oInvD, info0, count, cs, (int)(2 * cs)));
  else
    HIPCHK(h, potrf_lower(st, W0, tp, tp, 0, W0 + oInvD, info0, W0 + oStage, nullptr, nullptr, count, cs, (int)(2 * cs), &h->tune));
  hipLaunchKernelGGL(joint_tril_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)tp * tp + 255) / 256, 1024), count), dim3(256), 0, st, (const double*)W0,
                     (int64_t)tp, cs, tp, lc_dev);
  HIPCHK(h, hipGetLastError());
  std::vector<int> info((size_t)count * 2);
  HIPCHK(h, hipMemcpy2DAsync(info.data(), 2 * sizeof(int), info0, sizeof(double) * cs, 2 * sizeof(int), count, hipMemcpyDeviceToHost, st));
  HIPCHK(h, wait_stream(h, st));
  for (int c = 0; c < count; ++c)
    if (info[(size_t)c * 2]) {
      char msg[160];
      snprintf(msg, sizeof msg, "cell %d: the joint predictive covariance is not positive definite: pivot %d", c, info[(size_t)c * 2]);
      return fail(h, GPRX_ENOTPD, msg);
    }
  return GPRX_OK;
}
}  // namespace
