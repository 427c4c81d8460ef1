// GP path, part 6 of 6: prediction -- one exact model through L^-1 or by forward substitution, a batch of exact slots, the batched
// sparse predict behind its factorisation, and the slab loop of the host-buffer entry points.  After gp_objective.h.
#pragma once

namespace {
constexpr int PRED_TILE = 8192;
// test points per pass of ONE exact model's predict: the N x tile blocks Ks and V = L^-1 Ks stay at the 268 MB each they have at N = 4096,
// so a small model takes more points per pass (N = 1024: 13 passes of 7 692 points with four launches each spent 21 % of the predict outside
// the product; per-point results do not depend on the pass they fall into)
int pred_tile_for(int64_t np) { return np <= 1024 ? 4 * PRED_TILE : (np <= 2048 ? 2 * PRED_TILE : PRED_TILE); }

// what one exact factorisation contributes to a prediction through the explicit inverse: alpha, L^-1, the kernel's
// hyperparameters (a device lengthscale vector, or a row of the cell-parameter table) and the variance offset
struct ExactPredictSrc {
  const double* alpha;
  const double* Xinv;
  const double* ls_dev;
  const double* cell_par;  // row of the batch's cell-parameter table ([0] variance, [8..] lengthscales) or nullptr
  double variance, base;   // base = variance (+ noise for predict_y)
};

// transposed formulation, test points along the rows: Kst = k(Xs, X) (ts x np), mean = Kst alpha (row dots),
// Vt = Kst L^-T as an NT GEMM -- both operands k-contiguous, the GEMM kernel's fastest case; op(B) = L^-T is
// upper triangular, so the K range of a tile ends at its last column and every tile row mixes short and long
// tiles (no tail of long tiles) -- and var = base - row sums of Vt^2.  h->Ks holds 2 x np x tile doubles.
int exact_predict_inverse(gprx_handle h, const ExactPredictSrc& src, const double* xs_dev, int64_t ns, double* mean_dev, double* var_dev,
                                 int tile) {
  const int np = (int)h->np;
  const int64_t ld = h->np;
  hipStream_t st = h->stream;
  double* Vbuf = h->Ks.p + (size_t)h->np * tile;
  for (int64_t t0 = 0; t0 < ns; t0 += tile) {
    const int ts = (int)std::min<int64_t>(tile, ns - t0);
    const int tsp = (int)round_up(ts, NB);
    KmatArgs ka{xs_dev + t0 * h->d, h->X.p, src.ls_dev, h->Ks.p, ld, ts, (int)h->n, h->d, tsp, np, src.variance, 0.0, 0, 0.0, nullptr, 0};
    if (src.cell_par) {  // hyperparameters of a batch slot: straight from the device table (no upload, no synchronisation)
      ka.cell_par = src.cell_par;
      ka.diag_const = 1;
    }
    HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h)));
    hipLaunchKernelGGL(rowreduce_kernel, dim3((ts + 3) / 4), dim3(256), 0, st, (const double*)h->Ks.p, ld, src.alpha, ts, np, 0.0, 1.0, mean_dev + t0);
    // Vt is never stored: the GEMM's epilogue leaves the row sums of squares of its tiles (2 slabs per tile column), which
    // the final kernel adds in a fixed order -- 2 x 8 np tile bytes less HBM traffic per tile than storing and re-reading Vt
    // 64 x 64 tiles: operands by LDS-DMA and finer clipping of the triangular K range (measured at N = 4096, 100 000 points:
    // 3.65 M points/s = 61.2 TFLOP/s against 3.35 M with the 128 x 128 register-staged kernel)
    static const int ptile = env_int("GPRX_PREDICT_TILE", 64);
    const int nparts = 2 * ((np + ptile - 1) / ptile);
    HIPCHK(h, launch_gemm(st, 0, 1, tsp, np, np, 1.0, h->Ks.p, ld, src.Xinv, ld, 0.0, Vbuf, ld, GEMM_B_UPPER, ptile, 1, 0, 0, 0, 1, 0, 0, 0, nullptr, 0,
                          Vbuf, (int64_t)tile));
    hipLaunchKernelGGL(rowsq_final_kernel, dim3((ts + 255) / 256), dim3(256), 0, st, (const double*)Vbuf, nparts, (int64_t)tile, ts, src.base, var_dev + t0);
  }
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

int predict_dev(gprx_handle h, const double* xs_dev, int64_t ns, double* mean_dev, double* var_dev, int include_noise) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!h->factorized) return fail(h, GPRX_ESTATE, "gprx_predict before a successful gprx_factorize / gprx_objective");
  if (ns < 0 || (ns > 0 && (!xs_dev || !mean_dev || !var_dev))) return fail(h, GPRX_EINVAL, "null argument");
  hipStream_t st = h->stream;
  const int rows_per_chunk = 256;
  if (h->m != 0) return sgpr_predict_batch(h, 1, xs_dev, ns, mean_dev, var_dev, include_noise);  // cell block 0
  const int np = (int)h->np;
  const int64_t ld = h->np;
  const int tile = (int)std::min<int64_t>(pred_tile_for(h->np), round_up(ns, NB));
  // Many test points: V = L^-1 Ks as ONE triangular GEMM per tile against the explicit inverse (computed once
  // per factorisation, N^3/3 flops amortised over N* >= 2 N points) instead of the recursive solve's ~2 N/64
  // dependent launches per tile.  Few points: blocked forward substitution on L itself.
  // Measured at N = 4096 (tools/predict_sizes.py): the substitution path costs ~1.7 ms whatever the batch (2 N / 64
  // dependent launches), the inverse path 0.9 ms for L^-1 plus 0.3 us per point -- faster for every batch size; at larger
  // N the N^3 / 3 flops of L^-1 only pay from about N / 2 points on.  predict_path (gprx_set_tuning): 1 / 2 force a path.
  const int forced = h->predict_path;
  const bool use_inverse = forced == 1 || (forced != 2 && (h->have_linv || h->n <= 4096 || 2 * ns >= (int64_t)h->n));
  if ((rc = ensure(h, h->Ks, sizeof(double) * h->np * tile * (use_inverse ? 2 : 1)))) return rc;
  double* Vbuf = h->Ks.p + (use_inverse ? (size_t)h->np * tile : 0);
  if (use_inverse && !h->have_linv) {
    if ((rc = ensure(h, h->Xinv, sizeof(double) * h->np * ld))) return rc;
    if ((rc = ensure(h, h->Tmp, sizeof(double) * h->np * ld))) return rc;
    HIPCHK(h, hipMemsetAsync(h->Xinv.p, 0, sizeof(double) * h->np * ld, st));
    HIPCHK(h, trtri_lower(st, h->Kmat.p, ld, h->invD.p, h->Xinv.p, ld, h->Tmp.p, ld, np));
    h->have_linv = true;
  }
  const double base = h->variance + (include_noise ? h->noise : 0.0);
  if (use_inverse) {
    const ExactPredictSrc src{h->alpha.p, h->Xinv.p, h->invls.p, nullptr, h->variance, base};
    return exact_predict_inverse(h, src, xs_dev, ns, mean_dev, var_dev, tile);
  }
  const int nchunks = (np + rows_per_chunk - 1) / rows_per_chunk;
  if ((rc = ensure(h, h->pred, sizeof(double) * (size_t)nchunks * tile))) return rc;
  for (int64_t t0 = 0; t0 < ns; t0 += tile) {
    const int ts = (int)std::min<int64_t>(tile, ns - t0);
    const int tsp = (int)round_up(ts, NB);
    KmatArgs ka{h->X.p, xs_dev + t0 * h->d, h->invls.p, h->Ks.p, tile, (int)h->n, ts, h->d, np, tsp, h->variance, 0.0, 0, 0.0, nullptr, 0};
    HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h)));
    dim3 grid((ts + 255) / 256, nchunks);
    hipLaunchKernelGGL(colreduce_partial, grid, dim3(256), 0, st, h->Ks.p, (int64_t)tile, h->alpha.p, np, ts, rows_per_chunk, h->pred.p);
    hipLaunchKernelGGL(colreduce_final, dim3((ts + 255) / 256), dim3(256), 0, st, h->pred.p, nchunks, ts, 0.0, 1.0, 0, mean_dev + t0);
    HIPCHK(h, trsm_lower_left(st, h->Kmat.p, ld, h->invD.p, h->Ks.p, tile, np, tsp));
    hipLaunchKernelGGL(colreduce_partial, grid, dim3(256), 0, st, (const double*)h->Ks.p, (int64_t)tile, (const double*)nullptr, np, ts, rows_per_chunk,
                       h->pred.p);
    hipLaunchKernelGGL(colreduce_final, dim3((ts + 255) / 256), dim3(256), 0, st, h->pred.p, nchunks, ts, base, -1.0, 0, var_dev + t0);
  }
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

// Core of gprx_predict_batch: the test points are in device memory (xs_dev) and the results go to device memory
// (means_dev / vars_dev: (count, ns) row-major); asynchronous on the handle's stream after the batched factorisation.
// holds (gprx_predict_batch_held, checked by the caller): cell i is factorised without its held-out rows; the predict itself reads the
// cell's factors only and is the one of every other batch (a lone held cell takes the batched branch too).
int predict_batch_core(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                              double* means_dev, double* vars_dev, int include_noise, const CellHolds& holds = CellHolds{}) {
  int rc;
  hipStream_t st = h->stream;
  if (h->m == 0 && h->d <= CELL_PAR - CELL_PAR_LS) {
    // exact models: all factorisations by one batched launch sequence, then every slot predicts
    if ((rc = factorize_batch(h, count, units, thetas, 0, nullptr, nullptr))) return rc;
    if (ns == 0) return GPRX_OK;
    const bool use_inverse = h->predict_path != 2 && (h->n <= 4096 || 2 * ns >= (int64_t)h->n);
    if (!use_inverse) {
      for (int i = 0; i < count; ++i) {
        if ((rc = select_slot(h, i))) return rc;
        if ((rc = predict_dev(h, xs_dev, ns, means_dev + (int64_t)i * ns, vars_dev + (int64_t)i * ns, include_noise))) return rc;
      }
      return GPRX_OK;
    }
    // L^-1 of every slot by batched launches (trtri_lower with the cell index in its grids); each slot then predicts with
    // its alpha / L^-1 / row of the parameter table -- no per-cell upload or synchronisation
    const int np = (int)h->np;
    const int64_t ld = h->np, cs = h->cell_stride, gs = 2 * (int64_t)h->np * h->np;
    const int tile = (int)std::min<int64_t>(PRED_TILE, round_up(ns, NB));
    if ((rc = ensure(h, h->garena, sizeof(double) * (size_t)gs * count))) return rc;
    if ((rc = ensure(h, h->Ks, sizeof(double) * h->np * tile * 2))) return rc;
    for (int c = 0; c < count; ++c) HIPCHK(h, hipMemsetAsync(h->garena.p + (int64_t)c * gs, 0, sizeof(double) * h->np * ld, st));
    HIPCHK(h, trtri_lower(st, h->arena.p, ld, h->arena.p + h->off_invd, h->garena.p, ld, h->garena.p + (int64_t)np * ld, ld, np, count, cs, gs,
                          h->tune.update_tile ? h->tune.update_tile : 64));
    for (int i = 0; i < count; ++i) {
      const Theta& t = h->slot_theta[i];
      const double* cpar = h->cellpar.p + (int64_t)i * CELL_PAR;
      const ExactPredictSrc src{h->arena.p + (int64_t)i * cs + h->off_alpha, h->garena.p + (int64_t)i * gs, nullptr, cpar, t.variance,
                                t.variance + (include_noise ? t.noise : 0.0)};
      if ((rc = exact_predict_inverse(h, src, xs_dev, ns, means_dev + (int64_t)i * ns, vars_dev + (int64_t)i * ns, tile))) return rc;
    }
    h->have_linv = false;  // the single-cell views of the handle may point into the arena: their cached L^-1 is not this batch's
    return GPRX_OK;
  }
  if (h->m != 0 && (count > 1 || holds.lo != nullptr) && h->d <= CELL_PAR - CELL_PAR_LS) {
    // sparse models (what gpras runs): every cell factorised by ONE batched launch sequence, then one batched predict
    std::vector<Theta> ts;
    if ((rc = decode_cells(h, count, units, thetas, z, ts))) return rc;
    std::vector<double> elbo(count);
    std::vector<int> stv(count);
    if ((rc = sgpr_objective_batch(h, count, units, ts.data(), z, elbo.data(), nullptr, nullptr, stv.data(), holds))) return rc;  // ENOTPD included
    if (ns == 0) return GPRX_OK;
    return sgpr_predict_batch(h, count, xs_dev, ns, means_dev, vars_dev, include_noise);
  }
  for (int i = 0; i < count; ++i) {
    if ((rc = objective_impl(h, units[i], thetas + (int64_t)i * h->ntheta, z ? z + (int64_t)i * h->m * h->d : nullptr, 0, nullptr, nullptr)))
      return rc;
    if ((rc = predict_dev(h, xs_dev, ns, means_dev + (int64_t)i * ns, vars_dev + (int64_t)i * ns, include_noise))) return rc;
  }
  return GPRX_OK;
}

// The slab loop of gprx_predict_batch (transposed = false: results (count, ns)) and gprx_predict_batch_t (true: (ns, count)).  The test
// points go up ONCE; the results come back in slabs of cells, so that the device staging stays small at configs[3]'s size (100 000
// points: 1.6 MB per cell): `budget` doubles for the two result blocks of a slab, or `forced_slab` cells (GPRX_PREDICT_SLAB: tests force
// the slab-by-slab copies).  Transposed: every slab is transposed on the device before it leaves and the host block is written in
// its final layout -- whole when all cells fit one slab, by 2-D copies into the slab's columns otherwise.
constexpr int NO_FORCED_SLAB = std::numeric_limits<int>::min();
int predict_batch_slabs(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns, double* means,
                        double* vars, int include_noise, bool transposed, int64_t budget, int forced_slab, bool held = false,
                        const int64_t* hold_lo = nullptr, const int64_t* hold_hi = nullptr) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !thetas || ns < 0 || (ns > 0 && (!xs || !means || !vars))) return fail(h, GPRX_EINVAL, "null argument");
  if (held && (rc = check_holds(h, count, hold_lo, hold_hi))) return rc;
  const CellHolds holds = held ? CellHolds{hold_lo, hold_hi} : CellHolds{};
  int slab = (int)std::max<int64_t>(1, std::min<int64_t>(count, budget / std::max<int64_t>(2 * ns, 1)));
  if (forced_slab != NO_FORCED_SLAB) slab = std::max(1, std::min(count, forced_slab));
  if ((rc = ensure(h, h->xs, sizeof(double) * (ns * h->d + (transposed ? 4 : 2) * ns * slab + 16)))) return rc;
  double* dxs = h->xs.p;
  double* dmean = dxs + ns * h->d;
  double* dvar = dmean + ns * slab;
  double* tmean = dvar + ns * slab;  // (transposed only)
  double* tvar = tmean + ns * slab;
  if (ns > 0) HIPCHK(h, hipMemcpyAsync(dxs, xs, sizeof(double) * ns * h->d, hipMemcpyHostToDevice, h->stream));
  for (int c0 = 0; c0 < count; c0 += slab) {
    const int cnt = std::min(slab, count - c0);
    if ((rc = predict_batch_core(h, cnt, units + c0, thetas + (int64_t)c0 * h->ntheta, z ? z + (int64_t)c0 * h->m * h->d : nullptr, dxs, ns, dmean, dvar,
                                 include_noise, holds.from(c0))))
      return rc;
    if (ns > 0 && !transposed) {
      HIPCHK(h, hipMemcpyAsync(means + (int64_t)c0 * ns, dmean, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpyAsync(vars + (int64_t)c0 * ns, dvar, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
    } else if (ns > 0) {
      launch_transpose_small(h->stream, dmean, cnt, ns, tmean);
      launch_transpose_small(h->stream, dvar, cnt, ns, tvar);
      HIPCHK(h, hipGetLastError());
      if (cnt == count) {
        HIPCHK(h, hipMemcpyAsync(means, tmean, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(vars, tvar, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
      } else {
        HIPCHK(h, hipMemcpy2DAsync(means + c0, sizeof(double) * count, tmean, sizeof(double) * cnt, sizeof(double) * cnt, (size_t)ns, hipMemcpyDeviceToHost,
                                   h->stream));
        HIPCHK(h, hipMemcpy2DAsync(vars + c0, sizeof(double) * count, tvar, sizeof(double) * cnt, sizeof(double) * cnt, (size_t)ns, hipMemcpyDeviceToHost,
                                   h->stream));
      }
    }
    HIPCHK(h, wait_stream(h, h->stream));
  }
  return GPRX_OK;
}
}  // namespace
