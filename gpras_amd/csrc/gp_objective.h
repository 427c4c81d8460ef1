// GP path, part 5 of 6: one evaluation of the objective (loss, gradient) for a lone model, for many handles and for a batch of
// cells, and the optimiser entry that steps such evaluations on the host or hands over to gp_resident.h.  After gp_resident.h.
#pragma once

namespace {
// gprx_objective (grad given) and gprx_factorize (grad null)
int objective_impl(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss, double* grad) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  Theta t;
  if ((rc = decode_cell(h, unit, theta, z, t))) return rc;
  double value = 0.0;  // LML (exact) or ELBO (sparse)
  if (h->m != 0) {
    // one model is a batch of one cell -- the same kernels, the same summation order as any batch (a model evaluated alone and
    // inside a batch agree bit for bit); the factorisation stays in cell block 0, where gprx_predict reads it
    const int64_t nz = h->m * h->d;
    std::vector<double> g(grad ? h->ntheta : 0), gzv(grad ? nz : 0);
    int st = GPRX_OK;
    if ((rc = sgpr_objective_batch(h, 1, &unit, &t, z, &value, grad ? g.data() : nullptr, grad ? gzv.data() : nullptr, &st))) return rc;
    if (loss) *loss = -(value + log_prior(h, t, mask));
    if (grad) {
      chain_rule(h, t, mask, g.data(), grad);
      double* gz = grad + h->ntheta;
      for (int64_t e = 0; e < nz; ++e) gz[e] = (mask & GPRX_TRAIN_Z) ? -gzv[e] : 0.0;
    }
    for (double& tm : h->timings) tm = 0.0;  // (no phase events inside a sequence that is replayed from a graph)
    commit_current(h, unit, t, true);
    return GPRX_OK;
  }
  // exact model with gradient: ONE stream synchronisation for both halves, and alpha from the inverse the gradient builds (the
  // 64 dependent launches of the backward substitution drop out of the evaluation); a non-PD matrix is reported by the
  // factorisation's status as before (the gradient launches behind it are then wasted, not wrong: nothing is read back)
  const bool fused = grad && fused_eval() && !h->profiling;
  std::vector<double> ghost(fused ? 2 + h->d : 0);
  if (fused) {
    if ((rc = exact_factorize_enqueue(h, unit, t, true, false, false))) return rc;
    if ((rc = exact_gradient_enqueue(h, t, ghost.data(), true))) {
      hipStreamSynchronize(h->stream);
      return rc;
    }
    if ((rc = exact_factorize_finish(h, &value))) return rc;
  } else {
    if ((rc = exact_factorize(h, unit, t, &value))) return rc;
  }
  const double lp = log_prior(h, t, mask);
  if (loss) *loss = -(value + lp);
  if (grad) {
    std::vector<double> g(h->ntheta, 0.0);
    if (fused) {
      exact_gradient_collect(h, ghost.data(), g.data());
    } else {
      if ((rc = exact_gradient(h, t, g.data()))) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
    chain_rule(h, t, mask, g.data(), grad);
  } else {
    HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
  }
  HIPCHK(h, wait_stream(h, h->stream));
  for (int s = 0; s < 4; ++s) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->ev[s], h->ev[s + 1]);
    h->timings[s] = ms;
  }
  return GPRX_OK;
}

int factorize_many(int count, gprx_handle* handles, const int* units, const double* thetas, int mask, double* losses) {
  if (count < 0 || !handles || !units || !thetas) return fail(nullptr, GPRX_EINVAL, "null argument");
  std::vector<Theta> ts(count);
  // enqueue every cell's work first (nothing blocks), then wait for each: the cells overlap on the device.
  // With several cells in flight each one runs on its single stream (no look-ahead stream): measured, 12
  // cells reach 2.2x the single-cell rate that way and only 1.5x with two streams per cell.
  for (int i = 0; i < count; ++i) {
    gprx_handle h = handles[i];
    int rc;
    if ((rc = check_handle(h))) return rc;
    if (h->m != 0) return fail(h, GPRX_EINVAL, "gprx_factorize_many: exact models only");
    if ((rc = decode_cell(h, units[i], thetas + (int64_t)i * h->ntheta, nullptr, ts[i]))) return rc;  // (a cell at a time: each has its own handle)
    if ((rc = (count == 1) ? exact_factorize_enqueue(h, units[i], ts[i], true) : exact_factorize_replay(h, units[i], ts[i]))) return rc;
  }
  int first_error = GPRX_OK;
  for (int i = 0; i < count; ++i) {
    gprx_handle h = handles[i];
    hipSetDevice(h->device);
    double lml = 0.0;
    const int rc = exact_factorize_finish(h, &lml);
    if (rc && !first_error) first_error = rc;
    if (losses) losses[i] = rc ? std::numeric_limits<double>::quiet_NaN() : -(lml + log_prior(h, ts[i], mask));
  }
  return first_error;
}

int factorize_batch(gprx_handle h, int count, const int* units, const double* thetas, int mask, double* losses, int* status) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !thetas) return fail(h, GPRX_EINVAL, "count must be positive, units and thetas non-null");
  if (h->m != 0) return fail(h, GPRX_EINVAL, "gprx_factorize_batch: exact models only");
  if (h->d > CELL_PAR - CELL_PAR_LS) return fail(h, GPRX_EINVAL, "gprx_factorize_batch: d <= 64 only");
  // (the handle keeps the decoded parameter sets of the last batch: their lengthscale vectors are reused, no allocation per cell and call --
  // 512 cells of N = 512 spent 68 us here, 5 % of the call)
  std::vector<Theta>& ts = h->batch_thetas;
  if ((rc = decode_cells(h, count, units, thetas, nullptr, ts))) return rc;
  std::vector<double>& lml = h->batch_lml;
  if ((int)lml.size() < count) lml.resize(count);
  rc = exact_factorize_batch(h, count, units, ts.data(), lml.data(), status);
  if (rc != GPRX_OK && rc != GPRX_ENOTPD) return rc;
  if (losses)
    for (int i = 0; i < count; ++i) losses[i] = -(lml[i] + log_prior(h, ts[i], mask));  // NaN for a failed cell
  return rc;
}

// held (gprx_objective_batch_held): hold_lo / hold_hi are checked in front of everything else that looks at the cells, and a batch of
// ONE cell takes the batched sparse branch as well (objective_impl knows no holds)
int objective_batch(gprx_handle h, int count, const int* units, const double* theta, const double* z, int mask, double* losses,
                         double* grads, bool held = false, const int64_t* hold_lo = nullptr, const int64_t* hold_hi = nullptr) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count < 0 || !units || !theta || !losses) return fail(h, GPRX_EINVAL, "null argument");
  if (held && (rc = check_holds(h, count, hold_lo, hold_hi))) return rc;
  const CellHolds holds = held ? CellHolds{hold_lo, hold_hi} : CellHolds{};
  const int64_t gw = h->ntheta + h->m * h->d;
  if (h->m == 0 && count > 1 && h->d <= CELL_PAR - CELL_PAR_LS) {
    // exact models: every stage once for all cells (batched launches), results identical to the loop below
    std::vector<Theta> ts;
    if ((rc = decode_cells(h, count, units, theta, nullptr, ts))) return rc;
    std::vector<double> lml(count);
    const bool form_alpha = grads && fused_eval();  // (as gprx_objective: alpha from the gradient's inverse, same kernels -> same bits)
    const int frc = exact_factorize_batch(h, count, units, ts.data(), lml.data(), nullptr, !form_alpha);
    if (frc != GPRX_OK && frc != GPRX_ENOTPD) return frc;
    for (int i = 0; i < count; ++i) losses[i] = -(lml[i] + log_prior(h, ts[i], mask));
    if (grads) {
      std::vector<double> g((size_t)count * h->ntheta, 0.0);
      if ((rc = exact_gradient_batch(h, count, g.data(), form_alpha))) {
        if (form_alpha)  // (the slots hold factors without their alpha: nothing may predict from them)
          for (int i = 0; i < count; ++i) {
            h->slot_ok[i] = 0;
            h->slot_unit[i] = -1;
          }
        return rc;
      }
      for (int i = 0; i < count; ++i) {
        double* gi = grads + (int64_t)i * gw;
        if (h->slot_ok[i]) {
          chain_rule(h, ts[i], mask, g.data() + (size_t)i * h->ntheta, gi);
        } else {
          fill_nan(gi, h->ntheta);
        }
      }
    }
    return frc;
  }
  if (h->m != 0 && (count > 1 || (held && count == 1)) && h->d <= CELL_PAR - CELL_PAR_LS) {
    const int64_t nz = h->m * h->d;
    std::vector<Theta> ts;
    if ((rc = decode_cells(h, count, units, theta, z, ts))) return rc;
    std::vector<double> elbo(count), g(grads ? (size_t)count * h->ntheta : 0), gzv(grads ? (size_t)count * nz : 0);
    std::vector<int> st(count);
    const int frc = sgpr_objective_batch(h, count, units, ts.data(), z, elbo.data(), grads ? g.data() : nullptr, grads ? gzv.data() : nullptr, st.data(),
                                         holds);
    if (frc != GPRX_OK && frc != GPRX_ENOTPD) return frc;
    for (int i = 0; i < count; ++i) {
      losses[i] = -(elbo[i] + log_prior(h, ts[i], mask));  // NaN for a failed cell
      if (!grads) continue;
      double* gi = grads + (int64_t)i * gw;
      if (st[i] != GPRX_OK) {
        fill_nan(gi, gw);
        continue;
      }
      chain_rule(h, ts[i], mask, g.data() + (size_t)i * h->ntheta, gi);
      double* gzi = gi + h->ntheta;
      for (int64_t e = 0; e < nz; ++e) gzi[e] = (mask & GPRX_TRAIN_Z) ? -gzv[(size_t)i * nz + e] : 0.0;
    }
    return frc;
  }
  // one cell after the other (a single cell, or d > 64): same contract as the batched paths -- a cell
  // whose matrix is not positive definite gets NaN, the others are still evaluated, the first failure is returned
  int first_error = GPRX_OK;
  for (int i = 0; i < count; ++i) {
    rc = objective_impl(h, units[i], theta + (int64_t)i * h->ntheta, z ? z + (int64_t)i * h->m * h->d : nullptr, mask, losses + i,
                        grads ? grads + (int64_t)i * gw : nullptr);
    if (rc == GPRX_ENOTPD) {
      losses[i] = std::numeric_limits<double>::quiet_NaN();
      if (grads) fill_nan(grads + (int64_t)i * gw, gw);
      if (!first_error) first_error = rc;
      continue;
    }
    if (rc) return rc;
  }
  return first_error;
}

// gprx_adam_batch and gprx_adadelta_batch: one loop, two updates (kind: SF_OPT_ADAM, SF_OPT_ADADELTA of sgpr_asm.h).  Adadelta has no stop
// rule, so its batch never shrinks.  last_losses (optional): the loss of each cell's last evaluation.
// held (gprx_adam_batch_held / gprx_adadelta_batch_held): the ranges are checked first; the resident loops carry them in their table (the
// one around the general launch sequence re-uploads it whenever it reopens for the cells that still run), the host-stepped loop hands the
// running cells' ranges to the held objective.
int optimizer_batch(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter,
                           double* last_losses, int* n_evals, int* batches, bool held, const int64_t* hold_lo, const int64_t* hold_hi) {
#pragma clang fp contract(off)
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !theta || !n_evals || max_iter < 0) return fail(h, GPRX_EINVAL, "null argument");
  if (h->m != 0 && !z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
  if (held && (rc = check_holds(h, count, hold_lo, hold_hi))) return rc;
  const int nt = h->ntheta;
  const int64_t nz = h->m * h->d, gw = nt + nz;
  if (batches) *batches = 0;
  for (int i = 0; i < count; ++i) n_evals[i] = 0;
  if (last_losses) fill_nan(last_losses, count);  // (no evaluation yet)
  const bool adam = kind == SF_OPT_ADAM;
  // trainable elements of a cell's gradient row [d theta | d Z] (theta: [variance, lengthscales..., noise])
  std::vector<char> train((size_t)gw, 0);
  train[0] = (mask & GPRX_TRAIN_VARIANCE) != 0;
  for (int k = 1; k < nt - 1; ++k) train[k] = (mask & GPRX_TRAIN_LENGTHSCALE) != 0;
  train[nt - 1] = (mask & GPRX_TRAIN_NOISE) != 0;
  for (int64_t e = 0; e < nz; ++e) train[nt + e] = (mask & GPRX_TRAIN_Z) != 0;
  bool any = false;
  for (char t : train) any = any || t;
  if (!any) return GPRX_OK;  // nothing trainable: no step can change anything (optimizers._optimize_adam returns at once)
  static const bool adam_on_host = env_int("GPRX_ADAM_HOST", 0) != 0;  // escape hatch: the host-stepped loop
  // sparse models with d <= 64 keep the loop on the device ("sgpr_resident" = 0: never): around the five fused launches where the
  // evaluation takes them (M <= 64), around the general launch sequence otherwise
  if (h->m != 0 && h->sgpr_resident && h->d <= CELL_PAR - CELL_PAR_LS && !adam_on_host && max_iter > 0) {
    // (the cells are checked here, in front of the resident routes only: the host-stepped loop below checks them through its first
    // evaluation, so a call that takes no step -- max_iter = 0, or the early return above -- never looks at them)
    std::vector<Theta> checked;
    if ((rc = decode_cells(h, count, units, theta, z, checked))) return rc;
    h->last_route = sgpr_five_launches(h) ? 1 : 2;
    if (sgpr_five_launches(h))
      return sgpr_resident_fused(h, kind, count, units, theta, z, mask, max_iter, last_losses, n_evals, batches,
                                 held ? CellHolds{hold_lo, hold_hi} : CellHolds{});
    return sgpr_resident_general(h, kind, count, units, theta, z, mask, max_iter, last_losses, n_evals, batches,
                                 held ? CellHolds{hold_lo, hold_hi} : CellHolds{});  // (held here: "held_general" = 1, check_holds)
  }
  std::vector<double> mom((size_t)count * gw, 0.0), vel((size_t)count * gw, 0.0), best(count, std::numeric_limits<double>::infinity());
  std::vector<int> stale(count, 0), active(count);
  for (int i = 0; i < count; ++i) active[i] = i;
  std::vector<int> a_units(count);
  std::vector<int64_t> a_lo(held ? count : 0), a_hi(held ? count : 0);
  std::vector<double> a_theta((size_t)count * nt), a_z((size_t)count * nz), losses(count), grads((size_t)count * gw);
  for (int t = 1; t <= max_iter && !active.empty(); ++t) {
    const int na = (int)active.size();
    for (int j = 0; j < na; ++j) {
      const int i = active[j];
      a_units[j] = units[i];
      if (held) {
        a_lo[j] = hold_lo[i];
        a_hi[j] = hold_hi[i];
      }
      std::memcpy(&a_theta[(size_t)j * nt], theta + (size_t)i * nt, sizeof(double) * nt);
      if (nz) std::memcpy(&a_z[(size_t)j * nz], z + (size_t)i * nz, sizeof(double) * nz);
    }
    rc = objective_batch(h, na, a_units.data(), a_theta.data(), nz ? a_z.data() : nullptr, mask, losses.data(), grads.data(), held, a_lo.data(),
                         a_hi.data());
    if (batches) ++*batches;
    for (int j = 0; j < na; ++j) ++n_evals[active[j]];
    if (last_losses)  // (a failed cell holds NaN; after any other error the evaluation wrote no loss)
      for (int j = 0; j < na; ++j) last_losses[active[j]] = (rc == GPRX_OK || rc == GPRX_ENOTPD) ? losses[j] : std::numeric_limits<double>::quiet_NaN();
    if (rc) return rc;  // (GPRX_ENOTPD included: the reference's optimiser dies with the exception of that evaluation)
    const double alpha = adam ? adam_alpha((double)t) : 0.0;
    std::vector<int> next;
    next.reserve(na);
    for (int j = 0; j < na; ++j) {
      const int i = active[j];
      double* mo = &mom[(size_t)i * gw];
      double* ve = &vel[(size_t)i * gw];
      const double* g = &grads[(size_t)j * gw];
      for (int64_t e = 0; e < gw; ++e) {
        if (!train[e]) continue;
        double* x = e < nt ? theta + (size_t)i * nt + e : z + (size_t)i * nz + (e - nt);
        if (adam)
          adam_element(g[e], alpha, mo[e], ve[e], *x);  // (sgpr_asm.h: the resident loop's kernel runs the same function)
        else
          adadelta_element(g[e], mo[e], ve[e], *x);  // (the accumulated squared gradients and updates in the moments' arrays)
      }
      if (!adam || adam_keep_running(losses[j], best[i], stale[i])) next.push_back(i);
    }
    active.swap(next);
  }
  return GPRX_OK;
}

// (gprx_last_optimizer_route: the route and the stream waits of this call)
int optimizer_routed(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter,
                            double* last_losses, int* n_evals, int* batches, bool held = false, const int64_t* hold_lo = nullptr,
                            const int64_t* hold_hi = nullptr) {
  if (h) {
    h->last_route = 0;
    h->host_waits = 0;
  }
  const int rc = optimizer_batch(h, kind, count, units, theta, z, mask, max_iter, last_losses, n_evals, batches, held, hold_lo, hold_hi);
  if (h) h->last_host_waits = h->host_waits;
  return rc;
}
}  // namespace
