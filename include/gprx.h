/*
 * gprx.h -- C ABI of the MI355X-native GP regression engine (libgprx.so).
 *
 * Drop-in boundary for the hot path of fema-ffrd/gpras.  The reference has NO FFI or
 * plugin interface for this path: its boundary is the Python class GPRAS
 * (/root/reference/gpras/gpr.py:217-384) whose arithmetic is delegated to gpflow's SGPR.
 * Each entry point below names the reference lines whose work it replaces; the Python
 * shim that a gpras maintainer would bind (ctypes) is gpras_amd/_lib.py and
 * INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain pointers and sizes only; all floating point is IEEE binary64 ("f64").
 *   - host matrices are C-contiguous row-major (what numpy hands over after
 *     x.astype(np.float64), gpr.py:265-266, :333).  The caller owns every host buffer;
 *     the library copies during the call and never keeps a host pointer.
 *   - every function returns an int status (GPRX_OK == 0).  No C++ exception crosses the
 *     boundary.  gprx_last_error() returns a message for the last failure on that handle
 *     (or, with a NULL handle, of the calling thread's last handle-less failure).
 *   - a handle is bound to one device and one HIP stream and is NOT thread-safe; different
 *     handles may be driven from different host threads / processes (one per GPU).
 *   - "unconstrained" parameters are the optimiser's variables: softplus^-1 of kernel
 *     variance and lengthscale(s), softplus^-1(noise - 1e-6) for the likelihood variance
 *     (gpflow positive() / Gaussian likelihood lower bound, as used at gpr.py:298-305).
 *     theta = [w_variance, w_lengthscale[0..n_len-1], w_noise],  n_len = ard ? d : 1.
 *   - device-pointer variants (suffix _dev) take pointers obtained from gprx_dev_malloc or
 *     from any allocator of the same HIP runtime (e.g. torch.Tensor.data_ptr()).
 */
#ifndef GPRX_H
#define GPRX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPRX_VERSION 100 /* 0.1.0 */

/* status codes */
#define GPRX_OK 0
#define GPRX_EINVAL 1  /* bad argument                       -> ValueError / KeyError   */
#define GPRX_ENOTPD 2  /* Cholesky hit a non-positive pivot  -> numpy.linalg.LinAlgError */
#define GPRX_EHIP 3    /* HIP runtime error                  -> RuntimeError            */
#define GPRX_ENOMEM 4  /* device allocation failed           -> MemoryError             */
#define GPRX_ESTATE 5  /* call order violated (e.g. predict before factorize)           */
#define GPRX_ERCCL 6   /* RCCL missing or a collective failed                -> RuntimeError */
#define GPRX_ENOCONV 7 /* the eigensolver reached its sweep cap      -> numpy.linalg.LinAlgError */

/* kernel ids: the five stationary kernels KERNEL_FACTORY (gpr.py:21-37) can construct
 * with kernel(variance=, lengthscales=) at gpr.py:298 */
#define GPRX_KERNEL_RBF 0
#define GPRX_KERNEL_MATERN12 1
#define GPRX_KERNEL_MATERN32 2
#define GPRX_KERNEL_MATERN52 3
#define GPRX_KERNEL_EXPONENTIAL 4

/* trainable mask bits (gpflow.set_trainable at gpr.py:48-49, 115-125, 133-143) */
#define GPRX_TRAIN_VARIANCE 1
#define GPRX_TRAIN_LENGTHSCALE 2
#define GPRX_TRAIN_NOISE 4
#define GPRX_TRAIN_Z 8

typedef struct gprx_ctx* gprx_handle;
typedef struct gprx_pca_ctx* gprx_pca_handle;
typedef struct gprx_pcafit_ctx* gprx_pcafit_handle;
typedef struct gprx_hms_ctx* gprx_hms_handle;
typedef struct gprx_eigh_ctx* gprx_eigh_handle;
typedef struct gprx_ps_ctx* gprx_ps_handle;
typedef struct gprx_rs_ctx* gprx_rs_handle;
typedef struct gprx_al_ctx* gprx_al_handle;
typedef struct gprx_dg_ctx* gprx_dg_handle;
typedef struct gprx_ev_ctx* gprx_ev_handle;
typedef struct gprx_comm_ctx* gprx_comm;

/* ---- library / device -------------------------------------------------------------- */
int gprx_version(void);
const char* gprx_last_error(gprx_handle h);
int gprx_device_count(int* count);

/* ---- model handle ------------------------------------------------------------------ */
/* One handle = one training set x (n, d) shared by n_units output columns, i.e. the list
 * self.models that GPRAS._init_models builds (gpr.py:277-308).  m = number of inducing
 * points (SGPR, gpr.py:299); m == 0 selects the exact GP (Z = X specialisation). */
int gprx_create(int device, int64_t n, int d, int64_t m, int kernel_id, int ard, gprx_handle* out);
int gprx_destroy(gprx_handle h);
/* run all work of this handle on an existing HIP stream (e.g. torch's current stream) */
int gprx_set_stream(gprx_handle h, void* hip_stream);
int gprx_synchronize(gprx_handle h);

/* Form of the scaled squared distance r2 inside every kernel evaluation of this handle (kernel-matrix builds and the
 * g / h factors of the gradient passes):
 *   GPRX_DIST_DIFFERENCE (default)  r2 = sum_k ((a_k - b_k) / l_k)^2: no cancellation, r2(a, a) == 0 exactly;
 *   GPRX_DIST_EXPANDED              r2 = |a/l|^2 + |b/l|^2 - 2 (a/l).(b/l): the literal arithmetic of gpflow's
 *                                   square_distance, which the kernels constructed at gpr.py:298 evaluate.
 * The two agree to rounding for RBF / Matern32 / Matern52; for Matern12 / Exponential (not differentiable at r = 0) the
 * expanded form leaves r2 ~ 1e-15 on coincident points, which moves outputs by 1e-9 .. 2.5e-8:
 * a caller that promises 1e-8 against gpflow selects GPRX_DIST_EXPANDED for those two kernels -- the host class
 * gpras_amd.gpr.GPRAS does so by default. */
#define GPRX_DIST_DIFFERENCE 0
#define GPRX_DIST_EXPANDED 1
int gprx_set_distance_form(gprx_handle h, int form);

/* x: (n, d) row-major, y: (n, n_units) row-major -- the arrays GPRAS.fit stores after the
 * float64 cast (gpr.py:265-266). */
int gprx_set_data(gprx_handle h, const double* x, const double* y, int n_units);

/* SGPR.training_loss() and its gradient w.r.t. the unconstrained variables (replaces the
 * GradientTape / gpflow.optimizers.Scipy evaluations at gpr.py:61-62, 95, 127, 153-155,
 * 186-188, 197-203).  LogNormal(0,1) log-priors (gpr.py:303-305) are added for the
 * parameters whose mask bit is set, as gpflow does for trainable parameters.
 *   theta : n_theta = 2 + n_len unconstrained values
 *   z     : (m, d) inducing inputs, ignored (may be NULL) when m == 0
 *   loss  : out, scalar
 *   grad  : out or NULL; n_theta values followed by m*d values for Z; entries of
 *           parameters whose mask bit is clear are written as 0.
 * Leaves the factorisation resident, so gprx_predict may follow for the same (unit, theta, z).
 * A sparse model (m > 0) is evaluated as a batch of ONE cell of gprx_objective_batch, for every M, d and tuning: the same launches,
 * the same bits as that cell inside any batch, and the same GPRX_ENOTPD text ("cell 0: Kuu or B not positive definite: pivot N").
 * d > 64 exceeds the lengthscale slots of a row of the cell-parameter table: the cell's hyperparameters then travel in the launch
 * arguments and the sequence is launched eagerly instead of replayed from a graph.
 * The per-cell arguments (unit, theta, z) of this and of every batched evaluation, optimiser and predict entry point below are
 * checked before any device work, cell by cell, in this order: theta NULL, unit outside [0, n_units), a theta element that is not
 * finite, z NULL (m > 0), a z element that is not finite -- GPRX_EINVAL, the first fault names the message, no output is written.
 * (gprx_adam_batch / gprx_adadelta_batch clear n_evals, batches and losses first; a call that takes no step -- max_iter = 0, nothing
 * trainable in mask -- returns GPRX_OK without looking at the cells.) */
int gprx_objective(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss, double* grad);

/* Factorise only (kernel build + Cholesky + weights); what SGPR.predict_y recomputes on
 * every call at gpr.py:337.  loss may be NULL; otherwise receives the training loss with
 * priors for the parameters in mask. */
int gprx_factorize(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss);

/* Many independent cells on one GPU: factorise `count` exact models (one handle each, all on the caller's
 * thread) by enqueueing every handle's work before waiting for any of them, so the latency-bound panel
 * chains of different cells overlap on the device.  thetas: (count, n_theta); losses: count values.
 * Replaces a Python loop of gprx_factorize calls; each handle is left factorised as by gprx_factorize.  A cell whose matrix
 * is not positive definite gets a NaN loss, the others finish, and the call returns the first such error (GPRX_ENOTPD). */
int gprx_factorize_many(int count, gprx_handle* handles, const int* units, const double* thetas, int mask, double* losses);

/* Batched cells on ONE handle: `count` exact factorisations -- cell i = (units[i], thetas[i]), all on the handle's x,
 * which is what the reference's per-mode loop (gpr.py:272-274, 336-339), its multi-start (_optimize_multi_start, gpr.py:73-109) and its
 * differential-evolution objective (_optimize_differential_evolutions, gpr.py:44-70) evaluate one after the other.  Every kernel of the factorisation
 * is launched once for all cells (cell index in the grid), so small matrices still fill the GPU.  thetas: (count,
 * n_theta); losses (may be NULL): count training losses, NaN for a cell whose matrix is not positive definite; status
 * (may be NULL): per-cell GPRX_OK / GPRX_ENOTPD.  Returns GPRX_ENOTPD if any cell failed (the others are valid).
 * Results are bit-identical to gprx_factorize on each cell -- except where many SMALL matrices take the one-workgroup-per-cell
 * factorisation (default: N <= 256 from 32 cells, N <= 512 from 160, N <= 1024 from 256; tuning key "cell_kernel" = -1 forbids it,
 * 1 forces it): the same tile products with a tile's whole update formed as one sum, equal to the launch sequence to rounding
 * (1e-13 relative on the loss, tests/test_gpu_cells.py); and from 24 cells per launch on (the split panel) the right-hand side y of a
 * cell travels as a VECTOR through the launch sequence instead of a 64-row tile below the matrix (4.5 % fewer flops at N = 4096): the
 * factor and log det are gprx_factorize's bits, beta = L^-1 y and with it y^T K^-1 y are summed in another fixed order (1e-14 relative
 * on the loss, 1e-12 on gradients; tuning key "rhs_vector" = -1 keeps the tile and with it the single call's bits).
 * The factorisations stay resident in slots 0..count-1
 * until the next batch; gprx_select_slot makes one of them current for gprx_predict / gprx_predict_dev. */
int gprx_factorize_batch(gprx_handle h, int count, const int* units, const double* thetas, int mask, double* losses, int* status);
int gprx_select_slot(gprx_handle h, int slot);
/* device time (ms) of the last gprx_factorize_batch, HIP events on the handle's stream around the whole batch */
int gprx_last_batch_ms(gprx_handle h, double* ms);

/* SGPR.predict_y (gpr.py:336-339): predictive mean and variance at xs (ns, d) for the unit
 * factorised last.  include_noise != 0 adds the likelihood variance (predict_y); 0 gives
 * predict_f.  mean/var: ns values each.  Works after every successful gprx_factorize / gprx_objective (GPRX_ESTATE otherwise);
 * a sparse model predicts from its cell block, 4096 points per pass, as a cell of gprx_predict_batch does. */
int gprx_predict(gprx_handle h, const double* xs, int64_t ns, double* mean, double* var, int include_noise);
/* same, every pointer is a device pointer; asynchronous on the handle's stream */
int gprx_predict_dev(gprx_handle h, const double* xs_dev, int64_t ns, double* mean_dev, double* var_dev, int include_noise);

/* timings (ms, HIP events on the handle's stream) of the stages of the last
 * gprx_objective / gprx_factorize call: [kernel build, cholesky, solves, gradient].  Exact models only: after a sparse
 * evaluation (one launch sequence, replayed from a graph: no events inside) all four are 0. */
int gprx_last_timings(gprx_handle h, double* ms4);

/* Per-launch timing of the Cholesky's two kernels (exact path), for bench.py's roofline line.
 * With profiling enabled every gprx_factorize / gprx_objective / gprx_factorize_batch brackets each launch with HIP
 * events on the launch stream (this perturbs the run slightly: keep it off inside timed regions).
 * gprx_last_profile: out8 = [main GEMM kernel gemm_f64_kernel<0,1,64,64,0> (bulk trailing updates and in-block updates
 *                           with K > 128) total ms, launches, algorithmic flops (all cells of a batch), panel kernel
 *                           total ms, launches, short-K in-block updates (K = 64 / 128: GEMM with C
 *                           prefetch) total ms, launches, algorithmic flops] of the last exact factorisation(s). */
int gprx_set_profiling(gprx_handle h, int enabled);
int gprx_last_profile(gprx_handle h, double* out8);
/* The kernel-build launch (kmat_kernel: every 64 x 64 tile on or below the diagonal, all cells of a batch in one launch) of the
 * last PROFILED exact factorisation: duration by HIP events around that launch, and the bytes it writes (8 * 64 * 64 * lower tiles
 * * cells) -- bench.py's kernel_build_hbm figure (north_star: "HBM GB/s on the kernel build"; reference: the K(X, X) inside
 * every training_loss, /root/reference/gpras/gpr.py:153-155). */
int gprx_last_kernel_build(gprx_handle h, double* ms, double* bytes);
/* The one-workgroup-per-cell Cholesky launch (potrf_cell.h: the default for many cells of N <= 1024) of the last PROFILED
 * gprx_factorize_batch on a handle whose tuning forces it ("cell_kernel" = 1; without that a profiled batch runs the instrumented
 * launch sequence): duration by HIP events around that ONE launch, its algorithmic flops (N^3 / 3 per cell) and the cell count;
 * zeros when the last profiled call did not run it.  bench.py's other_sizes.N1024_d8_roofline. */
int gprx_last_cell_kernel(gprx_handle h, double* ms, double* flops, double* cells);

/* ---- batched small problems ------------------------------------------------------- */
/* Evaluate loss (+ gradient) for `count` units in one call: units[i] with theta row i
 * (count, n_theta) and z block i (count, m, d).  Replaces the serial loop over
 * self.models at gpr.py:272-274.  losses: count values; grads: (count, n_theta + m*d) or NULL.
 * With count > 1 (and d <= 64) every stage runs once for all cells, the cell index in every launch's grid: exact models
 * -- kernel build, Cholesky, solves, L^-1, K^-1, the trace pass (as gprx_factorize_batch) --, and sparse models.
 * Sparse models with M <= 64 inducing points (the reference's example configuration has 50) take FIVE launches per evaluation
 * whatever the cell count (round 5, csrc/sgpr_fused.h: Kuu and its factor | Kuf tile by tile on MFMA against the register-resident
 * L^-1, never stored | B, its factor and the M x M algebra of the gradient | the contractions with dk/dtheta and dk/dZ | sums in a
 * fixed order).  Larger M takes the general launch sequence (Kuf, Kuu, both Cholesky factorisations, A, B (split-K), c, the M x M
 * products of the gradient, both trace passes, dZ: ~45 launches serve all cells, replayed from a graph).  gprx_objective is the
 * same sequence with one cell: a model evaluated alone and inside a batch gives the same bits.
 * The tuning key "sgpr_fused" = 0 sends M <= 64 through that sequence as well (equal to rounding, not bit for bit).  A cell
 * whose matrix is not positive definite gets NaN loss and gradient and the call returns GPRX_ENOTPD after finishing the
 * others.  count == 1, and every count with d > 64 (one cell after the other), is gprx_objective per cell: the last cell stays
 * resident for gprx_predict.  A batch of several cells leaves the handle unfactorised (gprx_predict needs a gprx_factorize /
 * gprx_objective). */
int gprx_objective_batch(gprx_handle h, int count, const int* units, const double* theta, const double* z, int mask,
                         double* losses, double* grads);

/* Sizing of batched calls: free / total device memory, and the device bytes ONE cell of a batched call on this handle
 * occupies (exact models: kernel matrix + staging + alpha, plus L^-1 and K^-1 when gradients are asked for; sparse models:
 * the cell block of gprx_objective_batch).  A caller keeps count * cell_bytes below the free memory; a batch that does
 * not fit returns GPRX_ENOMEM and may be retried with fewer cells (results do not depend on the batch composition). */
int gprx_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes);
int gprx_cell_bytes(gprx_handle h, int with_gradient, int64_t* bytes);

/* ---- multi-GPU: independent units sharded over ranks, ONE gather at the end ------------------- */
/* The reference has no multi-device code; its unit loops (gpr.py:272-274, 336-339; restarts :87; CV configurations,
 * cross_validation.py:61) are serial and share nothing but x.  One process per GPU: unit u -> rank u mod world, no
 * communication during compute, and these calls for the single collective at the end.  RCCL is loaded at run time
 * (dlopen), communicators are bound to one device and one private stream; every buffer is DEVICE memory and the calls are
 * asynchronous on that stream (gprx_comm_synchronize waits), so results never bounce through the host.
 *   gprx_comm_unique_id : rank 0 creates the 128-byte id (ncclGetUniqueId); the launcher distributes it (any side channel:
 *                         torch.distributed's store, a file, MPI) -- the id is the only out-of-band datum.
 *   gprx_comm_init      : collective over all ranks (ncclCommInitRank).
 *   gprx_comm_all_gather: recv_dev (world * count) <- every rank's send_dev (count), rank-major (ncclAllGather).
 *   gprx_comm_gather    : to `root` only, as grouped ncclSend / ncclRecv (all inbound xGMI links of the root at once);
 *                         recv_dev is read on the root only.
 *   gprx_comm_all_reduce_max: element-wise maximum in place (the slowest rank's time of a benchmark).
 *   gprx_comm_all_gather_host: the same all-gather for small HOST buffers (fitted parameters), staged through the device;
 *                         synchronous.   gprx_comm_barrier: all ranks have arrived (one-element all-reduce + wait). */
#define GPRX_UNIQUE_ID_BYTES 128
/* Everything gprx_comm_init needs short of the collective itself: the device is selectable, HIP is initialised, RCCL is loaded
 * and its symbols resolve.  Ranks agree on this through their launcher BEFORE anyone calls gprx_comm_init (a rank that fails
 * here would otherwise leave the others blocked inside ncclCommInitRank). */
int gprx_comm_runtime_check(int device);
int gprx_comm_unique_id(unsigned char* id128);
int gprx_comm_init(int device, int rank, int world, const unsigned char* id128, gprx_comm* out);
int gprx_comm_destroy(gprx_comm c);
const char* gprx_comm_last_error(gprx_comm c);
/* rank / world as RCCL itself reports them for the communicator (ncclCommUserRank / ncclCommCount), not the caller's numbers */
int gprx_comm_rank(gprx_comm c, int* rank, int* world);
int gprx_comm_all_gather(gprx_comm c, const double* send_dev, double* recv_dev, int64_t count);
int gprx_comm_gather(gprx_comm c, const double* send_dev, double* recv_dev, int64_t count, int root);
int gprx_comm_all_reduce_max(gprx_comm c, double* buf_dev, int64_t count);
int gprx_comm_all_gather_host(gprx_comm c, const double* send, double* recv, int64_t count);
int gprx_comm_barrier(gprx_comm c);
int gprx_comm_synchronize(gprx_comm c);

/* ---- device memory helpers (for callers that keep inputs resident in HBM) ----------- */
int gprx_dev_malloc(int device, int64_t bytes, void** out);
int gprx_dev_free(int device, void* ptr);
int gprx_memcpy_h2d(int device, void* dst_dev, const void* src_host, int64_t bytes);
int gprx_memcpy_d2h(int device, void* dst_host, const void* src_dev, int64_t bytes);

/* ---- building blocks (exported for parity tests, profiling and bench.py) ----------- */
/* All matrices row-major f64 in device memory, leading dimension in elements.  These run on
 * the library's non-blocking utility stream of `device` (one per device; the library never touches the legacy NULL stream) and
 * synchronise that stream before returning unless noted. */

/* out[i, j] = variance * g(r(a_i, b_j)) + (i == j ? diag_add : 0)
 * a: (n1, d), b: (n2, d) device, ls: d host values (lengthscale per dimension; inputs are divided by it).
 * mode 0: all of the (n1p, n2p) padded rectangle, zero padding; mode 1: a == b, only tiles on or
 * below the diagonal are written (what the Cholesky reads); mode 2: a == b, all tiles.  Modes 1
 * and 2 pad (i >= n1 or j >= n2) with the identity.  mode + 4: the same with r2 in gpflow's expanded form
 * (GPRX_DIST_EXPANDED, see gprx_set_distance_form). */
int gprx_kmat(int device, int kernel_id, const double* a_dev, int64_t n1, const double* b_dev, int64_t n2, int d,
              const double* ls_host, double variance, double diag_add, double* out_dev, int64_t ld, int64_t n1p,
              int64_t n2p, int mode);

/* C = alpha * op(A) op(B) + beta * C;  ta/tb: 0 = as stored, 1 = transposed.  Supported:
 * (ta,tb) in {(0,1), (0,0), (1,0)}.  k must be a multiple of 16.  flags: GPRX_GEMM_* */
#define GPRX_GEMM_C_LOWER 1  /* compute only tiles touching the lower triangle of C            */
#define GPRX_GEMM_A_LOWER 2  /* op(A)[i,k] == 0 for k > i  (skip zero tiles)                  */
#define GPRX_GEMM_A_UPPER 4  /* op(A)[i,k] == 0 for k < i                                     */
#define GPRX_GEMM_B_LOWER 8  /* op(B)[k,j] == 0 for k < j                                     */
#define GPRX_GEMM_B_UPPER 16 /* op(B)[k,j] == 0 for k > j                                     */
int gprx_gemm(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
              const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, int flags, int tile);

/* In-place lower Cholesky of the (np, np) matrix (np multiple of 64) with `extra` right-hand
 * side rows stored below it (rows np .. np+extra-1, each of length np): on return the lower
 * triangle holds L, the extra rows hold (L^-1 rhs)^T, inv_diag (np/64 blocks of 64x64) holds
 * the inverses of the diagonal blocks.  info_host: 0, or 1-based index of the failing pivot. */
int gprx_potrf(int device, double* a_dev, int64_t lda, int64_t np, int64_t extra, double* inv_diag_dev, int* info_host);

/* ---- probes: every argument of the GEMM dispatcher and the host drivers and reductions of the triangular solves, for the block
 * tests.  All pointers are device pointers.  Each returns GPRX_EINVAL, before any device work, for what its kernels cannot take:
 * odd leading dimensions or batch / cell strides of what is read with 16-byte loads (A and B of a product, L, inv_diag, a matrix
 * right-hand side, X, T, the matrix of the row reduction), those pointers off a 16-byte boundary, k or kchunk not a multiple of 16,
 * np not a multiple of 64.  ldc of a product may be odd (C is read and written element by element; the vector form has ldc = 1), and
 * nothing is asked of the vectors of gprx_trsv_lower or of the operands of gprx_alpha_from_inverse, LOGDET_QUAD and COL, whose
 * kernels use scalar loads. */

/* gprx_gemm for batch x cells products: entry e of cell c reads A + c cell_a + e stride_a (B, C likewise) and uses
 * alpha_tab[c * alpha_stride] when alpha_tab is given.  rowsq != NULL: C is not stored; the row sums of squares of alpha op(A) op(B)
 * go to 2 * ceil(n / tile) slabs rowsq_ld apart; rowsq needs tile 64 or 128 and batch == cells == 1. */
int gprx_gemm_batched(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
                      const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, int flags, int tile, int batch,
                      int64_t stride_a, int64_t stride_b, int64_t stride_c, int cells, int64_t cell_a, int64_t cell_b, int64_t cell_c,
                      const double* alpha_tab_dev, int alpha_stride, double* rowsq_dev, int64_t rowsq_ld);

/* The same product with K cut into slices of kchunk, summed in a fixed order; ws: ceil(k / kchunk) * m * n doubles per cell, ws_cell apart. */
int gprx_gemm_splitk(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
                     const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, double* ws_dev, int kchunk, int cells,
                     int64_t cell_a, int64_t cell_b, int64_t cell_c, int64_t ws_cell, const double* alpha_tab_dev, int alpha_stride);

/* L x = b (transpose 0) or L^T x = b (1) in place, L lower (np, np) with the inverses of its 64 x 64 diagonal blocks in inv_diag;
 * batch systems whose L, inv_diag and b are all cs doubles apart.  work (transpose, batch 1): holds the right-hand side on entry and
 * is used up, b only receives the solution. */
int gprx_trsv_lower(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* b_dev, int64_t np, int transpose,
                    int batch, int64_t cs, double* work_dev);

/* gprx_potrf for `batch` matrices by a named route: 0 = the launch sequence with the fused panel, 1 = with the split panel (one
 * diagonal workgroup per cell, then a rows-only kernel), 2 = one workgroup per cell (extra a multiple of 64).  Cell c has its matrix
 * at a_dev + c cs, the inverses of its diagonal blocks at inv_diag_dev + c cs, its staging area (np * 129 doubles, scratch of routes 0
 * and 1) at stage_dev + c cs.  yvec_dev (route 1, batch > 1, extra == 0; else NULL): one right-hand side per cell as a vector of np
 * entries at yvec_dev + c cs, replaced by L^-1 y.  The schedule is the call's own, the process-wide tuning is neither read nor
 * changed: outer_block 0 (default) or any multiple of 64, update_tile 0 | 64 | 128, lookahead 1 (batch == 1, routes 0 and 1) = bulk
 * updates on a second stream.  info_host[batch]: 0 or col_base + the 1-based index of the cell's failing pivot; GPRX_ENOTPD when any
 * is non-zero.  GPRX_EINVAL before any device work for odd lda or cs, lda < np, batch > 1 with cs < lda (np + extra) (cells that
 * would overlap), pointers off a 16-byte boundary and every
 * combination named above that no route takes. */
int gprx_potrf_batched(int device, double* a_dev, int64_t lda, int64_t np, int64_t extra, double* inv_diag_dev, double* stage_dev,
                       double* yvec_dev, int batch, int64_t cs, int route, int outer_block, int update_tile, int lookahead, int col_base,
                       int* info_host);

/* L X = B in place, B (n, ncols); cells systems cs doubles apart.  src (n == 64): the right-hand side is read from there. */
int gprx_trsm_lower_left(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* b_dev, int64_t ldb, int64_t n,
                         int64_t ncols, int cells, int64_t cs, const double* src_dev);

/* X = L^-1: the blocks on and below the block diagonal of X are written, T (np, np) is scratch. */
int gprx_trtri_lower(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* x_dev, int64_t ldx, double* t_dev,
                     int64_t ldt, int64_t np, int cells, int64_t cs_l, int64_t cs_x, int tile);

int gprx_transpose_inplace(int device, double* x_dev, int64_t ld, int64_t n, int cells, int64_t cs);

/* alpha_j = sum_{i >= j} X[i][j] beta_i; part: cells * ceil(np / 512) * np doubles. */
int gprx_alpha_from_inverse(int device, const double* x_dev, int64_t ldx, const double* beta_dev, double* part_dev, double* alpha_dev, int64_t np,
                            int cells, int64_t cs_x, int64_t cs_b, int64_t cs_a);

/* The reductions of the solves.  LOGDET_QUAD: out[c * out_cell + {0, 1}] = sum log M[i][i], sum w[i]^2 (M square of order nrows).
 * COL: out[t] = (accumulate ? out[t] : base) + scale * sum_r (w ? w[r] M[r][t] : M[r][t]^2), partial: ceil(nrows / rows_per_chunk) * ncols
 * doubles per cell; base = base_tab[c * base_stride] (+ base_tab2[c * base_stride]) when given.  ROWSQ_FINAL: out[r] = base - the sum over
 * the ncols slabs, ldm apart, of M[slab * ldm + r].  ROW: out[r] = base + scale * sum_c (w ? w[c] M[r][c] : M[r][c]^2). */
#define GPRX_REDUCE_LOGDET_QUAD 0
#define GPRX_REDUCE_COL 1
#define GPRX_REDUCE_ROWSQ_FINAL 2
#define GPRX_REDUCE_ROW 3
int gprx_reduce_probe(int device, int op, const double* m_dev, int64_t ldm, const double* w_dev, int64_t nrows, int64_t ncols, double base,
                      double scale, int accumulate, double* partial_dev, int rows_per_chunk, double* out_dev, int cells, int64_t m_cell,
                      int64_t w_cell, int64_t p_cell, int64_t out_cell, const double* base_tab_dev, const double* base_tab2_dev, int base_stride);

/* The whole predict loop of gpr.py:336-339 in one call: cell i = (units[i], thetas[i], z block i for sparse models) is
 * factorised (exact models: all cells by one batched launch sequence) and predicts at the shared xs (ns, d);
 * means / vars: (count, ns) row-major (the transpose of GPRAS.predict's (ns, K)). */
int gprx_predict_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                       double* means, double* vars, int include_noise);

/* The same with the results in the layout GPRAS.predict returns (gpr.py:340-342: the modes' columns concatenated): means_t / vars_t
 * (ns, count) row-major -- every slab of cells is transposed on the device before it is copied out.  Same values. */
int gprx_predict_batch_t(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                         double* means_t, double* vars_t, int include_noise);

/* The same with the test points and the results in DEVICE memory (means_dev / vars_dev: (count, ns) row-major), asynchronous
 * on the handle's stream once the batched factorisation has returned: predictions that stay in HBM for the reverse
 * projection and the metrics (production/analysis/pipeline.py:260-288). */
int gprx_predict_batch_dev(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                           double* means_dev, double* vars_dev, int include_noise);

/* The JOINT predictive distribution of the same cells over the test points of ONE event: means_dev (count, ns) as above (equal to
 * gprx_predict_batch_dev's bit for bit: tested, for lone cells too, which that call evaluates through the single-model entry) and lc_dev (count, Tp, Tp), Tp = ns rounded up to 64: per cell the lower Cholesky factor of
 *   C = Kss - tmp1^T tmp1 + tmp2^T tmp2 + noise I,   tmp1 = L^-1 Kus,  tmp2 = LB^-1 tmp1
 * (gpflow SGPR.predict_f with full_cov), zeros above the diagonal, the identity on the padding.  include_noise == 0: the noise is left
 * out and jitter * variance (jitter = 1e-6, the library's Kuu jitter) goes on the diagonal instead before the factorisation: the
 * noise-free covariance of correlated rows is singular to working precision.  Sparse models with M <= 320, 1 <= ns <= 1024, d <= 64;
 * anything else is GPRX_EINVAL before any device work.  A non-positive pivot is GPRX_ENOTPD, the message names the cell.  The call
 * synchronises. */
int gprx_predict_joint_batch_dev(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                                 double* means_dev, double* lc_dev, int include_noise);

/* The reference's Adam driver (gpr.py:147-173: tf.keras.optimizers.Adam() defaults, at most max_iter steps, early stop once the
 * relative improvement of the loss stayed <= 1e-5 for more than 50 consecutive steps) for `count` cells in lock step.
 * Sparse models with M <= 64 (round 5): the loop is RESIDENT ON THE DEVICE -- variables, moments, best loss and patience counters
 * live in device memory, a step is four launches (the last one forms loss and gradient, applies the update and the stop rule and
 * opens the next step with Kuu of the new variables; softplus, its derivative and the LogNormal priors are evaluated inside the
 * kernel), cells that have stopped return at once from every launch, and the host only reads the stop flags every 25 steps
 * (GPRX_ADAM_CHECK_EVERY): nothing else crosses the host link between the call's first upload and its last download.
 * GPRX_ADAM_HOST=1 selects the host-stepped loop below instead; both give the same variables bit for bit (the scalar tail of an
 * evaluation and the update are ONE source for host and device, csrc/sgpr_asm.h, on exp / log written out in IEEE operations,
 * csrc/px_math.h).
 * Every other sparse model with d <= 64 -- M > 64, or M <= 64 with "sgpr_fused" = 0 -- keeps the loop on the device as well, around
 * the general launch sequence: a step is that sequence without its stage-in and stage-out launches, closed by ONE step kernel
 * (csrc/sgpr_step.h) that forms the trace sums, the loss and the gradient, applies the update and the stop rule and writes the next
 * step's parameter row; the step is captured into a linear graph per (cells, optimiser) and replayed, what changes between steps is
 * read from device memory, the flags are read every 25 steps as above, and at a read where cells have stopped the batch shrinks to
 * the running ones.  Same bits as the host-stepped loop.  "sgpr_resident" = 0 (gprx_set_tuning / gprx_set_handle_tuning) selects the
 * host-stepped loop for every sparse model; gprx_last_optimizer_route reports which loop a call took.  Other models (exact ones,
 * d > 64): every step
 * is ONE batched evaluation (gprx_objective_batch) of the cells still running, the update happens here on the host side of the
 * library -- no per-step round trip through the caller's language.  theta (count, n_theta) and z (count, m, d; NULL for exact
 * models) are the optimiser's variables, updated in place (elements outside `mask` stay as they are); n_evals[i] receives the
 * number of evaluations cell i took part in; batches (optional) the number of batched evaluations.  The arithmetic per element
 * is that of the NumPy statement of the update (one rounding per operation, no contraction): the result equals
 * gpras_amd.optimizers._optimize_adam on each cell bit for bit.  A cell whose matrix stops being positive definite ends the
 * call with GPRX_ENOTPD (gpr.py: the exception leaves the optimiser); theta / z hold the state of that step (resident loop: the
 * failing cell is as it was before the failing evaluation, the others may be up to 24 steps further: the flags are read every 25).
 * Its twin with Keras's Adadelta update is gprx_adadelta_batch below: same routes, same launches, another update. */
int gprx_adam_batch(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, int* n_evals, int* batches);

/* The reference's Adadelta driver, _optimize_adadelta (gpr.py:176-192: tf.keras.optimizers.Adadelta() defaults -- learning rate 1e-3,
 * rho 0.95, epsilon 1e-7), for `count` cells in lock step: exactly max_iter steps for every cell, no early stop, fresh accumulators
 * per call.  The routes are those of gprx_adam_batch: sparse models with M <= 64 run the loop resident on the device (the same four
 * launches per step, the last one with this update; the error word is read every 25 steps), the other sparse models with d <= 64
 * run it resident around the general launch sequence (the same step kernel with this update), every other model -- and every model
 * under GPRX_ADAM_HOST=1 or "sgpr_resident" = 0 -- takes one batched evaluation per step with the update on the host side of the library; both give the
 * same variables bit for bit (the update is one source for host and device, csrc/sgpr_asm.h adadelta_element: one rounding per
 * operation in the order of the NumPy statement in gpras_amd/optimizers.py).  theta, z, mask, n_evals and batches as in
 * gprx_adam_batch; a mask with nothing trainable returns at once.  losses (optional, count doubles) receives the loss of each
 * cell's last evaluation -- what the reference's driver returns -- and NaN where none was made or the last one failed.  A cell that
 * stops being positive definite ends the call with GPRX_ENOTPD and is named in gprx_last_error; theta / z as gprx_adam_batch
 * leaves them in that case. */
int gprx_adadelta_batch(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses,
                        int* n_evals, int* batches);

/* Which loop the handle's last call of gprx_adam_batch (_optimize_adam, gpr.py:147-173) or of
 * gprx_adadelta_batch (_optimize_adadelta, gpr.py:176-192) took, and how often that call waited for the stream.
 * route: 0 host-stepped, 1 resident around the five fused launches, 2 resident around the general launch sequence.
 * host_waits counts the loop's own waits.  A resident loop waits for its opening upload, once per window of 25 steps, for its
 * closing download, and for one more round trip per shrink of the batch; the host-stepped loop waits once per step.  The
 * allocation of a handle's buffers on its first call is not counted. */
int gprx_last_optimizer_route(gprx_handle h, int* route, int* host_waits);

/* ---- Held-out rows: the folds of a cross-validation as cells of ONE batch ---------------------------------------------------------
 * The four calls below are gprx_objective_batch, gprx_adam_batch, gprx_adadelta_batch and gprx_predict_batch with one more property
 * per cell: cell i's model does not see the training rows [hold_lo[i], hold_hi[i]) of the handle's data (`count` values each, behind
 * the arguments of the parent call).  Everything the parent's contract says holds, with "the data" read as "the kept rows": the loss
 * and the gradient are those of the model on x[keep], y[keep] (the reference's SGPR built on the fold's rows, as
 * production/analysis/cross_validation.py refits it), the optimiser loops run on that loss, and gprx_predict_batch_held factorises
 * every cell without its held rows before it predicts at xs (host arrays, results (count, ns)).
 *   hold_lo[i] == hold_hi[i]: the cell holds nothing; its results have the bits of the parent call.  A call in which no cell holds a
 *     row runs the parent's launches.
 *   A cell's values do not depend on what the other cells hold, on its position in the batch or on the batch's size, bit for bit; a
 *     cell that holds the suffix [k, n) out has the bits of the same cell on a handle created with the first k rows: a held column
 *     contributes exact zeros to every sum, chunks of 256 columns are added in chunk order, and the row count and y.y of the scalar
 *     tail are formed over the kept rows in row order, as gprx_set_data forms them.
 *   They serve sparse handles on the five fused launches: m <= 64, d <= 64, "sgpr_fused" = 1.  The resident loop carries the ranges
 *     through every step (each group of cells of a large batch its own part); with "sgpr_resident" = 0 or GPRX_ADAM_HOST=1 the
 *     host-stepped loop hands them to the held objective; both give the same variables bit for bit.  gprx_last_optimizer_route
 *     reports as for the parents.
 *   With the handle tuning key "held_general" = 1 they also serve sparse handles with d <= 64 on the general launch sequence (m > 64,
 *     or "sgpr_fused" = 0): the held columns of Kuf and the held entries of the staged y are exact zeros, so every later launch adds
 *     exact zeros for them.  Everything above holds there EXCEPT the suffix property: the trace partials are summed over
 *     tiles_m x tiles_n partials and the GEMM route changes at np = 1024, so the bits depend on the handle's n.  Calls in which no
 *     cell holds a row, and every call without "_held", run the launches and graphs they always ran.
 *   GPRX_EINVAL, before any device work and with the reason in gprx_last_error: an exact handle, m > 64, d > 64, "sgpr_fused" = 0
 *     (the last two: unless "held_general" = 1), a null range array, hold_lo[i] > hold_hi[i], a range outside [0, n], a range that
 *     keeps no row. */
int gprx_objective_batch_held(gprx_handle h, int count, const int* units, const double* theta, const double* z, int mask, double* losses,
                              double* grads, const int64_t* hold_lo, const int64_t* hold_hi);
int gprx_adam_batch_held(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, int* n_evals, int* batches,
                         const int64_t* hold_lo, const int64_t* hold_hi);
int gprx_adadelta_batch_held(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses,
                             int* n_evals, int* batches, const int64_t* hold_lo, const int64_t* hold_hi);
int gprx_predict_batch_held(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                            double* means, double* vars, int include_noise, const int64_t* hold_lo, const int64_t* hold_hi);

/* Leave-one-event-out predictions of fitted sparse models on their own training rows (model selection: the held-out score of every
 * training event of production/analysis/cross_validation.py without one refit per event).  Cell i = (units[i], thetas[i], z block i)
 * is factorised once; for every event e = rows [ev_lo[e], ev_hi[e]) of the handle's x the call returns, at those rows, SGPR predict_y
 * of the model built on ALL OTHER rows at the SAME hyperparameters and inducing points -- nothing is re-optimised per fold.  With
 * t1 = L^-1 k(Z, X[lo:hi]) and t2 = LB^-1 t1 (the predict path's tmp1 / tmp2):
 *   H = I - t2 t2^T / s,  Lh = chol(H),  c' = Lh^-1 (c - t2 y[lo:hi] / s),  W = Lh^-1 t2,
 *   mean_j = W[:, j]^T c',  var_j = v - colsum(t1^2)_j + colsum(W^2)_j  (+ s with include_noise)
 * one workgroup per (event, cell) after the head of the batched predict on tiles of consecutive events; a (cell, event) result has
 * the same bits whatever else is in the batch or in the event list.
 * means / vars: (count, N) row-major; rows that belong to no event come back NaN.  status: (count, n_events), 0 or the 1-based pivot
 * at which chol(H) failed (that event's rows are then NaN in that cell; the call still returns GPRX_OK).
 * GPRX_EINVAL, before any device work: an exact handle, more than 64 inducing points, d > 64, ranges that are unsorted, overlapping,
 * empty or outside [0, N], an event longer than one predict tile (4096 rows).  GPRX_ENOTPD: a cell's own factorisation failed. */
int gprx_loeo_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, int n_events, const int64_t* ev_lo,
                    const int64_t* ev_hi, double* means, double* vars, int include_noise, int* status);

/* ran: 1 when the handle's last gprx_loeo_batch ran its downdate kernel to the end, 0 when it returned an error (or none was made).
 * stage_ms (optional, 4 doubles) of that call: [0] the batched factorisation (host clock, its wait included), [1] the predict head of
 * the first tile, [2] the downdate kernel of the first tile, [3] everything between the first tile's start and the copies out (device). */
int gprx_last_loeo(gprx_handle h, int* ran, double* stage_ms);

/* The same leave-one-event-out predictions for sparse models with up to 320 inducing points (mp = 64 ceil(M / 64) <= 320; mp = 64 is
 * taken too).  H is mp x mp and no longer fits one workgroup: every (cell, event) gets a SLOT of a device workspace, and the downdate
 * runs per GROUP of consecutive events of a tile whose count x events slots fit the workspace -- a kernel that writes H = I - t2 t2^T / s
 * tile by tile and u = t2 y, the batched Cholesky and the batched triangular inverse (P = Lh^-1) over all slots of the group under a
 * schedule fixed by mp alone, c' = P (c - u / s), and a kernel that forms W = P t2 per 64-column chunk of the event with
 * mean = W^T c' and var += colsum(W^2) (+ s last).  Every sum has one order and workgroups share nothing: a (cell, event) result has
 * the same bits whatever else is in the batch, the event list, the tile or the group.  Outputs, status and return values as
 * gprx_loeo_batch.  max_slots > 0: at most so many slots per group (a group always holds at least one event); 0: as many as the
 * default workspace cap (2 GiB) holds.  GPRX_EINVAL, before any device work: an exact handle, mp > 320, d > 64, the range rules of
 * gprx_loeo_batch, max_slots < 0.  GPRX_ENOMEM: the workspace does not fit the free device memory.  gprx_last_loeo is not touched. */
int gprx_loeo_batch_blocked(gprx_handle h, int count, const int* units, const double* thetas, const double* z, int n_events, const int64_t* ev_lo,
                            const int64_t* ev_hi, double* means, double* vars, int include_noise, int max_slots, int* status);

/* ran: 1 when the handle's last gprx_loeo_batch_blocked ran to the end, 0 when it returned an error (or none was made); groups: how many
 * groups it ran.  stage_ms (optional, 6 doubles): [0] the batched factorisation (host clock, its wait included), [1] the predict head of
 * the first tile, then of the first group [2] the kernel that writes H, [3] the Cholesky and the inverse, [4] c' and the apply kernel,
 * [5] everything between the first tile's start and the copies out (device). */
int gprx_last_loeo_blocked(gprx_handle h, int* ran, int* groups, double* stage_ms);

/* ---- EOF (PCA) projection either side of the GP path: SURVEY.md section 8(f) row N1 ------------------- */
/* One projector = the fitted state of a reference PreProcessor (gpras/preprocess.py:868-927): `dry` (n_cells bytes, 1 =
 * always-dry cell, may be NULL = none), `elevations` (n_cells, needed for depth mode and for filling dry cells in wse mode),
 * and, over the n_wet = n_cells - sum(dry) wet cells in ascending cell order: `input_mean` (n_wet), `weights` (n_wet or
 * NULL = unweighted), `eofs` (k, n_wet) row-major; `x_mean`, `x_std` (k).  depth_mode != 0: inputs are water-surface
 * elevations converted with max(x - elevation, 0) (wse_2_depth, preprocess.py:1040-1044).  1 <= k <= 64. */
int gprx_pca_create(int device, int64_t n_cells, int k, const unsigned char* dry, const double* elevations, const double* input_mean,
                    const double* weights, const double* eofs, const double* x_mean, const double* x_std, int depth_mode,
                    gprx_pca_handle* out);
int gprx_pca_destroy(gprx_pca_handle p);
const char* gprx_pca_last_error(gprx_pca_handle p);
/* PreProcessor.transform (preprocess.py:1009-1038): x (rows, n_cells) -> z (rows, k), host buffers. */
int gprx_pca_transform(gprx_pca_handle p, const double* x, int64_t rows, double* z);
/* PreProcessor.reverse_transform (preprocess.py:1052-1085) with _linear_transform_for_var (:1087-1094): mean (rows, k)
 * [, var (rows, k)] -> full (rows, n_cells) [, var_full (rows, n_cells)]; var and var_full both NULL or both given. */
int gprx_pca_reverse(gprx_pca_handle p, const double* mean, const double* var, int64_t rows, double* full, double* var_full);
/* device-resident forms, asynchronous on the projector's stream (gprx_pca_synchronize waits).  x_dev: (rows, ld) with
 * ld = n_cells rounded up to a multiple of 16 (padding columns: any finite values); outputs as above with ld = k / n_cells. */
int gprx_pca_transform_dev(gprx_pca_handle p, const double* x_dev, int64_t rows, double* z_dev);
int gprx_pca_reverse_dev(gprx_pca_handle p, const double* mean_dev, const double* var_dev, int64_t rows, double* full_dev, double* vfull_dev);
int gprx_pca_synchronize(gprx_pca_handle p);
/* What production/analysis/pipeline.py:262-277 and :286 do to the reconstructed fields before the metrics, in place on the
 * device and on the projector's stream:  to_depth -- field (rows, n_cells): add_elevations_first != 0 ("depth" models:
 * y += elevations, then wse_2_depth) computes max((y + e) - e, 0), else max(y - e, 0) (PreProcessor.wse_2_depth,
 * preprocess.py:1040-1044; also for the truth field);  sqrt -- conf = sqrt(var) over `count` values;  transpose -- dst (cols,
 * rows) = src (rows, cols)^T, e.g. the (modes, points) block of gprx_predict_batch_dev into reverse's (points, modes). */
int gprx_pca_to_depth_dev(gprx_pca_handle p, double* field_dev, int64_t rows, int add_elevations_first);
int gprx_pca_sqrt_dev(gprx_pca_handle p, double* field_dev, int64_t count);
int gprx_pca_transpose_dev(gprx_pca_handle p, const double* src_dev, int64_t rows, int64_t cols, double* dst_dev);
/* Mode-count sweep (run_spatial_modes, production/analysis/cross_validation.py:96-102): what gprx_metrics_dev returns for the field that
 * gprx_pca_reverse_dev, gprx_pca_to_depth_dev and gprx_pca_sqrt_dev would give with the projector cut to its first counts[j] modes, for
 * every j and every event, in one pass that writes no field.  mean_dev, var_dev (may be NULL): (rows, k) of the FULL projector;
 * truth_dev: (rows, n_cells), already in the metrics' space; events: n_events disjoint, non-empty row ranges [event_lo[i], event_hi[i])
 * (host arrays, at most 65535); counts: n_counts (1..64) strictly increasing values in [1, k] (host array); depth_mode: 0 none (velocity),
 * 1 max(y - e, 0) ("wse" models), 2 max((y + e) - e, 0) ("depth" models), both need a projector created with elevations; v_tol >= 0: the
 * fidelity index at t_tol = 0.  rows < 2^31.  Device outputs:
 *   cell_sums  (n_counts, n_events, 6, n_cells): per cell over the event's rows: sum (x-y), sum (x-y)^2, sum conf, sum |x-y|, max_t y,
 *              x at the first timestep of that maximum (what metrics.py:52-53 gathers)
 *   cell_arg   (n_counts, n_events, n_cells) int32: that timestep, counted from the event's first row
 *   truth_peak (n_events, n_cells), truth_arg (n_events, n_cells) int32: max_t x and its first timestep
 *   row_sums   (n_counts, rows, 3): per row over the cells: sum (x-y), sum (x-y)^2, sum conf (0 for rows of no event)
 * and on the host matches (n_counts, n_events).  Per cell the numbers are those of the per-count chain bit for bit; row_sums is reduced
 * in another fixed order than gprx_metrics_dev's.  The call synchronises.  GPRX_EINVAL leaves the handle usable. */
int gprx_pca_sweep_dev(gprx_pca_handle p, const double* mean_dev, const double* var_dev, int64_t rows, const double* truth_dev, int64_t n_events,
                       const int64_t* event_lo, const int64_t* event_hi, int n_counts, const int* counts, int depth_mode, double v_tol,
                       double* cell_sums_dev, int* cell_arg_dev, double* truth_peak_dev, int* truth_arg_dev, double* row_sums_dev,
                       unsigned long long* matches);
/* device milliseconds of the last gprx_pca_sweep_dev of this handle; the counts one launch of it carries */
int gprx_pca_sweep_ms(gprx_pca_handle p, double* ms);
int gprx_pca_sweep_group(void);
/* Peak ensembles: members of a predictive distribution in EOF-score space pushed through the field chain of ONE event and reduced to the
 * event's peak per (member, cell), without writing a field.  scores_dev: (members * rows_e, k), member s in rows [s rows_e, (s + 1) rows_e)
 * -- the (rows, k) layout gprx_pca_reverse_dev reads; depth_mode as for gprx_pca_sweep_dev; member_group: members a workgroup carries, 0 for
 * the launcher's choice (gprx_pca_ensemble_group), else 1..64; peak_dev: (members, n_cells).  peak[s, c] is, bit for bit and whatever the
 * grouping, the first maximum over the rows of member s of gprx_pca_reverse_dev -> gprx_pca_to_depth_dev on that member's rows.
 * members * rows_e < 2^31.  The call synchronises; gprx_pca_ensemble_ms: device milliseconds of the last one. */
int gprx_pca_ensemble_peaks_dev(gprx_pca_handle p, const double* scores_dev, int64_t members, int64_t rows_e, int depth_mode, int member_group,
                                double* peak_dev);
int gprx_pca_ensemble_ms(gprx_pca_handle p, double* ms);
/* Draws into that layout: scores[(s rows_e + t) k + kk] = mean[kk, t] + w[kk, s, t] for t < rows_e; mean_dev (k, rows_e) and the factor of
 * gprx_predict_joint_batch_dev give w_dev (k, members, tp) = Zn Lc^T through gprx_gemm_batched.  Asynchronous on the projector's stream. */
int gprx_pca_pack_scores_dev(gprx_pca_handle p, const double* mean_dev, const double* w_dev, int64_t members, int64_t rows_e, int64_t tp,
                             double* scores_dev);
int gprx_pca_ensemble_group(gprx_pca_handle p, int64_t members, int* group);
/* The standard normals of one event, generated on the device: zn_dev (k, members, tp) as gprx_gemm_batched reads it ahead of
 * gprx_pca_pack_scores_dev, k the handle's mode count.  THE ADDRESSING IS THE CONTRACT: a draw is a pure function of
 * (seed, stream, event, mode, member, row) and of nothing else -- not of k, members, rows_e, member0 or the order of the calls:
 *   Philox4x64-10 (Random123's definition, the generator of numpy.random.Philox) with counter = (t >> 2, s, kk, e) and key = (seed, stream);
 *   the draw of row t is word w = t & 3 of that block;  e = event: the event's index in the caller's list of events, kk the mode, s the
 *   ABSOLUTE member member0 + sl of slot sl;  seed and stream are unsigned 64-bit.
 *   u = ((w >> 12) + 0.5) 2^-52, never 0 or 1;  z = PPND16(u), Wichura's algorithm AS 241 with every operation rounded once (csrc/normals.h).
 * zn[kk, sl, t] is that z for t < rows_e and an exact zero for rows_e <= t < tp.  raw = 1: the 64-bit words themselves are written
 * instead (read the block as uint64_t; the padding columns are zero words).  pair_offset = h > 0 (antithetic ensembles): the absolute
 * member s >= h is the exact negation of member s - h -- the same counter, the sign bit flipped (raw: the same words); 0 switches it off.
 * members >= 1, rows_e >= 1, members * rows_e < 2^31; tp >= rows_e, tp % 64 == 0; member0 >= 0, member0 + members <= 4096; event >= 0;
 * pair_offset >= 0 and, when set, member0 + members <= 2 pair_offset; zn_dev 16-byte aligned.  GPRX_EINVAL leaves the handle usable.
 * Asynchronous on the projector's stream. */
int gprx_pca_normals_dev(gprx_pca_handle p, uint64_t seed, uint64_t stream, int64_t event, int64_t member0, int64_t members, int64_t pair_offset,
                         int64_t rows_e, int64_t tp, int raw, double* zn_dev);
/* z_dev[i] = the normal of the word words_dev[i], 0 <= i < n < 2^31, by the same transform (u, then PPND16): the way in for words that no
 * draw reaches, the far tail and the two extreme words among them.  Asynchronous on the projector's stream. */
int gprx_pca_normal_transform_dev(gprx_pca_handle p, const uint64_t* words_dev, int64_t n, double* z_dev);
/* The last step of the same result on the existing kernels: field_dev (members * rows_e, n_cells) as gprx_pca_reverse_dev and
 * gprx_pca_to_depth_dev leave it; peak_dev (members, n_cells): per member the first maximum over its rows (a NaN is the maximum, as
 * gprx_metrics_dev has it).  At most 65535 members per call.  Asynchronous on the projector's stream. */
int gprx_pca_member_peaks_dev(gprx_pca_handle p, const double* field_dev, int64_t members, int64_t rows_e, double* peak_dev);
/* Statistics over the members of peak_dev (members, n_cells), 1 <= members <= 4096, every sum in member order:
 *   exceed (n_thr, n_cells) int32: the count of peak > thresholds[j] (strict), n_thr <= 8 (host array, no NaN)
 *   mean (n_cells): the plain sum over s = 0, 1, ... divided by members;  std (n_cells): sqrt of the sum of the squared deviations from
 *     that mean (second pass, each a rounded product then a rounded addition) divided by members (ddof = 0)
 *   order (n_rank, n_cells): the order statistics np.sort(peak, axis=0)[ranks[j]], exactly; n_rank <= 8 ranks in [0, members) (host array)
 *   wet_area (members, n_thr): sum over the cells of area[c] [peak[s, c] > thresholds[j]]; area_dev (n_cells) NULL: every area 1.0, the
 *     sum is an exact count.  Fixed order (lanes of a wave, waves of a workgroup, workgroups ascending): repeated calls give the same bits.
 * exceed / wet_area may be NULL when n_thr = 0, order when n_rank = 0.  The call synchronises.  GPRX_EINVAL leaves the handle usable. */
int gprx_pca_member_stats_dev(gprx_pca_handle p, const double* peak_dev, int64_t members, int n_thr, const double* thresholds, int n_rank, const int* ranks,
                              const double* area_dev, int* exceed_dev, double* mean_dev, double* std_dev, double* order_dev, double* wet_area_dev);
/* The ensemble against the truth: peak_dev (members, n_cells) and the observed peak obs_dev (n_cells), 1 <= members = S <= 4096.  Per cell,
 * with x_(0) <= ... <= x_(S-1) the members in np.sort's order (-0 before +0, every NaN last) and y the observation:
 *   below, equal (n_cells) int32: the counts of x_s < y and of x_s == y (values compared: -0 == +0)
 *   crps (n_cells): (2 acc) / ((double)S (double)S), acc = sum over i = 0, 1, ... of |x_(i) - y| w_i in that order, w_i = (S - i) - 0.5 where
 *     x_(i) > y and i + 0.5 elsewhere, each term a rounded product followed by a rounded addition: the CRPS of the empirical distribution,
 *     mean |x - y| - 1/2 mean |x - x'|, every term non-negative; the same bits for any permutation of the members
 *   order (n_rank, n_cells): x_(ranks[j]) read out of the sorted column, n_rank <= 8 ranks in [0, members) (host array): bit for bit the
 *     order of gprx_pca_member_stats_dev
 * A cell whose observation or any member is NaN: crps = NaN, below = equal = -1, order still in the key order.  Infinite members or
 * observation follow the formula as written: |inf - inf| is a NaN, so the CRPS of such a cell is NaN while below and equal stay counts.
 * A cell's outputs depend on its own column and observation alone.  order_dev may be NULL when n_rank = 0.  The call synchronises;
 * gprx_pca_member_verify_ms: device milliseconds of the last one; gprx_pca_member_verify_tile: the consecutive cells one workgroup sorts
 * at this member count.  GPRX_EINVAL leaves the handle usable. */
int gprx_pca_member_verify_dev(gprx_pca_handle p, const double* peak_dev, const double* obs_dev, int64_t members, int n_rank, const int* ranks,
                               double* crps_dev, int* below_dev, int* equal_dev, double* order_dev);
int gprx_pca_member_verify_ms(gprx_pca_handle p, double* ms);
int gprx_pca_member_verify_tile(int64_t members, int* tile_cells);
/* Event timing of the same members (csrc/timing.h): with y[t] the value gprx_pca_ensemble_peaks_dev forms at row t of a member, thresholds
 * thr[0 .. n_thr), n_thr <= 8 (host array, no NaN), per (member, cell) in rows counted from the event's first:
 *   t_peak      = the row of the first maximum (a NaN is the maximum and sticks): np.argmax(y)
 *   duration[j] = the number of rows with y[t] > thr[j] (strict; a NaN row is not counted)
 *   arrival[j]  = the first such row, or the sentinel rows_e when there is none
 * timing_dev: int32 (members, n_maps, n_cells), n_maps = 1 + 2 n_thr: map 0 t_peak, map 1 + j duration[j], map 1 + n_thr + j arrival[j].
 * gprx_pca_ensemble_timing_dev: the walk of gprx_pca_ensemble_peaks_dev with the same arguments; it also writes peak_dev (members, n_cells),
 * bit for bit that call's, so one walk serves both.  The maps do not depend on the grouping.  rows_e <= 2^31 - 2.  The call synchronises;
 * gprx_pca_ensemble_timing_ms: device milliseconds of the last one.
 * gprx_pca_member_timing_dev: the same maps from a resident field_dev (members * rows_e, n_cells) as gprx_pca_member_peaks_dev reads it (one
 * member of the truth: the observed maps); peak_dev may be NULL.  At most 65535 members per call.  Asynchronous on the projector's stream.
 * GPRX_EINVAL leaves the handle usable. */
int gprx_pca_ensemble_timing_dev(gprx_pca_handle p, const double* scores_dev, int64_t members, int64_t rows_e, int depth_mode, int member_group, int n_thr,
                                 const double* thresholds, double* peak_dev, int* timing_dev);
int gprx_pca_ensemble_timing_ms(gprx_pca_handle p, double* ms);
int gprx_pca_member_timing_dev(gprx_pca_handle p, const double* field_dev, int64_t members, int64_t rows_e, int n_thr, const double* thresholds,
                               double* peak_dev, int* timing_dev);
/* Statistics over the members of the maps [map0, map0 + n_sel) of a timing block (members, n_maps, n_cells), 1 <= members <= 4096, whose values
 * v_s lie in [0, rows_e], 1 <= rows_e <= 2^31 - 2; every loop in member order and every result an exact integer.  Per (map, cell):
 *   cdf (n_sel, n_lev, n_cells) int32: the count of v_s <= levels[l], n_lev <= 8 (host array)
 *   n_valid (n_sel, n_cells) int32 and sum (n_sel, n_cells) int64: the members with v_s != sentinel and the sum of their values; sentinel
 *     -1: every member counts, else a value in [0, rows_e] (the arrival maps: rows_e).  The mean is the caller's one division sum / n_valid.
 *   order (n_sel, n_rank, n_cells) int32: np.sort(v, axis=0)[ranks[j]] over ALL members (the sentinel rows_e is the largest value and sorts
 *     last), n_rank <= 8 ranks in [0, members) (host array): bisection on the values, ceil(log2(rows_e + 1)) passes over the members
 *   below, equal (n_sel, n_cells) int32, with obs_dev (n_sel, n_cells) int32, the observed value of each selected map: the counts of
 *     v_s < obs and of v_s == obs; obs_dev NULL: not written (below_dev, equal_dev may be NULL)
 * cdf_dev may be NULL when n_lev = 0, order_dev when n_rank = 0.  The call synchronises.  GPRX_EINVAL leaves the handle usable. */
int gprx_pca_timing_stats_dev(gprx_pca_handle p, const int* timing_dev, int64_t members, int n_maps, int map0, int n_sel, int64_t rows_e, int sentinel,
                              int n_lev, const int* levels, int n_rank, const int* ranks, const int* obs_dev, int* cdf_dev, int* n_valid_dev,
                              int64_t* sum_dev, int* order_dev, int* below_dev, int* equal_dev);
/* Depth-frequency maps of a weighted storm catalogue (csrc/frequency.h).  The state is the caller's device block:
 * rate_dev (n_levels, n_cells) doubles and nan_dev (n_cells) int32, both zero before the first event.  levels: host array, 1 <= n_levels <=
 * 256, finite and strictly increasing (d_0 < d_1 < ...).
 * gprx_pca_freq_accumulate_dev adds one event: peak_dev (members, n_cells), 1 <= members = S <= 4096, weight finite and >= 0.  Per cell c
 * and level l, with n = #{ s : peak[s, c] > d_l } (strict; a NaN member exceeds nothing; -0 and +0 both fail > 0.0):
 *   t = (double)n / (double)S,  u = weight * t,  rate[l, c] = rate[l, c] + u     (three rounded operations, no fma)
 *   nan[c] += #{ s : peak[s, c] is NaN }
 * rate[:, c] is non-increasing in l exactly; a permutation of the members or an event of weight 0 changes no bit; a cell's state depends
 * on its own column alone; the order of the events is the caller's.  One pass over peak, counting in integers; no atomics on global
 * memory.  The call synchronises; gprx_pca_freq_ms: device milliseconds of the last accumulate.
 * gprx_pca_freq_invert_dev: aep: host array of 1 <= n_aep <= 16 targets, finite and > 0; interp 0 (linear) or 1 (step).  Per cell and target p,
 * k = #{ l : rate[l, c] >= p }:  bracket (n_aep, n_cells) int32 = k;  depth (n_aep, n_cells) = -inf where k = 0, +inf where k = n_levels, else
 * step: d_{k-1};  linear: a = r_{k-1} - p, b = r_{k-1} - r_k, f = a / b, g = d_k - d_{k-1}, depth = d_{k-1} + g * f (each operation rounded).
 * A cell with nan[c] > 0: depth NaN, bracket -1.  The call synchronises.
 * Every refusal is GPRX_EINVAL with its reason in gprx_pca_last_error; a refused call writes nothing and leaves the handle usable. */
int gprx_pca_freq_accumulate_dev(gprx_pca_handle p, const double* peak_dev, int64_t members, int n_levels, const double* levels, double weight,
                                 double* rate_dev, int* nan_dev);
int gprx_pca_freq_invert_dev(gprx_pca_handle p, const double* rate_dev, const int* nan_dev, int n_levels, const double* levels, int n_aep, const double* aep,
                             int interp, double* depth_dev, int* bracket_dev);
int gprx_pca_freq_ms(gprx_pca_handle p, double* ms);

/* ---- fitting the EOF preprocessor: PreProcessor.fit (gpras/preprocess.py:947-1007) --------------------------------------- */
/* The fitted state gprx_pca_create takes, computed on the device.  Single-batch IncrementalPCA (sklearn partial_fit, first
 * batch): 2 <= n_samples <= n_wet.  North's rule (preprocess.py:1323-1353) runs on the host between the two calls, as does
 * the eigendecomposition of the small Gram matrix.
 *
 * create: uploads x (n_samples, n_cells) once and runs
 *   - the wetness classes and the input mean: wse_2_depth (:1041-1045) for mode 1, classify_wetness_wse / _depth
 *     (:1096-1126) with _classify_depths (:1128-1133) for modes 0 / 1, every cell TF for mode 2 (:969-977); the mean of the
 *     PCA input over the wet cells (:977-980) in numpy's pairwise order over each column and one division (bit-identical to the reference's mean);
 *   - the compaction, centring and weighting (:977-986: subtract, then weight; weights: n_cells values, or NULL = none)
 *     and IncrementalPCA's own centring of that matrix (partial_fit: X -= col_mean);
 *   - the Gram matrix G = Xc Xc^T of the twice-centred matrix (fp64 MFMA, split-K slabs summed in a fixed order).
 *   mode: 0 = wse, 1 = depth, 2 = velocity (elevations may then be NULL).  Fewer wet cells than samples: GPRX_EINVAL.  Not
 *   enough device memory for x, the two compacted copies and the Gram slabs: GPRX_ENOMEM before anything is allocated. */
int gprx_pcafit_create(int device, const double* x, int64_t n_samples, int64_t n_cells, const double* elevations, const double* weights,
                       int mode, double wet_threshold, gprx_pcafit_handle* out);
/* classes (n_cells): 0 = "" (maximum exactly at the threshold, or NaN), 1 = AD, 2 = TF, 3 = AF (:1128-1133);
 * input_mean (room for n_cells, the first n_wet are written: :980); gram (n_samples, n_samples); n_wet.  G comes down from the
 * device on the first call (create itself downloads nothing of size n_samples^2); GPRX_ESTATE when the first call comes after
 * gprx_pcafit_eig or after a components call, which reuse the block that holds G. */
int gprx_pcafit_gram(gprx_pcafit_handle f, unsigned char* classes, double* input_mean, double* gram, int64_t* n_wet);
/* u (n_samples, k) row-major: the eigenvectors of G of the k largest eigenvalues lambda (k), all > 0, 0 <= k < n_samples.
 * eofs (k, n_wet) = diag(lambda^-1/2) u^T Xc with svd_flip(u_based_decision=False) applied (pca.components_[:k], :1000);
 * z (n_samples, k) = Xc_once eofs^T, the training projection whose column mean / std are x_mean / x_std (:1004-1007). */
int gprx_pcafit_components(gprx_pcafit_handle f, int k, const double* u, const double* lam, double* eofs, double* z);
/* device milliseconds of the last create / components: upload of x, statistics, centring, Gram, components, projection */
int gprx_pcafit_timings(gprx_pcafit_handle f, double* ms);
/* The same fit with the eigendecomposition on the device; the Gram matrix, its eigenvectors and its
 * eigenvalues stay in device memory.  eig: classes, input_mean, n_wet as gprx_pcafit_gram returns them; lam: the n_samples
 * eigenvalues of G, descending, unclamped (the caller clamps at 0 and divides by n_samples - 1: preprocess.py:988-1002 reads
 * explained_variance_); sweeps: Jacobi sweeps taken.  GPRX_ENOCONV when the solver does not converge.  Call order: create, eig,
 * components_dev.  GPRX_ESTATE on a second call of eig (the solver overwrites G) and when eig comes after gprx_pcafit_components
 * or components_dev (they reuse the block that holds G).  components_dev: eofs and z as gprx_pcafit_components writes them, from the k leading
 * eigenpairs held on the device; every one of those eigenvalues must be > 0, 0 <= k < n_samples; after eig only.  eig_ms: device
 * milliseconds of the eigensolver (gprx_pcafit_timings keeps its six values). */
int gprx_pcafit_eig(gprx_pcafit_handle f, unsigned char* classes, double* input_mean, double* lam, int64_t* n_wet, int* sweeps);
int gprx_pcafit_components_dev(gprx_pcafit_handle f, int k, double* eofs, double* z);
int gprx_pcafit_eig_ms(gprx_pcafit_handle f, double* ms);
/* The fit for any number of samples.  create_auto uploads x and takes the Gram route when n_samples <=
 * n_wet (and n_samples <= min(n_cells, 16384)): the handle then behaves as one from gprx_pcafit_create, bit for bit.  Otherwise it
 * takes the COVARIANCE route, the reference's IncrementalPCA on one batch of more rows than columns or on several batches: the
 * statistics with the column means in numpy's order for long columns (pieces of 8192 rows, each in its pairwise tree, added left to
 * right: input_mean stays bit-identical to the reference), compaction, the second centring and C = Xc2^T Xc2 (n_wet, n_wet), unscaled.
 * Domain of that route: 2 <= n_samples < 2^31 - 16, 1 <= n_wet <= 16384.  *route: GPRX_PCAFIT_GRAM or GPRX_PCAFIT_COV.
 *   cov: the counterpart of gprx_pcafit_gram: classes, input_mean, C and n_wet (same call-order rules).
 *   components_cov: v (k, n_wet) row-major, the eigenvectors of the k largest eigenvalues of C as rows, unflipped, 0 <= k <=
 *     min(n_samples - 1, n_wet); eofs (k, n_wet) = v with svd_flip(u_based_decision=False) applied, z (n_samples, k) = Xc_once eofs^T.
 *   gprx_pcafit_eig / components_dev serve a covariance-route handle as well: lam then has n_wet entries and the components are the
 *     leading eigenvector columns of U, gathered on the device as rows.
 * A call that does not fit the handle's route (gram / components on a covariance handle, cov / components_cov on a Gram handle)
 * returns GPRX_ESTATE with a message that names the route.  Timings: the fourth value is the covariance product on that route. */
#define GPRX_PCAFIT_GRAM 0
#define GPRX_PCAFIT_COV 1
int gprx_pcafit_create_auto(int device, const double* x, int64_t n_samples, int64_t n_cells, const double* elevations, const double* weights,
                            int mode, double wet_threshold, int* route, gprx_pcafit_handle* out);
int gprx_pcafit_cov(gprx_pcafit_handle f, unsigned char* classes, double* input_mean, double* cov, int64_t* n_wet);
int gprx_pcafit_components_cov(gprx_pcafit_handle f, int k, const double* v, double* eofs, double* z);
int gprx_pcafit_destroy(gprx_pcafit_handle f);
const char* gprx_pcafit_last_error(gprx_pcafit_handle f);

/* ---- symmetric eigensolver ------------------------------------------------------------------------
 * Eigenvalues and eigenvectors of a real symmetric fp64 matrix by parallel two-sided block Jacobi on the device, with the
 * conventions of numpy.linalg.eigh(a, UPLO="L"): only the lower triangle of the input is read, the eigenvalues ascend and column
 * i of v belongs to lam[i].  Every eigenvector is turned so that its entry of largest magnitude (lowest index on ties) is positive.
 * Two calls on the same input give the same bits.  Matrices are row-major.  Stop: off(A)_F <= n eps ||A||_F, tested before the
 * first sweep and after every sweep; 30 sweeps without it, or a non-finite entry, return GPRX_ENOCONV and write no result.
 *
 * create: a handle for matrices up to n_max x n_max, 1 <= n_max <= 16384, with its own stream; three n_max x n_max blocks of
 *   device memory (GPRX_ENOMEM before anything is allocated when they do not fit).
 * eigh: a_host (n, lda) in, lam_host (n) and v_host (n, n; may be NULL) out, all host arrays; a_host is not changed.
 * eigh_dev: the same on device buffers: a_dev (n, lda) IS OVERWRITTEN (its diagonal ends as the unsorted eigenvalues), lam_dev (n),
 *   v_dev (n, ldv); returns when the result is complete.  The work runs on the handle's own non-blocking stream: whatever wrote
 *   a_dev on another stream must have finished before the call.
 * info: Jacobi sweeps of the last call (0: the matrix was diagonal to working accuracy) and off(A)_F / ||A||_F at its end. */
int gprx_eigh_create(int device, int n_max, gprx_eigh_handle* out);
int gprx_eigh(gprx_eigh_handle h, int n, const double* a_host, int64_t lda, double* lam_host, double* v_host);
int gprx_eigh_dev(gprx_eigh_handle h, int n, double* a_dev, int64_t lda, double* lam_dev, double* v_dev, int64_t ldv);
int gprx_eigh_info(gprx_eigh_handle h, int* sweeps, double* off_rel);
int gprx_eigh_destroy(gprx_eigh_handle h);
const char* gprx_eigh_last_error(gprx_eigh_handle h);

/* ---- HmsPreProcessor: gpras/preprocess.py:1165-1320 ------------------------------------------------
 * create: x (rows, n_features), C order (fortran = 0: x[t * ld + c]) or F order (fortran = 1: x[c * ld + t]), goes up once and
 * stays on the device.  bc_idx / precip_idx: the columns of x[:, bc_mask] / x[:, precip_mask] (:1231-1232), in order, the host's
 * np.arange(n_features)[mask].  input_mean (n_features): NULL for a fit (gprx_hms_cov computes it, :1226), the fitted one for a
 * transform (:1266).  Needs rows >= 1 (a fit: 2), one precip column at least, min(rows, n_precip) <= 16384.  Not enough device memory:
 * GPRX_ENOMEM before anything is allocated. */
int gprx_hms_create(int device, const double* x, int64_t rows, int64_t ld, int64_t n_features, int fortran, const int64_t* bc_idx, int64_t n_bc,
                    const int64_t* precip_idx, int64_t n_precip, const double* input_mean, gprx_hms_handle* out);
/* The column pass and the product behind IncrementalPCA().fit(x_precip) (:1235-1236): input_mean (n_features) = x.mean(axis=0);
 * X2 = the once-centred precip block centred again by its own column mean.  route 0 (rows >= n_precip): cov (n_precip, n_precip)
 * = X2^T X2, whose eigenvectors are the components; route 1 (rows < n_precip): cov (rows, rows) = X2 X2^T, the Gram matrix. */
int gprx_hms_cov(gprx_hms_handle h, double* input_mean, double* cov, int* route);
/* Route 1 only: eofs (k, n_precip) = diag(lambda^-1/2) u^T X2 with svd_flip(u_based_decision=False) (pca.components_[:k], :1246);
 * u (rows, k) row-major eigenvectors of the Gram matrix for its k largest eigenvalues lambda (all > 0), 0 <= k < rows. */
int gprx_hms_components(gprx_hms_handle h, int k, const double* u, const double* lam, double* eofs);
/* The features [x_bc, x_precip eofs^T, avg_precip, api(avg_precip, 0.85), api(avg_precip, 1)] (:1251-1257, :1271-1277) with
 * eofs (k, n_precip); w1 / w2: the API weights k**i of the host (:1293), their first n1 / n2 entries (the rest, up to
 * window = rows, are exact zeros).  fit = 1: x_mean / x_std (n_bc + k + 3) out -- the column mean and np.std of the entries that
 * are not zero (:1260-1261); fit = 0: x_mean / x_std in, out (rows, n_bc + k + 3) = (features - x_mean) / x_std (:1280). */
int gprx_hms_features(gprx_hms_handle h, int k, const double* eofs, const double* w1, int64_t n1, const double* w2, int64_t n2, double* x_mean,
                      double* x_std, int fit, double* out);
/* device milliseconds: upload of x, column pass, covariance / Gram, components, projection, API, statistics / standardisation */
int gprx_hms_timings(gprx_hms_handle h, double* ms);
int gprx_hms_destroy(gprx_hms_handle h);
const char* gprx_hms_last_error(gprx_hms_handle h);
/* calc_antecedent_precipitation_index (:1284-1294): out[t] = sum_{i=0}^{min(t, window-1)} w[i] a[t-i], t < n, on the device;
 * w: the first n_w (<= window) weights, finite; the others are zeros (cut from the sum when a is finite).  n or window < 1:
 * GPRX_EINVAL (np.convolve raises on an empty operand). */
int gprx_api(int device, const double* a, int64_t n, const double* w, int64_t n_w, int64_t window, double* out);

/* ---- pseudo-surface low-fidelity model: gpras/preprocess.py:454-697 --------------------------------
 * RatingCurve.predict (preprocess.py:511-513): out[i] = s(x[i]), i < n, for the cubic B-spline with FITPACK's knot vector
 * knots[0..nt) (boundary knots repeated four times, 8 <= nt <= 72) and coefficients coef[0..nt-4), what
 * LSQUnivariateSpline.get_knots / get_coeffs describe (:492-496).  Arguments outside [knots[3], knots[nt-4]] are evaluated with
 * the end polynomial pieces (FITPACK's ext = 0).  NaN in, NaN out. */
int gprx_spline_eval(int device, const double* knots, int nt, const double* coef, const double* x, int64_t n, double* out);
/* The numeric state of PseudoSurfaceDataBuilder (preprocess.py:516-579): elev (n_cells) = cell_elevations, idx (n_cells) =
 * cell_interpolater (:669-674), every value in [0, n_centerline) or GPRX_EINVAL; w (n_centerline) = cl_interpolater (:667) or NULL
 * (then gprx_ps_fit_centerline / gprx_ps_set_weights before a surface); the two rating curves (:620-632) as for gprx_spline_eval,
 * nt = 0 for a handle without curves.  Not enough device memory: GPRX_ENOMEM before anything is allocated. */
int gprx_ps_create(int device, int64_t n_cells, const double* elev, const int32_t* idx, int64_t n_centerline, const double* w, const double* us_knots,
                   int us_nt, const double* us_coef, const double* ds_knots, int ds_nt, const double* ds_coef, gprx_ps_handle* out);
int gprx_ps_destroy(gprx_ps_handle h);
const char* gprx_ps_last_error(gprx_ps_handle h);
int gprx_ps_set_weights(gprx_ps_handle h, const double* w);
/* _set_centerline_interpolater (preprocess.py:643-667): over the rows with us_q > 0 or ds_q > 0 (:657),
 * w[c] = np.median((us_wse - centerline_wse[:, c]) / (us_wse - ds_wse)), c < n_centerline; centerline_wse (rows, n_centerline)
 * row-major.  np.median's semantics: a NaN ratio makes the column NaN, infinities order as the ends, an even count gives
 * (a + b) / 2.  The weights stay in the handle and come back in w.  No kept row: GPRX_EINVAL. */
int gprx_ps_fit_centerline(gprx_ps_handle h, const double* us_wse, const double* ds_wse, const double* us_q, const double* ds_q,
                           const double* centerline_wse, int64_t rows, double* w);
/* device milliseconds (waits for the handle's stream): ms[0] the kernel of the last gprx_ps_fit_centerline, ms[1] the kernel of
 * the last gprx_ps_surface_dev; 0 for what has not run */
int gprx_ps_timings(gprx_ps_handle h, double* ms);
/* get_lf_plan_data's first step (preprocess.py:587-589): the two rating curves turn the flows us_q / ds_q (T) into the boundary
 * elevations, which stay in the handle as the boundary series of the calls below; us_wse / ds_wse (T) receive them unless NULL. */
int gprx_ps_rating(gprx_ps_handle h, const double* us_q, const double* ds_q, int64_t T, double* us_wse, double* ds_wse);
/* the boundary series given directly (T each) */
int gprx_ps_set_boundaries(gprx_ps_handle h, const double* us_wse, const double* ds_wse, int64_t T);
/* interpolate_centerline (preprocess.py:634-637): out (T, n_centerline) = us - outer(us - ds, w) */
int gprx_ps_centerline(gprx_ps_handle h, double* out);
/* interpolate_surface (preprocess.py:639-641): out (rows, n_cells) = centerline[:, idx], centerline (rows, n_centerline) */
int gprx_ps_gather(gprx_ps_handle h, const double* centerline, int64_t rows, double* out);
/* get_lf_plan_data (preprocess.py:591-597) for the boundary series of the handle:
 * out[t, c] = np.maximum(np.maximum(us[t] - (us[t] - ds[t]) * w[idx[c]], elev[c]), fluvial[t, c]); fluvial (T, n_cells) is the
 * result of get_lf_fluvial_est (:601-606), or NULL (that floor is skipped).  Host buffers, staged in row slabs. */
int gprx_ps_surface(gprx_ps_handle h, const double* fluvial, double* out);
/* The same for rows [t0, t0 + rows) of the boundary series on device buffers: fluvial_dev (rows, ldf) or NULL, out_dev (rows, ldo),
 * ldf, ldo >= n_cells.  Columns [n_cells, ldo) of out are set to 0, so that out_dev can be the padded input of
 * gprx_pca_transform_dev while fluvial_dev is the output of gprx_pca_reverse_dev (ldf = n_cells).  out_dev == fluvial_dev (in place)
 * needs ldf == ldo.  Asynchronous on the handle's stream: gprx_ps_synchronize before another handle reads out_dev. */
int gprx_ps_surface_dev(gprx_ps_handle h, int64_t t0, int64_t rows, const double* fluvial_dev, int64_t ldf, double* out_dev, int64_t ldo);
int gprx_ps_synchronize(gprx_ps_handle h);
/* rows per device pass of gprx_pca_transform (the split-K plan of gprx_pca_transform_dev depends on the rows of a call, so a
 * caller of the _dev entry that wants the bits of gprx_pca_transform cuts its rows into the same slabs) */
int gprx_pca_slab_rows(gprx_pca_handle p, int64_t* rows);

/* ---- LF-to-HF mesh resampling: gpras/preprocess.py:163-174, :363-377, :433-451 ---------------------
 * The low-fidelity field on the high-fidelity cells of the two "Upskill HEC-RAS" builders, from a (T, n_src) output block of the
 * plan to (T, n_out).
 *   n_vert = 1 (RasUpskillDataBuilder, :363-377; get_hf_plan_data's gather, :173): idx (n_out) = lf_resampler / hf_resampler,
 *     out[t, j] = src[t, idx[j]]; with elev (n_out) = cell_elevations the result is floored, v < elev[j] ? elev[j] : v
 *     (:375-376: a NaN value stays, a NaN elevation never wins); weights must be NULL.
 *   n_vert = 3 (RasInterpolaterBuilder, :433-451): idx (n_out, 3) the vertices of the simplex that holds each point, as columns of
 *     src, weights (n_out, 3) its barycentric coordinates c; acc = ((0.0 + c0 z0) + c1 z1) + c2 z2, the operations of scipy's
 *     LinearNDInterpolator in their order.  With elev: out = (acc < elev || acc != acc) ? elev : acc (:449-450); without: acc.
 *     A point outside the hull (find_simplex == -1) has idx (-1, -1, -1): its acc is NaN whatever the weights say.
 * Every index lies in [0, n_src) or the call returns GPRX_EINVAL, as it does for another n_vert, n_src outside [1, 2^28] (a
 * cell's byte offset in its row is a 32-bit number on the device), n_out outside [1, 2^31 - 1024) and weights that do not go
 * with n_vert.  Not enough device memory: GPRX_ENOMEM before anything is allocated. */
int gprx_rs_create(int device, int64_t n_src, int64_t n_out, int n_vert, const int32_t* idx, const double* weights, const double* elev,
                   gprx_rs_handle* out);
int gprx_rs_destroy(gprx_rs_handle h);
const char* gprx_rs_last_error(gprx_rs_handle h);
/* get_lf_plan_data (:363-377, :433-451) on host arrays: src (T, n_src) -> out (T, n_out), staged in row slabs (device memory
 * does not grow with T).  src2 (T, n_src) or NULL: given, out = sqrt(vx vx + vy vy) of the two gathered operands, the velocity
 * magnitude of :367-373, which has no floor: it needs an n_vert = 1 handle without elevations (GPRX_EINVAL otherwise). */
int gprx_rs_apply(gprx_rs_handle h, const double* src, const double* src2, int64_t T, double* out);
/* The same for `rows` rows on device buffers: src_dev / src2_dev (rows, lds), lds >= n_src; out_dev (rows, ldo), ldo >= n_out
 * (GPRX_EINVAL otherwise, as for rows outside [0, 2^31 - 1024); the handle stays usable).  Columns [n_out, ldo) of out are set to 0, so that out_dev can be the padded
 * input of gprx_pca_transform_dev.  out_dev must not overlap the sources.  Asynchronous on the handle's stream:
 * gprx_rs_synchronize before another handle reads out_dev. */
int gprx_rs_apply_dev(gprx_rs_handle h, int64_t rows, const double* src_dev, int64_t lds, const double* src2_dev, double* out_dev, int64_t ldo);
int gprx_rs_synchronize(gprx_rs_handle h);
/* device milliseconds of the kernel of the last gprx_rs_apply_dev (waits for the handle's stream); 0 when none has run */
int gprx_rs_timings(gprx_rs_handle h, double* ms);

/* ---- per-event temporal clipping: gpras/preprocess.py:89-155 ----------------------------------------
 * DataBuilder.get_cutoff (preprocess.py:135-147) with _delta_cols_norm (preprocess.py:149-155), and the row slices that
 * _align_datasets (preprocess.py:89-116) and aligned_ref_line_df (preprocess.py:125-133) take with its result.  `combo` is 1 to 4
 * device blocks side by side that share `rows`: block b is (rows, cols[b]) with pitch ld[b] >= cols[b]; columns [cols[b], ld[b]) are
 * never read and may hold anything.  The rule, quirks included:
 *   rows before the first row that holds a NaN in any column are used (preprocess.py:138-140): T' of them;
 *   dx = |diff(combo, axis=0)|, n_c = sum_t dx[t, c] with 0 -> 1, dx /= n_c (preprocess.py:151-154);
 *   r_t = sum_c dx[t, c], r /= sum r, cum = cumsum(r) (preprocess.py:142-143);
 *   stop = argmax(cum > threshold), start = argmax(cum > 10e-4) (preprocess.py:145-146): indices of DIFFERENCE rows, used unshifted
 *   as row indices of the values; no crossing gives 0, an all-constant block (0 / 0) gives (0, 0).
 * The sums run in a fixed order (csrc/align.h) that does not depend on how the columns are cut into blocks: the same input gives
 * the same bits of the curve.  A handle owns a stream and its scratch, grown on demand (GPRX_ENOMEM before anything is allocated
 * when it does not fit). */
int gprx_al_create(int device, gprx_al_handle* out);
int gprx_al_destroy(gprx_al_handle h);
const char* gprx_al_last_error(gprx_al_handle h);
int gprx_al_synchronize(gprx_al_handle h);
/* get_cutoff (preprocess.py:135-147) over device blocks.  blocks_dev, cols, ld: host arrays of n_blocks entries (device pointers,
 * columns, pitches).  Returns once *start, *stop and *rows_used (T'; may be NULL) are on the host; curve (host, room for rows - 1
 * doubles) or NULL receives cum, T' - 1 values: what _plot_cutoff_diagnostic (preprocess.py:157-161) shows.  GPRX_EINVAL, the
 * message saying which: n_blocks outside 1..4, cols < 1, ld < cols, rows < 1, a threshold that is not finite, fewer than 2 rows, or
 * fewer than 2 rows left after the NaN trim (the reference raises ValueError from argmax of an empty sequence; *rows_used is set).
 * The handle stays usable. */
int gprx_al_cutoff_dev(gprx_al_handle h, int n_blocks, const double* const* blocks_dev, const int64_t* cols, const int64_t* ld, int64_t rows,
                       double threshold, int64_t* start, int64_t* stop, int64_t* rows_used, double* curve);
/* The same for one host matrix x (rows, cols), which is uploaded into the handle's scratch first. */
int gprx_al_cutoff(gprx_al_handle h, const double* x, int64_t rows, int64_t cols, double threshold, int64_t* start, int64_t* stop,
                   int64_t* rows_used, double* curve);
/* values[start:stop, :] of _align_datasets (preprocess.py:110-112) and of aligned_ref_line_df (preprocess.py:132) for one block:
 * dst_dev (stop - start, ldd) = rows [start, stop) of src_dev (., lds), columns [cols, ldd) set to 0.0 -- with ldd = cols rounded
 * up to a multiple of 16 dst_dev is the input of gprx_pca_transform_dev.  stop <= start copies nothing (numpy's empty slice).  The
 * caller keeps stop within the rows of src_dev.  Asynchronous on the handle's stream: gprx_al_synchronize before another handle
 * reads dst_dev.  dst_dev must not overlap src_dev. */
int gprx_al_clip_dev(gprx_al_handle h, const double* src_dev, int64_t lds, int64_t cols, int64_t start, int64_t stop, double* dst_dev, int64_t ldd);
/* ms[4]: device milliseconds of the last cutoff call by stage -- the NaN scan, the column normalisers, the row sums (with the
 * combination of the strips), the finish (waits for the handle's stream); zeros when none has run */
int gprx_al_timings(gprx_al_handle h, double* ms);

/* ---- the numerics of the diagnostic plots: gpras/utils/plotting.py:155-233, 716-859 ------------------------
 * What gen_plots (production/analysis/pipeline.py:90-210) computes inside its figures from the (T*, cells) fields that
 * pipeline.py:260-277 hands it, on fields that stay in HBM:
 *   performance_cdf (plotting.py:201-233): np.sort(np.abs(lf - hf).flatten()) (plotting.py:221-222), a device radix sort of fp64
 *     keys (csrc/diag.h), equal to np.sort BIT FOR BIT: the sorted sequence of a multiset is unique; NaN sorts last, -0.0 becomes
 *     +0.0, denormals survive;
 *   performance_scatterplot (plotting.py:155-198): the joint min and max (plotting.py:183, 191) and the sum of squares behind the
 *     rmse (plotting.py:185, 193), summed in an order fixed by n alone;
 *   map_detection_categories (plotting.py:716-859): per event the column maxima (plotting.py:765-766), the check for negative values
 *     (plotting.py:776-777), the wet threshold (plotting.py:780-781) and one category per cell (plotting.py:792-802).
 * A handle owns a stream and its workspace (the second sort buffer, the histograms, the tile counts and offsets, the chunk sums),
 * grown on demand and reused across calls.  Every call waits for its work.  Errors: GPRX_EINVAL with a message (null pointer,
 * n < 1, E < 1, a rank or an event range out of bounds), GPRX_ENOMEM, a HIP status; the handle stays usable.  No C++ exception
 * crosses the boundary (std::bad_alloc is GPRX_ENOMEM). */
int gprx_dg_create(int device, gprx_dg_handle* out);
int gprx_dg_destroy(gprx_dg_handle h);
const char* gprx_dg_last_error(gprx_dg_handle h);
int gprx_dg_synchronize(gprx_dg_handle h);
/* out_dev (n) = np.sort of the n unsigned 64-bit keys keys_dev, which are left unchanged; the two must not overlap.  1 <= n <= 2^40.
 * LSD radix sort, 8 bits per pass; a pass whose digit takes one value over all keys is skipped. */
int gprx_dg_sort_u64_dev(gprx_dg_handle h, const uint64_t* keys_dev, int64_t n, uint64_t* out_dev);
/* out_dev (n) = np.sort(np.abs(a - b).flatten()) (plotting.py:221-222) of two device arrays of n doubles, which are left
 * unchanged: the key bits(fabs(a[i] - b[i])) is built where the sort reads it. */
int gprx_dg_sort_abs_residual_dev(gprx_dg_handle h, const double* a_dev, const double* b_dev, int64_t n, double* out_dev);
/* the last sort: bit p of *executed_mask set when pass p (byte p of the key) ran; ms[2]: device milliseconds of the histogram sweep
 * and of the passes (either pointer may be NULL) */
int gprx_dg_sort_info(gprx_dg_handle h, int* executed_mask, double* ms);
/* out[j] = sorted_dev[ranks[j]], j < m: ranks and out are HOST arrays (a subsample of the curve of plotting.py:226-227); a rank
 * outside [0, n) is GPRX_EINVAL */
int gprx_dg_gather_dev(gprx_dg_handle h, const double* sorted_dev, int64_t n, const int64_t* ranks, int64_t m, double* out);
/* out[4] (host): the min and the max over both arrays (NaN when either holds one, as ndarray.min / max; plotting.py:183, 191), the sum
 * of (p - hf)^2 in the fixed order of csrc/diag.h, and n: rmse = sqrt(out[2] / out[3]) (plotting.py:185, 193) */
int gprx_dg_scatter_summary_dev(gprx_dg_handle h, const double* p_dev, const double* hf_dev, int64_t n, double* out);
/* truth_dev, pred_dev (rows, cells); event e is rows [ev_lo[e], ev_hi[e]) (host arrays, E of them).  codes_dev (E, cells) bytes:
 * 1 Detected, 2 Miss, 3 False Alarm, 4 Correct Negative (0 unless include_cn), 0 where a NaN is compared (plotting.py:792-802), of
 * the maxima over the event's rows ignoring NaN (plotting.py:765-766) with values below thr set to 0 (plotting.py:780-781).
 * *first_negative_event: the first event with a negative maximum, where the reference raises ValueError (plotting.py:776-777), else -1. */
int gprx_dg_detect_dev(gprx_dg_handle h, const double* truth_dev, const double* pred_dev, int64_t rows, int64_t cells, const int64_t* ev_lo,
                       const int64_t* ev_hi, int64_t E, double thr, int include_cn, unsigned char* codes_dev, int64_t* first_negative_event);

/* ---- storm-event selection: production/pre_processing/event_selection.py:13-257 -----------------------------
 * The first stage of the reference's workflow, EventSelection, on a long frame of (event, hour) rows that stays in HBM:
 *   _calculate_return_periods (event_selection.py:34-67): the per-event maxima of precip-cum and inflow, the block maxima over
 *     arrival_rate consecutive events, their descending sort, first-occurrence unique, the (n_blocks + 1) / rank knots, and scipy's
 *     linear interp1d with extrapolation at both ends -- every result equal to the reference's BIT FOR BIT;
 *   _select_diverse_storms (event_selection.py:148-185): the two pivots with their zero fill, an exact PCA of each (column means in a
 *     fixed order, Xc^T Xc and Xc V on the fp64 MFMA GEMM, eigh on the host or by gprx_ev_eigh), the standardised (E, 2k) score
 *     matrix and the farthest-point loop, incrementally (one launch per pick, all enqueued at once), ties to the lowest row.
 * The caller sorts once on the host: ev_rank[r] is the rank of row r's event id among the sorted unique ids, hour[r] its position inside
 * its event (the reference's cumcount, event_selection.py:153-155); the three value columns arrive in their original row order.
 * Domain: 1 <= n_events < 2^31, 1 <= n_hours <= 4096, n_events x (n_hours rounded up to 16) <= 2^28; finite values; the hours of an
 * event exactly 0 .. len - 1, every (event, hour) once: otherwise GPRX_EINVAL with a message.  A handle owns a stream and all device
 * memory; every call waits for its work.  No C++ exception crosses the boundary. */
int gprx_ev_create(int device, int64_t rows, int64_t n_events, int64_t n_hours, const int32_t* ev_rank, const int32_t* hour, const double* precip_excess,
                   const double* precip_cum, const double* inflow, gprx_ev_handle* out);
/* a handle without a frame: it serves gprx_ev_farthest on a caller's score matrix only */
int gprx_ev_create_empty(int device, gprx_ev_handle* out);
int gprx_ev_destroy(gprx_ev_handle h);
const char* gprx_ev_last_error(gprx_ev_handle h);
int gprx_ev_synchronize(gprx_ev_handle h);
/* host outputs, any of them NULL: the maxima over each event's own hours (the zero fill does not enter: a negative maximum survives)
 * and the number of hours of each event */
int gprx_ev_maxima(gprx_ev_handle h, double* max_precip_cum, double* max_inflow, int32_t* lengths);
/* fits both return-period functions and evaluates each at its own maxima: rp_* (n_events) host outputs (may be NULL), n_knots[2] the
 * numbers of distinct block maxima.  Fewer than two distinct block maxima: GPRX_EINVAL (interp1d needs two knots). */
int gprx_ev_return_periods(gprx_ev_handle h, int64_t arrival_rate, double* rp_precip_cum, double* rp_inflow, int64_t* n_knots);
/* out[i] = the fitted function `which` (0 precip-cum, 1 inflow) at values[i], n host doubles: scipy's interp1d._call_linear operation
 * for operation, so values below the lowest and above the highest knot extrapolate as the reference does */
int gprx_ev_rp_eval(gprx_ev_handle h, int which, const double* values, int64_t n, double* out);
/* which: 0 the precip-excess pivot, 1 the inflow pivot.  mean (n_hours) and cov (n_hours, n_hours) = Xc^T Xc, not yet divided by
 * n_events - 1: host outputs.  The covariance also stays on the device for one gprx_ev_eigh. */
int gprx_ev_cov(gprx_ev_handle h, int which, double* mean, double* cov);
/* eigh of the covariance of the last gprx_ev_cov by the device solver (gprx_eigh_dev's kernels): lam (n_hours) ascending, v (n_hours,
 * n_hours) eigenvectors in columns, host outputs; *sweeps may be NULL.  GPRX_ENOCONV as gprx_eigh_dev. */
int gprx_ev_eigh(gprx_ev_handle h, double* lam, double* v, int* sweeps);
/* the scores Xc V of block `which`: components (k, n_hours) host, one component per row with its sign already chosen; 2k <= 64 */
int gprx_ev_scores(gprx_ev_handle h, int which, int k, const double* components);
/* both score blocks side by side, (n_events, 2k), each column standardised with the population standard deviation in a fixed order
 * (scale 1 for a constant column); scores_out host, may be NULL.  The matrix stays on the device for gprx_ev_farthest. */
int gprx_ev_standardise(gprx_ev_handle h, double* scores_out);
/* The farthest-point loop on the rows of scores_dev (n, d) row-major on the device, or of the handle's standardised scores when it is
 * NULL (then n = n_events, d = 2k).  selected: n_selected distinct rows (host); num picks, each the candidate whose squared distance
 * to its nearest selected row (direct differences, summed over the columns in order) is largest, the lowest row on a tie.  picks
 * (num) in pick order and pick_dist (num), the square root of that distance: host outputs.  2 <= n < 2^31, d <= 64,
 * 1 <= n_selected, 1 <= num <= n - n_selected. */
int gprx_ev_farthest(gprx_ev_handle h, const double* scores_dev, int64_t n, int d, const int32_t* selected, int64_t n_selected, int64_t num, int32_t* picks,
                     double* pick_dist);
/* ms[8], device milliseconds of the last call of each stage: upload + pivot + maxima, return periods, covariance of block 0 and of
 * block 1, scores (both blocks), standardisation, selection, device eigh */
int gprx_ev_timings(gprx_ev_handle h, double* ms);

/* ---- fused error metrics over two fields: SURVEY.md section 8(f) row N3 (gpras/metrics.py:85-318) ---------- */
/* Two streaming passes over x (truth), y (prediction) and conf (may be NULL), each (rows, cells) row-major, yield every
 * reduction the reference's metric functions need:
 *   row_sums  (rows, 4): per timestep, over cells: sum (x-y), sum (x-y)^2, sum conf, sum |x-y|
 *   cell_sums (5, cells): per cell, over timesteps: sum (x-y), sum (x-y)^2, sum conf, max_t x, max_t y
 *   cell_arg  (2, cells): first timestep of the maximum of x and of y (numpy argmax semantics, metrics.py:35-36)
 *   matches: number of (t, cell) pairs counted by the fidelity index with lag tolerance t_tol (0..8) and value tolerance
 *            v_tol (metrics.py:187-197). */
int gprx_metrics(int device, const double* x, const double* y, const double* conf, int64_t rows, int64_t cells, int t_tol, double v_tol,
                 double* row_sums, double* cell_sums, int* cell_arg, unsigned long long* matches);
/* same with device-resident fields and outputs (matches is a host pointer; the call synchronises) */
int gprx_metrics_dev(int device, const double* x_dev, const double* y_dev, const double* conf_dev, int64_t rows, int64_t cells, int t_tol,
                     double v_tol, double* row_sums_dev, double* cell_sums_dev, int* cell_arg_dev, unsigned long long* matches);

/* ---- k-means inducing-point initialisation: SURVEY.md section 8(f) row N4 (gpras/gpr.py:312-315) ---------------------- */
/* The Lloyd iterations of KMeans(n_clusters=M, random_state=0, n_init="auto").fit(x) (scikit-learn's
 * _kmeans_single_lloyd) on the device.  x: (n, d) host, already centred (KMeans subtracts the column means); centers: (m, d)
 * host, in: the k-means++ seeding (host: sklearn.cluster.kmeans_plusplus on RandomState(0), as KMeans draws it), out: the
 * final centres (still centred); tol: absolute (mean(var(x)) * 1e-4); labels: n values out; n_iter: iterations run.
 * Stops like scikit-learn: labels repeat (strict convergence) or sum of squared centre shifts <= tol, at most max_iter.
 * *empty = 1 when a cluster lost all members (scikit-learn relocates it; centres / labels are then undefined and the
 * caller falls back to scikit-learn).  d <= 64. */
/* k-means++ seeding of the same KMeans call on the device (sklearn.cluster._kmeans._kmeans_plusplus behind gpr.py:313).  The host
 * keeps the RandomState(0) draws, which do not depend on the data: first_id = random_state.choice(n), uniforms = (m - 1) x trials
 * values of random_state.uniform(size=trials) with trials = 2 + int(log(m)).  x: (n, d) host, already centred; xsq: its squared row
 * norms (sklearn.utils.extmath.row_norms).  indices_out: the m chosen rows of x.  Candidate distances, the running minimum, the
 * potentials and the cumulative-sum search run on the device. */
int gprx_kmeans_pp(int device, const double* x, int64_t n, int d, const double* xsq, int m, int trials, int64_t first_id, const double* uniforms,
                   int64_t* indices_out);
int gprx_kmeans_lloyd(int device, const double* x, int64_t n, int d, double* centers, int m, double tol, int max_iter, int32_t* labels,
                      int* n_iter, int* empty);

/* out[c] = field[idx[c], c] for a device-resident field (rows, cells): the gathers x[x_mts, np.arange(x.shape[1])] that
 * every *_mts function of the reference performs (gpras/metrics.py:119-121, 133-135, 147-151, 167-171, 215-224, ...) when
 * the CALLER supplies the timesteps (x_mts / y_mts), as export_metric_summary does at metrics.py:46-57.  idx: cells host
 * values; negative values count from the end as in numpy; an index outside [-rows, rows) gives GPRX_EINVAL (numpy raises
 * IndexError).  out: cells host values. */
int gprx_gather_rows(int device, const double* field_dev, int64_t rows, int64_t cells, const int64_t* idx, double* out);

/* Tuning of the Cholesky schedule; value 0 restores the default.  gprx_set_tuning changes the PROCESS DEFAULTS: they
 * are read by the handle-less building blocks (gprx_potrf) and COPIED into a handle when it is created, so a handle never
 * sees a later change (handles on different host threads do not share mutable tuning state); gprx_set_handle_tuning changes
 * one handle's copy.  Set process defaults before creating handles, from one thread.  Keys:
 * "outer_block" (multiple of 128), "update_tile" (64 | 128: workgroup tile of the bulk trailing update), "no_lookahead"
 * (1: single stream), "split_panel" (1: always one diagonal workgroup + a rows-only kernel per panel, -1: never; default: from
 * 24 cells per launch on).
 * "cell_kernel" (1: batched cells always take the one-workgroup-per-cell factorisation, -1: never; default by size, see
 * gprx_factorize_batch).
 * "rhs_vector" (-1: batched cells always carry their right-hand side as a 64-row tile below the matrix, as single calls do; default 0:
 * as a vector wherever the split panel runs -- potrf_rows_kernel<..., YVEC>; see gprx_factorize_batch).
 * "rows_pair" (batched cells under the split panel; 1, the default: the rows below a pair of panels are solved by ONE launch,
 * potrf_rows_pair_kernel, which reads the left panel's solved rows back through the L2; 0: one rows launch per panel.  The factor is the
 * same bit for bit; with the right-hand side as a vector, 64 entries of y per pair are updated in another summation order).  The probe
 * gprx_potrf_batched reads this key from the process defaults.
 * "dag" (1: ONE matrix is factored by the tile-DAG kernel -- a single persistent launch, the dependent chain of diagonal
 * blocks in one workgroup, every other tile task claimed from a queue and ordered by per-tile version counters in device memory;
 * deterministic, within rounding of the default; default 0 = the launch-per-panel schedule, which measured faster on MI355X:
 * DESIGN.md section 3.2b).  Applies to EAGER single factorisations only (gprx_factorize / gprx_objective): the graph replays of
 * gprx_factorize_many and every batched call always run the launch-per-panel schedule.
 * "poison_workspace" (testing, 1: the L^-1 workspace of the gradient starts as NaN patterns instead of whatever it held -- the
 * gradient never depends on its old contents, and no longer zeroes it).
 * Every schedule gives the same factor up to rounding; fused and split panels are bit-identical.
 * "predict_path": 0 choose (default), 1 always the triangular GEMM against L^-1, 2 always blocked forward substitution.
 * "sgpr_fused": 1 (default) sparse models with M <= 64 take the five-launch evaluation and the device-resident Adam loop, 0: the
 * general launch sequence (gprx_objective_batch); a handle's cell blocks are rebuilt when its value changes.
 * "sgpr_resident": 1 (default) the optimiser loops of sparse models with d <= 64 (gprx_adam_batch, gprx_adadelta_batch) stay on the
 * device, 0: the host-stepped loop for every sparse model -- one process can run both routes (gprx_last_optimizer_route).
 * "held_general" (gprx_set_handle_tuning only; default 0): 1: the four gprx_*_held calls also serve sparse handles with d <= 64 on the
 * GENERAL launch sequence -- m > 64, and m <= 64 with "sgpr_fused" = 0 -- whose Kuf build, stage-in and step kernel then read the hold
 * table (csrc/sgpr_held.hip); 0: they refuse such handles, as described at gprx_objective_batch_held.
 * "sgpr_groups_from" (process-wide): the device-resident Adam loop runs a batch of at least this many cells (stated at N = 4096, i.e.
 * 16 chunks of 256 training points per cell: the criterion is cells x chunks > 16 (value - 1), a pass that needs a second round of the
 * CUs) as two groups of cells on two streams, one launch apart, so that one group's one-workgroup-per-cell launches overlap the
 * other's streamed passes (default 17; 1: always; 0: never; every cell's values are the same bits either way).
 * "wait_handover_us" (process-wide): microseconds of polling after which a wait hands over to hipStreamSynchronize (default
 * 200 000; tests set 0 to force the hand-over).
 * "loeo_blocked_potrf" (process-wide, a measurement aid of gprx_loeo_batch_blocked; -1, the default, keeps the schedule fixed per
 * mp): the schedule of chol(H) over the slots -- 0 launch sequence with the fused panel, 1 with the split panel, 2 one workgroup per
 * slot (not at mp = 64).
 * "pcafit_rowsplit" (process-wide, the yardstick of the covariance route of the EOF fit; a fit handle does all of its device work
 * inside gprx_pcafit_create_auto, which reads the value when it runs): 1 (default) the statistics, the compaction and the second
 * centring of that route run the row-split kernels of csrc/pca_fit_tall.h, 0: the one-thread-per-cell kernels of the Gram route on
 * the same chunked operation list.  Same bits either way. */
int gprx_set_tuning(const char* key, int value);
int gprx_set_handle_tuning(gprx_handle h, const char* key, int value);

/* The device exponentials on an array of HOST values (parity tests): which = 0: the kernel-matrix build's exp (2^(j/64) table in LDS +
 * degree-5 polynomial, arguments <= 0), which = 1: the degree-13 form the gradient passes use.  x, out: n host doubles. */
int gprx_exp_probe(int device, int which, const double* x, int64_t n, double* out);

/* measured back-to-back v_mfma_f64_16x16x4_f64 rate of the whole chip, TFLOP/s */
int gprx_mfma_f64_peak(int device, double* tflops);

#ifdef __cplusplus
}
#endif
#endif /* GPRX_H */
