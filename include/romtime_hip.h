/*
 * romtime_hip.h -- C ABI of libromtime_hip.so (MI355X / gfx950).
 *
 * The reference (KikeM/romtime @ v0) has no FFI layer: its "operator API" is a
 * Python class surface over NumPy/SciPy calls.  Each entry point
 * below replaces one of those library call sites; the citation is the
 * reference file:line (relative to /root/reference) it stands in for.
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer (hipMalloc'ed or a torch CUDA
 *     tensor's data_ptr()); f64 = double, indices = int64_t;
 *   - work is enqueued on the ctx's stream (rt_ctx_set_stream) and the call
 *     returns without synchronising unless stated;
 *   - return value: 0 ok, <0 argument / runtime error (rt_last_error has the
 *     text), >0 numerical warning (RT_WARN_*); nothing throws;
 *   - the caller owns all buffers; a ctx owns a scratch arena that grows on
 *     demand (hipMalloc: not capturable on first use);
 *   - one ctx per host thread; calls on one ctx are serialised by its stream.
 */
#ifndef ROMTIME_HIP_H
#define ROMTIME_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ctx rt_ctx;

#define RT_OK 0
#define RT_ERR_ARG (-1)
#define RT_ERR_HIP (-2)
#define RT_ERR_UNSUPPORTED (-3)
#define RT_WARN_ZERO_NORM 1   /* zero-norm column in orth(normalize=True), pod.py:32-33 yields NaN */
#define RT_WARN_SINGULAR 2    /* zero pivot in a dense solve */

#define RT_ROW_MAJOR 0        /* element (i,j) at p[i*ld + j]  (NumPy C order)  */
#define RT_COL_MAJOR 1        /* element (i,j) at p[j*ld + i]  (NumPy F order; np.array(list_of_vectors).T, deim.py:384) */

int rt_version(void);
int rt_ctx_create(rt_ctx** out, int device);
void rt_ctx_destroy(rt_ctx* ctx);
int rt_ctx_set_stream(rt_ctx* ctx, void* hip_stream);
int rt_ctx_synchronize(rt_ctx* ctx);
const char* rt_last_error(rt_ctx* ctx);
/* dispatch statistics of the most recent GEMM-class launch: [0]=grid, [1]=splits, [2]=tile */
int rt_last_launch_info(rt_ctx* ctx, int64_t* info3);

/* Measurement: when on, every GEMM-class call brackets its main MFMA kernel (not the slab
 * reduction) with hipEvents on the ctx stream; rt_last_gemm_ms synchronises on the second event
 * and returns that kernel's duration in milliseconds. */
int rt_ctx_set_profile(rt_ctx* ctx, int on);
/* Named switches.  "eig_one_xcd" (default 1): the small eigensolver may place its cooperating workgroups on one
 * XCD and hand off through that XCD's L2 (placement is verified on the device); it needs every CU of that XCD,
 * so processes that share a GPU turn it off (a hand-off timeout of rt_sym_eig_values is the symptom).
 * "eig_xcd" (default 0, 0 .. 7): the XCD that form puts its workgroups on.  Contexts with different values (each on
 * a stream of its own) run their eigensolves side by side - eight small PODs at a time, romtime_amd.pipeline.PodLanes;
 * two eigensolves in flight on the SAME XCD would starve each other of CUs (they end in the hand-off's time-out).
 * "sweep_graph" (default 0): rt_hrom_bdf_sweep captures one time step as a hipGraph (its kernels read the step from a
 * device counter) and replays it for steps 1 .. nt-1 instead of launching two kernels per step; for hosts that
 * cannot keep ahead of the device.  The call then returns only when the sweep has finished.  Ignored while the ctx's
 * reduced solver is RT_SOLVER_GMRES (rt_ctx_set_reduced_solver): the launches are then eager.
 * "pod_blocked" (default 0): rt_pod_orth takes snapshot sets of 2049 .. 16384 columns through rt_sym_eig_blocked at
 * level 0 and at every deflated level, instead of returning RT_ERR_UNSUPPORTED. */
int rt_ctx_set_option(rt_ctx* ctx, const char* name, int value);
/* "cu_limit" (default 0 = the device's CU count; a multiple of 8): the number of CUs this ctx sizes its persistent grids
 * for - set it on a ctx whose stream is CU-masked (below) so that, e.g., the snapshot Gram kernel launches exactly the
 * workgroups its share of the chip holds.
 * "gram_pace" (default 1): the workgroups of an XCD in the snapshot Gram kernel keep within two stages of each other
 * (a progress word per XCD, bounded naps for leaders), so that the tiles sharing a panel read it from the L2 while it is
 * still there: L2<-fabric reads of the off-diagonal launch 10.4 -> 4.13 GB on 1e6 x 512 at no cost in time on the whole
 * chip; 0 switches it off (the POD pipeline does, for the Gram on its 224-CU stream: +2 % there). */

/* CU-partitioned streams (throughput mode of the POD: the n x n eigensolve of one snapshot set runs beside the Gram
 * kernel of the next on disjoint CUs).  Creates a HIP stream whose kernels run only on CUs [first, first + count) of
 * EVERY XCD (MI355X: 32 CUs per XCD; a mask must leave no XCD empty).  *stream is a hipStream_t for rt_ctx_set_stream. */
int rt_stream_create_cu_range(int device, int first_cu_per_xcd, int n_cu_per_xcd, void** stream);
int rt_stream_destroy(void* stream);
int rt_last_gemm_ms(rt_ctx* ctx, double* ms);
/* Event counters kept on the device by the kernels themselves (nothing on the hot path waits for them); reading one
 * synchronises the ctx stream.  Names: "eig_timeouts" (hand-offs of the small eigensolver that hit their wall-clock
 * bound: results of that call were invalid and the caller took another route), "eig_one_xcd" / "eig_general_form"
 * (tridiagonalisations that ran each hand-off form), "eig_wide_form" (tridiagonalisations of 1024 < n <= 2048, which hand
 * nothing off: every dependency is a kernel boundary), "gram_off_xcd" (workgroups of the snapshot Gram kernel that ran on
 * another XCD than the one their K range was laid out for: should stay 0), "sweep_newton_iterations", "sweep_restarts",
 * "sweep_lu_fallbacks", "sweep_solves" (the four numbers of rt_last_sweep_stats), "sweep_gmres_iterations" (GMRES inner
 * iterations of the most recent sweep, RT_SOLVER_GMRES), "sweep_gmres_unconverged" (its systems that GMRES left with
 * info != 0).  All six sweep counters are zeroed at the start of every sweep, whatever its solver.  "eig_blocked" /
 * "eig_blocked_not_reducible" (rt_sym_eig_blocked calls that ended with status 0 / status 1) and "eig_blocked_rank" (R of
 * the most recent of those calls: a value, not a count). */
int rt_ctx_get_counter(rt_ctx* ctx, const char* name, int64_t* value);
/* The same for the most recent launch of the snapshot Gram kernel (rt_gram, n >= 97, long X): its own event pair,
 * so it can be read at the end of a POD step, after the GEMMs that followed it, without holding the host back. */
int rt_last_gram_ms(rt_ctx* ctx, double* ms);
/* Which form rt_gram takes for an n_rows x n_cols snapshot set on num_cus compute units (host logic only, no GPU needed:
 * diagnostics and the CPU-side tests): out[0] = 0 the generic symmetric GEMM, 1 two launches (out[3] / out[4] sub-splits
 * per off-diagonal / diagonal tile and XCD), 2 one launch with uniform slots (out[1] / out[2] per tile) whose paced
 * workgroups read the snapshots once. */
int rt_gram_plan_info(int num_cus, int64_t n_rows, int64_t n_cols, int* out);
/* The slot plan of one launch of the two-launch form (since version 430; host logic only): launch 0 the off-diagonal
 * tiles, 1 the diagonal ones, for the row range of XCD xcd (0..7).  out[0] = tiles of the launch, out[1] = regular slots
 * per tile (stage q, q + out[1], ... below out[4]), out[2] = spare slots in use (0: the plain launch), out[3] = most tails
 * per spare slot (spare slot j takes the stages [out[4], out[5]) of out[0] / out[2] consecutive tiles, the first
 * out[0] % out[2] spare slots one tile more), out[4] = n_main, out[5] = 16-row stages of the range.  RT_ERR_UNSUPPORTED
 * where rt_gram_plan_info gives another form or the launch has no tile. */
int rt_gram_spare_plan_info(int num_cus, int64_t n_rows, int64_t n_cols, int launch, int xcd, int* out);

/* ---- POD (src/romtime/rom/pod.py:7-62) ------------------------------------------------ */

/* G = X^T X (n_cols x n_cols, row-major, full symmetric).  X is n_rows x n_cols with
 * leading dimension ld in the given layout.  This is the local part of the snapshot
 * Gram matrix: with row-sharded X the caller all-reduces G (RCCL) before rt_gram_scale.
 * Replaces the O(N n^2) part of scipy.linalg.svd(..., lapack_driver="gesvd") (pod.py:38). */
int rt_gram(rt_ctx* ctx, const double* X, int64_t n_rows, int64_t n_cols, int64_t ld, int layout,
            double* G);

/* colnorm[j] = sqrt(G[j][j]) (== np.linalg.norm(X, axis=0), pod.py:32); if normalize != 0,
 * G <- D^-1 G D^-1 (the Gram matrix of np.divide(X, l2_norms), pod.py:33).  A zero norm
 * propagates NaN exactly as the reference does and *status_flag (device int, may be NULL)
 * is set to RT_WARN_ZERO_NORM. */
int rt_gram_scale(rt_ctx* ctx, double* G, int64_t n, double* colnorm, int normalize, int* status_flag);

/* The whole of `orth` (pod.py:7-62) in one call, for hosts that bind this library without the Python layer: column
 * norms (normalize != 0), Gram matrix, all singular values, energy curve, truncation with the reference's precedence
 * (tol != 0: energy < tol, strict; else num != 0: first num; else sigma > 1e-7), basis.  X: n_rows x n_cols DEVICE matrix
 * (ld, layout), n_cols <= 2048 (RT_ERR_UNSUPPORTED beyond; with the ctx option "pod_blocked" n_cols <= 16384, every level's
 * eigensolve through rt_sym_eig_blocked, and RT_ERR_UNSUPPORTED where that reports a set that is not reducible).  Q: DEVICE buffer n_rows x q_cols row-major; on return its first *r_out columns are the
 * basis (the others are zero or unspecified); if the rule keeps more than q_cols modes the call returns RT_ERR_ARG with
 * *r_out = the number needed.  s_host / energy_host: HOST arrays of min(n_rows, n_cols) entries - ALL singular values and
 * the whole energy curve, as the reference returns them.  *levels_out (may be NULL): Gram passes taken (1 = single pass;
 * more = deflated levels for spectra deeper than 1e-2).  Returns RT_WARN_ZERO_NORM (and no basis) where
 * the reference raises on a zero-norm snapshot with normalize.  Synchronises the ctx stream (the truncation rule needs
 * the spectrum on the host).  Single device: a row-sharded host sums the Gram matrices itself and uses the pieces below. */
int rt_pod_orth(rt_ctx* ctx, const double* X, int64_t n_rows, int64_t n_cols, int64_t ld, int layout, int64_t num,
                double tol, int normalize, double* Q, int64_t q_cols, int64_t* r_out, double* s_host,
                double* energy_host, int* levels_out);

/* One single-pass POD, ENQUEUED on the ctx stream and not waited for: Gram matrix, scaling, all eigenvalues, the k
 * leading eigenvectors, back-projection Q (n_rows x k, row-major) = X D^-1 W S^-1.  The decisions `orth` takes from the
 * spectrum (deflated levels for deep spectra, Rayleigh-Ritz for clusters, the zero-norm error) are the caller's, after
 * the fact: lam (n_cols, descending, device), status2 (device ints: [0] eigensolver hand-off status, [1] zero-norm
 * flag), colnorm (n_cols).  G (n x n), Z and Zs (n x k) are work space the caller owns; 3 <= n_cols <= 1024, k <= n_cols.
 * One host call per snapshot set:
 * what lets romtime_amd.pipeline.PodLanes keep eight small PODs on the chip (eight contexts, "eig_xcd" 0 .. 7). */
int rt_pod_enqueue(rt_ctx* ctx, const double* X, int64_t n_rows, int64_t n_cols, int64_t ld, int layout, int64_t k,
                   int normalize, double* G, double* colnorm, double* lam, int* status2, double* Z, double* Zs, double* Q);

/* Zs (n x k row-major) = D^-1 W S^-1: W = Z (n x k eigenvectors of the Gram matrix, rt_sym_eig_vectors), D = diag(colnorm)
 * (NULL: identity, normalize == False), S_j = sqrt(lam_j) (device eigenvalues; S^-1 = 0 where lam_j <= 0).  The matrix the
 * back-projection Q = X Zs multiplies (pod.py:33,38 combined); one launch, no host data. */
int rt_pod_backproject_weights(rt_ctx* ctx, const double* Z, int64_t n, int64_t k, const double* colnorm, const double* lam,
                               double* Zs);

/* C (m x n, row-major, ldc) = A^T B with A: N x m, B: N x n (each with ld + layout).
 * np.matmul(V.T, AhV) (utils.py:112), np.matmul(V.T, Vfh) (deim.py:509), V.T.dot(f)
 * (rom.py:133,156).  A == B with m == n computes only the upper triangle and mirrors it. */
int rt_gemm_tn(rt_ctx* ctx, const double* A, int64_t lda, int a_layout, const double* B, int64_t ldb,
               int b_layout, int64_t N, int64_t m, int64_t n, double* C, int64_t ldc);

/* Y (N x k, ldy, y_layout) = X (N x n, ldx, x_layout) * T (n x k, row-major, ldt).
 * The POD back-projection U_r = X (D^-1 W_r S_r^-1) and V.dot(uN) (rom.py:111-112). */
int rt_gemm_nn(rt_ctx* ctx, const double* X, int64_t ldx, int x_layout, const double* T, int64_t ldt,
               int64_t N, int64_t n, int64_t k, double* Y, int64_t ldy, int y_layout);
/* Y = beta Y + alpha X T, same operands.  The deflation of the multi-level POD, X <- X - Q (Q^T X), in place
 * (Gram-Schmidt sweep between the levels; the reference gets deep spectra from dgesvd itself, pod.py:38). */
int rt_gemm_nn_axpby(rt_ctx* ctx, const double* X, int64_t ldx, int x_layout, const double* T, int64_t ldt,
                     int64_t N, int64_t n, int64_t k, double alpha, double beta, double* Y, int64_t ldy,
                     int y_layout);

/* Thin update of a tall row-major matrix: Y_dst (N x n) = Y_src diag(colscale) + alpha X (N x k) T (k x n), k <= 64
 * (RT_ERR_UNSUPPORTED above), colscale optional (NULL = 1), Y_src == Y_dst allowed.  The deflation sweep
 * X <- X - Q (Q^T X) of the levelled POD (romtime_amd/pod.py; replaces what dgesvd's bidiagonalisation does
 * implicitly in rom/pod.py:38); HBM-bound streaming kernel. */
int rt_rank_update(rt_ctx* ctx, const double* Ysrc, int64_t ldys, const double* colscale, const double* X, int64_t ldx,
                   const double* T, int64_t ldt, int64_t N, int64_t k, int64_t n, double alpha, double* Ydst,
                   int64_t ldyd);

/* Out-of-place transpose: dst (cols x rows, row-major, ld_dst) = src (rows x cols, row-major, ld_src)^T. */
int rt_transpose(rt_ctx* ctx, const double* src, int64_t rows, int64_t cols, int64_t ld_src, double* dst,
                 int64_t ld_dst);

/* ---- DEIM (src/romtime/deim/deim.py:517-561, :159, :212) -------------------------------- */

/* Greedy interpolation-index selection on the collateral basis Phi (N x m).
 * idx[k] = argmax_i |phi_k - Phi[:, :k] c|, c = solve(Phi[idx[:k], :k], phi_k[idx[:k]]),
 * first maximum on ties (np.argmax, deim.py:531,553).  PT_U (m x m row-major) = Phi[idx, :]
 * (np.matmul(P.T, basis), deim.py:159,212).  margin (m, may be NULL) = (top1-top2)/top1 of
 * |residual| per step.  Synchronises the stream before returning. */
int rt_deim_greedy(rt_ctx* ctx, const double* Phi, int64_t N, int64_t m, int64_t ld, int layout,
                   int64_t* idx, double* PT_U, double* margin);

/* One selection step of oversampled (M)DEIM, since version 450: more entries than modes, least squares in place of
 * interpolation (gappy POD).  The rule is GappyPOD+E (Peherstorfer, Drmac, Gugercin, SIAM J. Sci. Comput. 42, 2020; the
 * reference stops at m entries for m modes, deim.py:517-561).  With A = Phi[p, :] the rows picked so far, the host takes
 * the thin SVD of A and hands over w (m DEVICE doubles), the right singular vector of the smallest singular value, and
 * g = sigma_{m-1}^2 - sigma_m^2 (HOST double).  For every row i of Phi (N x m, ld and layout as for rt_deim_greedy)
 *     rho_i = ||Phi[i, :]||^2,  c_i = Phi[i, :] . w,  a_i = g + rho_i,  q_i = 4 g c_i^2,
 *     score_i = q_i / (a_i + sqrt(max(a_i^2 - q_i, 0)))   (0 where q_i = 0),
 * half of which is a lower bound on the growth of sigma_min^2 when row i joins.  pick (one DEVICE int64) = the argmax over the rows whose
 * byte in taken (N DEVICE bytes) is zero, the lowest index on ties, -1 when every row is taken; top2 (two DEVICE doubles)
 * = the best score and the runner-up among those rows, -1 where there is none.  g = 0 gives all scores 0 and the lowest
 * free index.  Enqueued on the ctx stream and not waited for.
 *   - One pass over Phi (8 N m bytes): rho and c come from the row while it is in registers, nothing of size N is stored.
 *     The sums of a row run in a fixed order that depends on the layout and m alone; workgroups of 512 rows reduce to
 *     (top1, index, top2) in the order (score descending, index ascending) and a second launch of one workgroup merges the
 *     partials (ctx leaf arena).  No floating-point atomics; the grid depends on N alone, so pick and top2 have the same
 *     bits on any CU share ("cu_limit").
 *   - A null pointer, N < 1, m < 2, a short ld, an unknown layout and a g that is negative or not finite return
 *     RT_ERR_ARG; m > 1024 or N > 512 (2^31 - 1), beyond what rt_deim_greedy takes, RT_ERR_UNSUPPORTED; all before any launch.
 *   - rt_last_launch_info: [0] workgroups, [1] lanes per row (1: column-major), [2] 512 rows per workgroup (512000). */
int rt_deim_oversample_step(rt_ctx* ctx, const double* Phi, int64_t N, int64_t m, int64_t ld, int layout, const double* w,
                            double g, const uint8_t* taken, int64_t* pick, double* top2);
/* The argument checks and the launch plan of rt_deim_oversample_step - host logic only, no GPU and no pointer is followed:
 * the same return code, and on RT_OK info3 (may be NULL) = {workgroups, rows per workgroup, lanes per row}. */
int rt_deim_oversample_step_plan_info(const double* Phi, int64_t N, int64_t m, int64_t ld, int layout, const double* w, double g,
                                      const uint8_t* taken, const int64_t* pick, const double* top2, int64_t* info3);

/* ---- projections (src/romtime/utils.py:96-113,136-149; deim/mdeim.py:153-192) ----------- */

/* Y (N x r row-major, ldy) = A V, A in CSR (N rows), V (n_colsA x r row-major, ldv).
 * scipy.sparse.csr_matrix.dot(dense) (utils.py:111). */
int rt_csr_spmm(rt_ctx* ctx, const int64_t* indptr, const int64_t* indices, const double* data, int64_t N,
                const double* V, int64_t ldv, int64_t r, double* Y, int64_t ldy);

/* AN (r x r row-major) = V^T (A V)   (project_csr, utils.py:96-113). */
int rt_project_csr(rt_ctx* ctx, const int64_t* indptr, const int64_t* indices, const double* data, int64_t N,
                   const double* V, int64_t ldv, int64_t r, double* AN);

/* Batched over B value-vectors on one fixed CSR pattern: data_batch holds B value vectors,
 * vector b at data_batch + b*ld_data (stride 1) when data_layout == RT_COL_MAJOR, or element
 * e of vector b at data_batch[e*ld_data + b] when RT_ROW_MAJOR (the (nnz x m) basis_fom array
 * in C order).  AN_batch is B x r x r.  MDEIM.project_basis (mdeim.py:153-192) with
 * vector_to_csr folded away (the pattern is already CSR-ordered, mdeim.py:145-149), and the
 * online multi-parameter sweep. */
int rt_project_csr_batched(rt_ctx* ctx, const int64_t* indptr, const int64_t* indices,
                           const double* data_batch, int64_t ld_data, int data_layout, int64_t B, int64_t N,
                           const double* V, int64_t ldv, int64_t r, double* AN_batch);

/* How the fused projection (r <= 128) walks a CSR pattern of N rows (indptr, indices: DEVICE arrays): it takes the rows
 * in stages of 32 and reads one record per stage from a table built on the device.  This builds that table with the
 * kernel the projection uses, copies it back and unpacks it - tests and diagnostics; read-only, it launches nothing
 * else and synchronises the ctx's stream.  records: HOST array [ceil(N / 32)][6] = {e0 first entry of the stage's rows,
 * lo first row of their column window, ne entries, nrow rows of the window (0: the stage is not windowed, its rows are
 * gathered from global memory, and lo is the stage's first row), mr longest row, uni 1 when all 32 rows have mr entries}.
 * A stage is windowed when its columns and its own rows span at most 48 rows and it has at most 512 entries.
 * *any_unwindowed (HOST) = 1 when some stage is not. */
int rt_project_stage_info(rt_ctx* ctx, const int64_t* indptr, const int64_t* indices, int64_t N, int64_t* records,
                          int* any_unwindowed);

/* ---- reduced solve (np.linalg.solve: deim.py:491-492; gmres on a dense r x r: rom.py:492) --- */

/* Solve K_b x_b = rhs_b for b < B by LU with partial pivoting, one workgroup per system.
 * K (B x r x r row-major) is left untouched (the factors are not an output), rhs (B x r) is overwritten with x.
 * info (B device ints, may be NULL): 0, or RT_WARN_SINGULAR. r <= 128. */
int rt_dense_solve_batched(rt_ctx* ctx, double* K, double* rhs, int64_t r, int64_t B, int* info);
/* K X = B for many right-hand sides against ONE r x r matrix (r <= 128): K row-major (device, untouched), B and X
 * r x nrhs row-major (device, distinct), *info (device int, may be NULL) = RT_WARN_SINGULAR on an exactly zero pivot.
 * Pivoted LU in LDS, one thread per right-hand side.  Replaces np.linalg.solve(PT_U.T, basis_rom.T) - the theta solve of
 * deim.py:477-493 applied once to every column of a projected collateral basis, when the interpolation matrix is folded
 * into the expansion of a hyper-reduced operator (romtime_amd/sweep.py). */
int rt_dense_solve_multi(rt_ctx* ctx, const double* K, int64_t r, const double* B, double* X, int64_t nrhs, int* info);
/* Least squares against ONE rows x cols matrix A, rows >= cols, for many right-hand sides, since version 450: what the
 * theta solve and its folds become when oversampling makes PT_U rectangular (np.linalg.lstsq in the reference's terms).
 * A row-major (device, untouched); B and X row-major (device, distinct, B untouched).
 *   trans = 0: X (cols x nrhs) minimises ||A X - B||_2 column by column, B rows x nrhs (the theta fit);
 *   trans = 1: X (rows x nrhs) is the minimum-norm solution of A^T X = B, B cols x nrhs: X = (A^+)^T B (the folds,
 *              PT_U^T Z^T = basis_rom^T and PT_U^T Psi^T = basis_fom^T).
 * Householder QR in LDS, factorised by every workgroup for itself, one thread per right-hand side (256 per workgroup);
 * no normal equations.  A column's result depends neither on nrhs nor on its place.  *info (device int, may be NULL) =
 * RT_WARN_SINGULAR on an exactly zero diagonal of R (a column that repeats an earlier one bit for bit gives one), else 0.
 * For rows == cols the answers agree with rt_dense_solve_multi to rounding.  Limits: cols <= 128, rows <= 256 and
 * rows x (cols | 1) <= 18432 (A beside its work space in the CU's 160 KiB of LDS; every rows x cols <= 16384 within the
 * first two bounds fits); RT_ERR_UNSUPPORTED beyond.  Null pointers, B == X, sizes < 1, rows < cols and another trans
 * return RT_ERR_ARG.  trans = 0 keeps a rows x nrhs work array in the ctx's leaf arena. */
int rt_dense_lstsq_multi(rt_ctx* ctx, const double* A, int64_t rows, int64_t cols, int trans, const double* B, double* X,
                         int64_t nrhs, int* info);
/* The argument checks and the launch plan of rt_dense_lstsq_multi - host logic only, no GPU and no pointer is followed:
 * the same return code, and on RT_OK info3 (may be NULL) = {workgroups, right-hand sides per workgroup, LDS bytes}. */
int rt_dense_lstsq_multi_plan_info(const double* A, int64_t rows, int64_t cols, int trans, const double* B, const double* X,
                                   int64_t nrhs, int64_t* info3);


/* The same solve for a SEQUENCE of slowly changing matrices (the reduced systems of consecutive time steps differ by
 * O(dt)): K_b^-1 is tracked in Xinv (B x r x r, caller-owned device memory carried from call to call) and refreshed by
 * Newton-Schulz iterations on the matrix cores, x = Xinv b plus one step of iterative refinement against K; the first
 * call (have_prev = 0), a matrix that moved too far, or one the iteration gives up on (singular to working precision:
 * then pivoted LU inside the same kernel) cost more, the answers agree with rt_dense_solve_batched to rounding.  This is
 * what rt_rom_bdf_sweep / rt_hrom_bdf_sweep call every step.  info as above.  r <= 80 (three padded matrices in LDS):
 * RT_ERR_UNSUPPORTED beyond.  rt_ctx_get_counter("sweep_lu_fallbacks" | "sweep_restarts" | ...) tells what happened. */
int rt_tracked_solve_batched(rt_ctx* ctx, const double* K, double* Xinv, double* rhs, int64_t r, int64_t B, int have_prev,
                             int* info);

/* ---- GMRES reduced solve: the reference's own solver, scipy.sparse.linalg.gmres(K_N, b_N, atol=1e-10, tol=1e-10,
 *      maxiter=1e6) with restart 20, x0 = 0, no preconditioner and info never checked (rom.py:36,414-425,492) ---------- */
#define RT_SOLVER_DIRECT 0   /* default: tracked inverse / pivoted LU, as above */
#define RT_SOLVER_GMRES 1    /* restarted GMRES with SciPy's stopping decisions */
typedef struct {
  double rtol, atol;         /* SciPy's rtol (rom.py:36 spells it tol) and atol; >= 0 */
  int64_t restart, maxiter;  /* Krylov dimension of a cycle (min(restart, r) is used) and outer cycles; >= 1 */
} rt_gmres_opts;             /* host struct */
/* x_b with K_b x_b = b_b for b < B: the control flow of SciPy 1.15's gmres step for step (norms, modified Gram-Schmidt,
 * breakdown test h1 <= eps h0, Givens rotations with LAPACK dlartg semantics, the inner test presid <= ptol, SciPy's
 * back substitution, the outer test and the ptol update), so the stopping decisions and the iterate are SciPy's up to
 * rounding.  K (B x r x r row-major), b and x (B x r) are DEVICE arrays; r <= 128 (RT_ERR_UNSUPPORTED beyond), options
 * out of range RT_ERR_ARG.  info (B device int64, may be NULL): SciPy's info, 0 or maxiter (|b - K x| > max(atol,
 * rtol |b|)); iters (B device ints, may be NULL): inner iterations, i.e. the calls of a callback_type="pr_norm" callback.
 * One wave per system; a system's result does not depend on B or on its place in the batch. */
int rt_gmres_batched(rt_ctx* ctx, const double* K, const double* b, double* x, int64_t r, int64_t B,
                     const rt_gmres_opts* opts, int64_t* info, int* iters);
/* What rt_rom_bdf_sweep / rt_hrom_bdf_sweep solve each step's systems with: RT_SOLVER_DIRECT (the default; opts may be
 * NULL) or RT_SOLVER_GMRES with opts (copied).  In GMRES mode a step's systems go to one GMRES launch that also forms
 * b_N and closes the step; "sweep_graph" is ignored; "sweep_solves", "sweep_gmres_iterations" and
 * "sweep_gmres_unconverged" tell what happened. */
int rt_ctx_set_reduced_solver(rt_ctx* ctx, int kind, const rt_gmres_opts* opts);

/* ---- online sweep (RomConstructor*.solve, rom/rom.py:430-555, :877-929) on the device --------- */
typedef struct {
  int64_t N, nnz, r, n_mu, nt;   /* DoFs, pattern nonzeros, reduced size (<= 128), parameter points, time steps */
  double dt;
  int bdf2;                      /* 1: BDF2 with u* = 2 u_h - u_h^{n-1} (fom.BDF_SCHEME == "2"), 0: BDF1 */
  const int64_t* indptr;         /* CSR pattern shared by every operator (device) */
  const int64_t* indices;
  const double* V;               /* N x r row-major reduced basis */
  const double* mass_values;     /* nnz: mass matrix values */
  int64_t n_terms;               /* affine operator terms */
  const double* term_values;     /* n_terms x nnz: value vector of each term */
  const double* term_coef;       /* nt x n_mu x n_terms: theta_q(mu, t) of step s at [s][mu][q] */
  const double* tril_values;     /* nnz or NULL: T of the state-dependent term diag(u*) T (trilinear, rom.py:931-952) */
  int64_t n_rhs;
  const double* rhs_terms;       /* n_rhs x N: source vectors (lifting / forcing) */
  const double* rhs_coef;        /* nt x n_mu x n_rhs */
} rt_sweep_desc;
/* K_N = bdf M_N + dt V^T(sum_q theta_q A_q + diag(u*) T)V,  b_N = M_N(2u^n - u^{n-1}/2) + dt V^T f,
 * u^{n+1} = K_N^-1 b_N, for all n_mu parameter points per step, nt steps, zero initial condition
 * (rom.py:451-453).  uN_out: n_mu x nt x r (device).  Everything stays on the ctx stream. */
int rt_rom_bdf_sweep(rt_ctx* ctx, const rt_sweep_desc* desc, double* uN_out);

/* ---- hyper-reduced online sweep (the (M)DEIM path of RomConstructor*.solve: interpolate(which=ROM),
 *      deim.py:416-452,477-493, mdeim.py:230-261; assemble_system rom.py:877-929) on the device ------------- */
typedef struct {
  int64_t r, n_mu, nt;           /* reduced size (<= 128), parameter points, time steps */
  double dt;
  int bdf2;                      /* as rt_sweep_desc */
  int64_t m_mass, m_lin, m_nl, m_rhs; /* interpolation coefficients: mass operator, the other (mu,t)-dependent
                                    operators together, the state-dependent operator, the source vectors */
  const double* Z;               /* (m_mass + m_lin + m_nl) x (r*r): row e = the r x r matrix that local entry e
                                    multiplies = column e of basis_rom PT_U^-1 (mdeim.py:153-192 with the theta
                                    solve of deim.py:491-492 folded in); blocks in the order mass | lin | nl */
  const double* Zf;              /* m_rhs x r: the same for the DEIM source vectors (deim.py:495-515) */
  const double* F_mass;          /* nt x n_mu x m_mass: the operator's entries at its interpolation entries,
                                    assemble(mu, t, entries=dofs) (deim.py:429-433), for every step and mu */
  const double* F_lin;           /* nt x n_mu x m_lin */
  const double* F_rhs;           /* nt x n_mu x m_rhs */
  const double* W;               /* m_nl x r: local entries of the state-dependent operator are S (W u_N* + C)
                                    (N-MDEIM, nonlinear.py:247-283: the trilinear form is linear in u_h = V u_N) */
  const double* C_nl;            /* nt x n_mu x m_nl or NULL */
  const double* S_nl;            /* nt x n_mu or NULL (= 1) */
} rt_hsweep_desc;
/* M_N = sum_e F_mass[e] Z_e;  K_N = bdf M_N + dt (sum_e F_lin[e] Z_e + sum_e S (W u* + C)_e Z_e);
 * b_N = M_N (2u^n - u^{n-1}/2) + dt Zf^T F_rhs;  u* = 2u^n - u^{n-1} (BDF2) or u^n;  zero initial condition.
 * No quantity of size N_h is touched.  uN_out: n_mu x nt x r (device). */
int rt_hrom_bdf_sweep(rt_ctx* ctx, const rt_hsweep_desc* desc, double* uN_out);
/* How the reduced systems of the most recent sweep on this ctx were solved (the reference calls GMRES once per step,
 * rom.py:492; by default K_N^-1 is tracked from step to step): stats4 = { Newton-Schulz iterations, systems restarted from
 * K^T/(|K|_1 |K|_inf), systems handed to the pivoted LU, systems solved }.  Synchronises the ctx stream. */
int rt_last_sweep_stats(rt_ctx* ctx, int64_t* stats4);

/* ---- error certification of whole trajectories (compute_error per time step, rom/base.py:52-73; the S-ROM estimator
 *      compute_rom_difference, utils.py:173-212; the three curves of HyperReducedPiston._evaluate, hrom.py:546-582) ---- */
/* err[j][t] = || U_j[:, t] - B a_j[t] ||_2 / sqrt(N) and ref[j][t] = || U_j[:, t] ||_2 / sqrt(N) for n_traj trajectories
 * and nt steps each, the lifted trajectory B a never stored.  B: N x k row-major basis (ldb), k <= 128 (RT_ERR_UNSUPPORTED
 * beyond).  A: coefficients, trajectory j is the nt x k row-major matrix (lda) at A + j * stride_a - with lda = r and
 * stride_a = nt * r exactly the uN_out of the sweeps above.  U: full-order snapshots, trajectory j the N x nt matrix
 * (ldu, u_layout) at U + j * stride_u; RT_COL_MAJOR = every snapshot contiguous (np.vstack(cols).T).  U == NULL: the
 * term is absent and err is the estimator || B a_t || / sqrt(N) (ref must then be NULL: RT_ERR_ARG, as for sizes < 1).
 * err, ref (may be NULL): n_traj x nt.  Any leading dimensions, 8-byte aligned bases.  No floating-point atomics: the
 * sums run in a fixed order that depends on N, nt and the ctx's CU count only, so a trajectory's bits depend neither on
 * n_traj nor on its place in the batch; sqrt and the division are the correctly rounded IEEE operations.  Scratch from the
 * ctx's leaf arena; rt_last_launch_info: [0] workgroups, [1] row slices, [2] tile 32 rows x 64 steps. */
int rt_trajectory_errors(rt_ctx* ctx, const double* B, int64_t ldb, const double* A, int64_t lda, int64_t stride_a,
                         const double* U, int64_t ldu, int u_layout, int64_t stride_u, int64_t N, int64_t k, int64_t nt,
                         int64_t n_traj, double* err, double* ref);

/* ---- physical outputs of whole trajectories: the mass  int rho(u) dx  on the moving mesh per time step
 *      (compute_mass_conservation with compute_rho / compute_p, fom/nonlinear.py:601-683; the third block of
 *      HyperReducedPiston._evaluate, hrom.py:586-621) ---- */
#define RT_FN_POWER 0   /* f(z) = (c0 + c1 z)^p, par = {c0, c1, p} (host) */
/* out[j][t] = scale[j][t] * sum_i w_i f(E_i . a_j[t]) for n_traj trajectories and nt steps each, since version 370; the
 * lifted trajectory E a is never stored.  E: n_pts x k row-major (lde >= k), k <= 128 (RT_ERR_UNSUPPORTED beyond), 8-byte
 * aligned: the basis evaluated at the quadrature points.  w: n_pts DEVICE weights, NULL = 1.  A: coefficients laid out
 * exactly as for rt_trajectory_errors (the uN_out of the sweeps goes in unchanged).  scale: n_traj x nt DEVICE factors,
 * NULL = 1 (the domain length L(mu_j, t) of the moving mesh).  out: n_traj x nt DEVICE.  fn selects f and par (HOST) holds
 * its parameters; RT_FN_POWER is the only one.  Null E, A, par or out, sizes < 1, an unknown fn and lde or lda < k return
 * RT_ERR_ARG.
 *   - The base is b = fma(c1, z, c0).  Where p equals an integer in 1 .. 8 exactly, f is repeated multiplication in one
 *     association - b2 = b b, b4 = b2 b2, then b, b2, b2 b, b4, b4 b, b4 b2, (b4 b2) b, b4 b4 - so exact data gives exact
 *     bits.  Every other p goes through pow: a negative base with a non-integer p gives NaN in that step's output, and in
 *     that step's output only.
 *   - Rows past n_pts are predicated out of the sum, not multiplied by a zero weight: with c0 = 0 and p < 0 a padded row
 *     evaluates f(0) = inf, and inf * 0 would poison a sum that is finite.
 *   - No floating-point atomics: partial sums are written as [trajectory][row slice][step] (ctx leaf arena) and a finish
 *     kernel adds the slices in order and applies scale.  The slicing depends on n_pts, nt and the ctx's CU count only, so
 *     a trajectory's bits depend neither on n_traj nor on its place in the batch.
 *   - rt_last_launch_info: [0] workgroups, [1] row slices, [2] tile 32 rows x 64 steps, as rt_trajectory_errors. */
int rt_trajectory_integrals(rt_ctx* ctx, const double* E, int64_t lde, const double* w, const double* A, int64_t lda,
                            int64_t stride_a, const double* scale, int64_t n_pts, int64_t k, int64_t nt, int64_t n_traj,
                            int fn, const double* par, double* out);
/* The argument checks and the launch plan of rt_trajectory_integrals for a ctx of num_cus CUs - host logic only, no GPU
 * and no pointer is followed: the same return code, and on RT_OK info3 (may be NULL) as rt_last_launch_info reports it. */
int rt_trajectory_integrals_plan_info(int num_cus, const double* E, int64_t lde, const double* w, const double* A, int64_t lda,
                                      int64_t stride_a, const double* scale, int64_t n_pts, int64_t k, int64_t nt,
                                      int64_t n_traj, int fn, const double* par, const double* out, int64_t* info3);

/* ---- certification of the (M)DEIM interpolants over whole snapshot sets (evaluate of the three classes, deim.py:226-261
 *      and nonlinear.py:470-540; run by default for every hyper-reductor, hrom.py:491-502, 796-809) ---- */
/* err[q] = (1/group) sum_{i < group} || f_s - I(f_s) ||_2 / sqrt(N), s = q group + i, for the S snapshots of F, since
 * version 380; I(f) = Psi f[idx] with entry pin_row replaced by pin_value where pin_row >= 0 (MDEIM's Dirichlet entry,
 * deim.py:449-450), and ref[q] (may be NULL) the same mean of || f_s ||_2 / sqrt(N), always of the data as they are.  No
 * theta array, interpolant or modified copy of the snapshots is stored.  Psi: N x m row-major DEVICE matrix (ldpsi >= m),
 * the basis with the theta solve folded in, basis_fom PT_U^-1; m <= 128 (RT_ERR_UNSUPPORTED beyond).  idx: m HOST flat
 * indices into a snapshot, each checked to lie in [0, N) before anything is launched (RT_ERR_ARG otherwise): the
 * coefficients of a snapshot are its own entries at idx.  F: N x S DEVICE matrix (ldf, f_layout); RT_COL_MAJOR = every
 * snapshot contiguous (what rt_p1_local_assembly writes).  err, ref: S / group DEVICE values.  Any legal leading
 * dimensions, 8-byte aligned bases.  Null Psi, idx, F or err, sizes < 1, S % group != 0, pin_row outside [-1, N), an
 * unknown layout and short leading dimensions return RT_ERR_ARG, all before any launch.
 *   - (f - l), the square and the sums are separate IEEE operations, sqrt and the divisions correctly rounded; the group
 *     mean is a running sum in index order and one division, as nonlinear.py:518-535 forms it.
 *   - No floating-point atomics: partial sums are written as [snapshot][row slice] (ctx leaf arena) and a finish kernel
 *     adds the slices in order.  The slicing depends on N and the ctx's CU count only, so the bits of a snapshot's error
 *     depend neither on S, its place in the block, nor group: a set may be handed over in chunks.
 *   - rt_last_launch_info: [0] workgroups, [1] row slices, [2] tile 32 rows x 64 snapshots. */
int rt_interpolation_errors(rt_ctx* ctx, const double* Psi, int64_t ldpsi, const int64_t* idx, int64_t m, const double* F,
                            int64_t ldf, int f_layout, int64_t N, int64_t S, int64_t group, int64_t pin_row, double pin_value,
                            double* err, double* ref);
/* The argument checks and the launch plan of rt_interpolation_errors for a ctx of num_cus CUs - host logic only, no GPU:
 * idx (a host array) is read, no other pointer is followed.  The same return code, and on RT_OK info3 (may be NULL) as
 * rt_last_launch_info reports it. */
int rt_interpolation_errors_plan_info(int num_cus, const double* Psi, int64_t ldpsi, const int64_t* idx, int64_t m,
                                      const double* F, int64_t ldf, int f_layout, int64_t N, int64_t S, int64_t group,
                                      int64_t pin_row, double pin_value, const double* err, const double* ref, int64_t* info3);

/* ---- closed-form local assembly of the 1-D P1 operators at (M)DEIM entries (the step before the path) ----------
 * What ``assemble(mu, t, entries=dofs[, u_n])`` returns for the reference's 1-D problems (fom/base.py:523-599 per-entry
 * assembly of the forms in fom/nonlinear.py:374-494; closed forms as in testing/mock.py:30-85), for n_states states at
 * once: out[s][e] = operator(kind; h[s], coef[s], nodal function of state s) at entry (rows[e], cols[e]) of the
 * (nx + 1) x (nx + 1) matrix, or at vector entry rows[e] for RT_P1_LOAD (cols = NULL).  h[s] = L(mu, t) / nx is the
 * cell size of state s, coef[s] a scalar factor (NULL = 1; the diffusivity alpha(mu, t) for the stiffness).  The
 * nodal function (w of the trilinear form int w u' v, f of the load int f v): state_mode 1 = state is n_states x (nx+1)
 * nodal values, 2 = state is n_states amplitudes of the ramp amp * node / nx (the piston lifting g = amp x / L), 0 = none.
 * First / last dof are Dirichlet rows (identity rows, zero load).  Feeds the F tables of rt_hrom_bdf_sweep. */
#define RT_P1_MASS 0
#define RT_P1_STIFFNESS 1
#define RT_P1_CONVECTION 2
#define RT_P1_TRILINEAR 3
#define RT_P1_LOAD 4
/* RT_P1_LOAD_P2: int f v with f the P2 interpolant of the data on every cell - what FEniCS integrates for an
 * Expression(..., degree=2) (fom/heat.py:119 forcing; fom/base.py:452-495 lifting data), exact for quadratic f:
 * out = coef h/3 (f_{i-1/2} + f_i + f_{i+1/2}).  state_mode 1 = n_states x (2 nx + 1) values (vertex k at 2k, midpoint
 * of cell k at 2k+1), state_mode 3 = n_states x 3 coefficients of a0 + a1 x + a2 x^2 in the physical coordinate.
 * Reproduces the reference's known-answer tables expected_mat_fh / expected_mat_fgh_time (tests/test_mpf1.py:288-302):
 * forcing problems/mfp1.py:38-39; lifting vector = -h dg_dt(x_i) (fom/heat.py:131-169) = this kind with coef = -1. */
#define RT_P1_LOAD_P2 5
int rt_p1_local_assembly(rt_ctx* ctx, int kind, int64_t nx, const int64_t* rows, const int64_t* cols, int64_t m,
                         int64_t n_states, const double* h, const double* coef, int state_mode, const double* state,
                         double* out);

/* ---- snapshot sets of the closed-form 1-D P1 operators over a product grid (what the six (M)DEIM objects are trained on,
 *      rom/hrom.py:419-448, 1092-1146: one whole operator per (mu, t), deim/deim.py:384-389, or per (mu, t, psi),
 *      deim/nonlinear.py:437-443), since version 440 ----
 * out is (n_par n_fun) x m: column (p, f) - parameter row p, nodal function f - is the m contiguous values at
 * out + (p n_fun + f) m, so out is the RT_COL_MAJOR m x S set, S = n_par n_fun, that rt_gram and rt_pod_orth take as it is.
 *   value = beta out_old + (zero_first && e == 0 ? 0 : v),
 * v bit for bit what rt_p1_local_assembly returns for the same kind, entry (rows[e], cols[e]), h, coef and nodal function
 * (both call one function, csrc/p1_entry.h).  Parameter row p carries h[p], coef[p] (NULL = 1) and, by par_mode, what
 * rt_p1_local_assembly's state_mode carries: 2 = par is n_par ramp amplitudes, 3 = par is n_par x 3 polynomial
 * coefficients (RT_P1_LOAD_P2 only), 0 = par is NULL.  fun: n_fun x (nx + 1) nodal functions shared by every parameter row
 * (n_fun x (2 nx + 1) for RT_P1_LOAD_P2).  Exactly one of par / fun supplies the nodal function of the kinds that integrate
 * one (RT_P1_TRILINEAR and the loads; with par, n_fun = 1); the other kinds take n_fun = 1, fun = NULL, par = NULL.
 *   - beta = 0 does not read out; otherwise v is rounded before it is added to the rounded beta out_old (beta = 1: the
 *     sum of two tables, rounded once per entry, without a temporary).  zero_first: entry 0 of every column adds 0 (the
 *     boundary entry of the MDEIM snapshots, deim/deim.py:388-389).
 *   - One launch for any n_par n_fun m < 2^62: a grid stride over (column, entry), lanes along the entries.  Vector stores
 *     only, no atomics, every word of out written by one thread.  A row outside [0, nx] gives 0.
 *   - Null rows, h, out (cols for the matrix kinds), sizes < 1, nx < 2, an unknown kind or par_mode, a par / fun combination
 *     the kind cannot take and a count of 2^62 or more return RT_ERR_ARG, nx > 2^22 RT_ERR_UNSUPPORTED, all before any launch.
 *   - rt_last_launch_info: [0] workgroups, [1] launches (1), [2] 1 x 256 words per workgroup and pass. */
int rt_p1_snapshot_sets(rt_ctx* ctx, int kind, int64_t nx, const int64_t* rows, const int64_t* cols, int64_t m,
                        int64_t n_par, const double* h, const double* coef, int par_mode, const double* par,
                        int64_t n_fun, const double* fun, int zero_first, double beta, double* out);
/* The argument checks and the launch plan of rt_p1_snapshot_sets for a ctx of num_cus CUs - host logic only, no GPU and no
 * pointer is followed: the same return code, and on RT_OK info2 (may be NULL) = {workgroups, launches}. */
int rt_p1_snapshot_sets_plan_info(int num_cus, int kind, int64_t nx, const int64_t* rows, const int64_t* cols, int64_t m,
                                  int64_t n_par, const double* h, const double* coef, int par_mode, const double* par,
                                  int64_t n_fun, const double* fun, int zero_first, double beta, const double* out,
                                  int64_t* info2);

/* ---- full-order BDF sweeps of the closed-form 1-D P1 models (the time loop of OneDimensionalSolver.solve,
 *      fom/base.py:693-831, for the heat problem fom/heat.py:57-82, 251-262 and the piston fom/nonlinear.py:322-494;
 *      testing/mock.py: MockHeatEquation.solve, MockBurgers.solve) for a batch of parameter points, since version 390 ---- */
typedef struct {
  int64_t nx, n_mu, nt;    /* cells (N_h = nx + 1 >= 3), parameter points, steps of THIS call */
  int64_t first_step;      /* global index of this call's first step: the step with global index 0 is BDF1 */
  double dt;
  int bdf2;                /* as rt_sweep_desc */
  int state_in_w;          /* 1: w includes u* (Burgers), 0: linear problem (heat) */
  const double* tab;       /* nt x n_mu x 7 DEVICE: h, alpha, c0, c1, a0, a1, a2 of step s, point j */
  const double* u_init;    /* NULL = zero state (then first_step must be 0), else n_mu x 2 x N_h DEVICE: u^n, u^{n-1} */
} rt_fom_desc;             /* host struct */
/* Every step solves, for each point, the tridiagonal system of the interior rows i = 1 .. nx-1
 *     l_i = bdf h/6 + dt(-alpha/h - b_{i-1}),  d_i = bdf 4h/6 + dt(2 alpha/h + b_{i-1} - a_i),  u_i = bdf h/6 + dt(-alpha/h + a_i),
 *     rhs_i = h/6 (past_{i-1} + 4 past_i + past_{i+1}) + dt h/3 (f(x_i - h/2) + f(x_i) + f(x_i + h/2)),  x_i = i h,
 * with a_e = (2 w_e + w_{e+1})/6, b_e = (w_e + 2 w_{e+1})/6 per cell of the nodal function w_i = s u*_i + c0 + c1 i/nx
 * (s = state_in_w), f = a0 + a1 x + a2 x^2 (the RT_P1_LOAD_P2 rule), and bdf = 1.5, u* = 2u^n - u^{n-1}, past = 2u^n -
 * u^{n-1}/2 from global step 1 on when bdf2 is set, otherwise 1, u^n, u^n: mass + stiffness + ONE trilinear form, which
 * covers MockSolver's constant convection (c0 = -1), the ALE ramp of the moving heat problem and the lifting ramp of the
 * piston (c1), and the state.  The Dirichlet values u_0 = u_nx = 0 are written as zeros.
 *   - U_out: trajectory j starts at U_out + j stride_mu and its step s is the N_h contiguous values at + s ld_step - the
 *     RT_COL_MAJOR N_h x nt snapshot matrix that rt_gram, rt_pod_orth and rt_trajectory_errors take unchanged.
 *   - info: n_mu DEVICE ints, each 0, or 1 + the global index of the first step in which some row is not diagonally
 *     dominant (|d| < |l| + |u|) or a pivot is not finite.  The sweep of a flagged point carries on (there is no pivoting,
 *     so its values are then not to be trusted); a flag never affects another point.
 *   - Null desc, tab, U_out or info, sizes < 1, nx < 2, ld_step < N_h, trajectories that overlap (n_mu > 1 needs
 *     stride_mu >= (nt-1) ld_step + N_h) and u_init == NULL with first_step != 0 return RT_ERR_ARG before any launch.  nx <= 2^22; beyond, or where the states and factors
 *     of the call (40 KiB x ceil((nx-1)/1024) per point, ctx leaf arena) exceed 64 GiB, RT_ERR_UNSUPPORTED.
 *   - One workgroup per parameter point and the whole time loop in one launch; no workgroup waits for another, so n_mu may
 *     exceed the CU count, nothing can time out and a CU-masked stream gives the same bits.  Each of up to 1024 threads
 *     eliminates a partition of consecutive rows formed on the fly, the partitions' last unknowns are solved for in LDS
 *     by cyclic reduction, and the back-substitution inside every partition follows; no pivoting, no floating-point atomics.
 *   - The bits of a trajectory depend on nx, its own table rows, dt and the flags only - not on n_mu, the point's place in
 *     the batch, the ctx's CU count or how the horizon is cut into calls (u_init = the two last states of the call before).
 *   - rt_last_launch_info: [0] workgroups, [1] partitions per system, [2] rows per partition. */
int rt_p1_fom_bdf_sweep(rt_ctx* ctx, const rt_fom_desc* desc, double* U_out, int64_t ld_step, int64_t stride_mu, int* info);
/* The argument checks and the partitioning of rt_p1_fom_bdf_sweep - host logic only, no GPU and no pointer but desc is
 * followed (U_out and info, which it does not take, count as given): the same return code, and on RT_OK info3 (may be
 * NULL) = {workgroups, partitions per system, rows per partition}. */
int rt_p1_fom_bdf_sweep_plan_info(int num_cus, const rt_fom_desc* desc, int64_t ld_step, int64_t stride_mu, int64_t* info3);
/* The same sweep, certified by the backward error of every step's solve instead of by diagonal dominance, since version
 * 410.  Dominance, |d| >= |l| + |u|, holds for the rows above only where about |w| dt/h <= 2 bdf/3 + 2 alpha dt/h^2 - a
 * CFL number below one or a cell Peclet number below two - and is sufficient, not necessary: the unpivoted elimination
 * is backward stable far outside that regime (the piston at alpha = 1e-6, CFL 10 to 2000), and this entry measures it.
 *   - The solve is that of rt_p1_fom_bdf_sweep: for equal inputs U_out has the same bits.
 *   - defect: n_mu x desc->nt DEVICE doubles, defect[j nt + s] = the componentwise backward error of step s of point j,
 *       omega = max over the interior rows i of |rhs_i - (l_i x_{i-1} + d_i x_i + u_i x_{i+1})|
 *                                               / (|l_i x_{i-1}| + |d_i x_i| + |u_i x_{i+1}| + |rhs_i|)      (0/0 = 0),
 *     x the new state, the rows formed again by the formulas above from the same two older states, l_1 = u_{nx-1} = 0:
 *     the smallest relative perturbation of every entry of the step's system for which x solves it exactly.  +inf where
 *     a pivot, a partition's last unknown or a value of the new state is not finite.
 *   - info: n_mu DEVICE ints, each 0, or 1 + the global index of the first step whose defect is not finite or above
 *     defect_tol.  Dominance is not looked at.  The sweep of a flagged point carries on; a flag never affects another point.
 *   - The argument checks of rt_p1_fom_bdf_sweep; a null defect and a defect_tol that is negative or NaN return
 *     RT_ERR_ARG before any launch.  The new state goes to a third state array, so that both older states are still
 *     there when the defect is formed: 48 KiB x ceil((nx-1)/1024) per point of ctx leaf arena (six arrays, not five),
 *     RT_ERR_UNSUPPORTED beyond 64 GiB; the defect pass reads three arrays more per step (thirteen, not ten).
 *   - Everything else as rt_p1_fom_bdf_sweep: one workgroup per point, no waiting between workgroups, no floating-point
 *     atomics, nx <= 2^22; the bits of a trajectory AND its defects do not depend on n_mu, the point's place in the batch
 *     or how the horizon is cut into calls.  No pivoting and no refinement: a flagged point is not to be trusted. */
int rt_p1_fom_bdf_sweep_certified(rt_ctx* ctx, const rt_fom_desc* desc, double* U_out, int64_t ld_step, int64_t stride_mu,
                                  double defect_tol, double* defect, int* info);
/* The plan query of the certified entry: as rt_p1_fom_bdf_sweep_plan_info, info4 (may be NULL) = {workgroups, partitions
 * per system, rows per partition, scratch bytes per point}. */
int rt_p1_fom_bdf_sweep_certified_plan_info(int num_cus, const rt_fom_desc* desc, int64_t ld_step, int64_t stride_mu,
                                            int64_t* info4);

/* ---- residuals of lifted reduced trajectories in the full-order step system, since version 420: what the time loop of
 *      OneDimensionalSolver.solve (fom/base.py:693-831) solves at every step, evaluated at x^t = B a_j[t] instead of
 *      solved - an error indicator of an online sweep that needs no full-order solve and no second reduced model ---- */
/* desc is the descriptor of rt_p1_fom_bdf_sweep for the same points and steps: nx, n_mu (the number of trajectories), nt,
 * first_step, dt, bdf2, state_in_w, tab.  desc->u_init must be NULL: the two older states come as coefficients, a_init =
 * NULL for a zero state (then first_step must be 0), else n_mu x 2 x k DEVICE, a^n and a^{n-1} of every trajectory.
 * B: the (nx+1) x k row-major basis, ldb >= k, k <= 128 (RT_ERR_UNSUPPORTED beyond); A, lda, stride_a exactly as for
 * rt_trajectory_errors (the uN_out of the sweeps goes in unchanged).  With the lifted states x^t = B a_j[t], whose values
 * at the nodes 0 and nx are taken as 0 whatever B holds in those rows (the Dirichlet zeros the sweep writes), step s of
 * trajectory j has the interior rows i = 1 .. nx-1 of rt_p1_fom_bdf_sweep, formed from the lifted states of the steps
 * s-1 and s-2 with l_1 = u_{nx-1} = 0, and
 *     r_i = fma(-u_i, x_{i+1}, fma(-d_i, x_i, fma(-l_i, x_{i-1}, rhs_i))),  s_i = |l_i x_{i-1}| + |d_i x_i| + |u_i x_{i+1}| + |rhs_i|,
 *     res[j nt + s] = sqrt(sum_i r_i^2),   scale[j nt + s] = sqrt(sum_i s_i^2)     (n_mu x nt DEVICE each; scale may be NULL).
 *   - res / scale is the 2-norm companion of the componentwise defect of rt_p1_fom_bdf_sweep_certified: a few eps for the
 *     sweep's own trajectory (B = I), the size of the reduction and hyper-reduction error otherwise.
 *   - A lifted value that is not finite makes res NaN or inf at the steps that read it - its own and, as an older state,
 *     the two after it - and at no other step and in no other trajectory.
 *   - Null desc, tab, B, A or res, a non-null desc->u_init, sizes < 1, nx < 2, ldb or lda < k and a_init == NULL with
 *     first_step != 0 return RT_ERR_ARG before any launch; nx > 2^22 and k > 128 RT_ERR_UNSUPPORTED.
 *   - The lifted trajectory is never stored: 32-row stages of B against a 64-step coefficient block on the f64 matrix
 *     cores, as rt_trajectory_errors; the lifted tile goes through LDS, and a stage evaluates its inner 30 rows, a block
 *     its last 62 steps.  No floating-point atomics: partial sums go to [trajectory][row slice][step] in the ctx's leaf
 *     arena and a second kernel adds the slices in order.  The slicing depends on nx and the ctx's CU count only, so the
 *     bits of a trajectory depend neither on n_mu, nor on its place in the batch, nor on how the horizon is cut into
 *     calls (a_init = the two last coefficient rows of the call before).
 *   - rt_last_launch_info: [0] workgroups, [1] row slices, [2] tile 30 rows x 62 steps (30062). */
int rt_trajectory_residuals(rt_ctx* ctx, const rt_fom_desc* desc, const double* B, int64_t ldb, int64_t k, const double* A,
                            int64_t lda, int64_t stride_a, const double* a_init, double* res, double* scale);
/* The argument checks and the slicing of rt_trajectory_residuals for a ctx with num_cus CUs - host logic only, no GPU,
 * and no pointer but desc is followed: the same return code, and on RT_OK info3 (may be NULL) as rt_last_launch_info
 * reports it. */
int rt_trajectory_residuals_plan_info(int num_cus, const rt_fom_desc* desc, const double* B, int64_t ldb, int64_t k,
                                      const double* A, int64_t lda, int64_t stride_a, const double* a_init, const double* res,
                                      const double* scale, int64_t* info3);

/* ---- small symmetric eigenproblem of the Gram matrix, on the device (3 <= n <= 2048) ---------- */
/* Householder tridiagonalisation (32 cooperating workgroups, 128 for n > 512; matrix resident in LDS) + Sturm
 * multisection:
 * lam (n, device) = all eigenvalues of the symmetric G (n x n row-major, not modified), DESCENDING.
 * status (device int, may be NULL): 0, or 1 if the inter-workgroup hand-off timed out (results
 * invalid).  Replaces the eigenvalue half of LAPACK's work inside scipy.linalg.svd (pod.py:38).
 * 1024 < n <= 2048 (since version 350) takes the wide route: the work copy of G lives in the ctx's composite arena
 * (2 n^2 doubles with the reflectors: 64 MB at the limit) and the reduction is about 2 n launches on the ctx stream, one
 * per dependency - no workgroup waits for another, so it needs no co-resident team, cannot time out (status is 0) and
 * gives the same bits on a CU-masked stream as on the whole chip; counter "eig_wide_form".  All three entry points
 * below take 3 <= n <= 2048; n > 2048 returns RT_ERR_UNSUPPORTED. */
int rt_sym_eig_values(rt_ctx* ctx, const double* G, int64_t n, double* lam, int* status);
/* The same, but only the eigenvalues with descending index in [first, first + count) are searched and written
 * (lam[first .. first+count)); the tridiagonalisation is complete either way.  For a row-sharded POD every rank
 * holds the same G after the all-reduce: the ranks split the multisection (and the eigenvectors, by passing
 * lam + first and their share of k to rt_sym_eig_vectors) and all-gather the pieces. */
int rt_sym_eig_values_part(rt_ctx* ctx, const double* G, int64_t n, int64_t first, int64_t count, double* lam,
                           int* status);
/* Eigenvectors of the k LARGEST eigenvalues by inverse iteration on the tridiagonal form and
 * back-transformation; must directly follow rt_sym_eig_values on the same ctx (it reuses the
 * reflectors kept in the ctx's workspace).  W: n x k row-major, column t pairs with lam[t]. */
int rt_sym_eig_vectors(rt_ctx* ctx, int64_t n, int64_t k, const double* lam, double* W);

/* Two-sided Jacobi eigen-decomposition of a symmetric n x n DEVICE matrix A (row-major, not modified; its upper triangle
 * is what counts), 1 <= n <= 2048 (RT_ERR_UNSUPPORTED beyond; null or non-positive arguments RT_ERR_ARG), since version
 * 360: A = W diag(lam) W^T, lam (n, device) DESCENDING and stable on ties by index, eigenvectors in the columns of W
 * (n x n row-major, device).  The rotations and the relative stopping rule |a_pq| <= eps sqrt(|a_pp a_qq|) are those of
 * rt_host_jacobi_eigh below, so small eigenvalues of a graded matrix come out to high relative accuracy; the order is a
 * round-robin tournament (n - 1 rounds of n / 2 disjoint pairs per sweep, n rounds with one idle index when n is odd),
 * one launch per round on the ctx stream, the work copies and the rotations in the ctx's composite arena (3 n^2 doubles:
 * 96 MB at the limit).  The host reads one integer per sweep (it synchronises the stream) and stops after a sweep without
 * rotations or after max_sweeps: *sweeps_done (HOST int, may be NULL) = sweeps run, the closing one included; status
 * (DEVICE int) = 0, or 1 when max_sweeps ended the loop (lam and W are written either way).  Grids and every operation
 * depend on n alone and there is no floating-point atomic: the same bits on a CU-masked stream, on every rank, every time.
 * rt_last_launch_info: [0] sweeps, [1] rounds per sweep, [2] workgroups of a round.  The second-pass Gram matrix of the
 * POD (romtime_amd/pod.py, passes=2). */
int rt_sym_jacobi_eigh(rt_ctx* ctx, const double* A, int64_t n, double* lam, double* W, int max_sweeps, int* sweeps_done,
                       int* status);

/* ---- Gram matrices of 2049 .. 16384 snapshots: block Rayleigh-Ritz (since version 400; the eigenvalue half of
 *      scipy.linalg.svd, pod.py:38, for sets wider than the eigensolver above takes) ---------- */
/* The partition rule, host logic only: p = ceil(n / block_max) contiguous blocks whose widths differ by at most one, the
 * wider ones first (widths[b] = n / p + (b < n % p)).  *p_out = p; widths (p entries, may be NULL).  n < 1, block_max < 1
 * or a null p_out return RT_ERR_ARG, p > 8 RT_ERR_UNSUPPORTED (16384 = 8 x 2048). */
int rt_sym_eig_blocked_plan_info(int64_t n, int64_t block_max, int64_t* p_out, int64_t* widths);
#define RT_EIG_BLOCKED_OK 0
#define RT_EIG_BLOCKED_NOT_REDUCIBLE 1
#define RT_EIG_BLOCKED_SOLVE_FAILED 2
/* Leading eigenpairs of a symmetric positive semi-definite G (n x n row-major DEVICE matrix, not modified), 2048 < n <=
 * 16384, whose spectrum decays (a snapshot Gram matrix).  The diagonal blocks of the partition above (block_max = 2048)
 * go through rt_sym_eig_values / rt_sym_eig_vectors one after the other; block b keeps the rho_b eigenvectors W_b whose
 * eigenvalue exceeds floor_rel * lam_max, lam_max the largest block eigenvalue of all; with W = blockdiag(W_b) (n x R, R =
 * sum rho_b) the R x R matrix G_M = (W^T G W + its transpose) / 2 goes through the same eigensolver (closed form for R <= 2)
 * and its eigenpairs (theta, Y) give the Ritz pairs (theta, W Y) of G:  0 <= lam_i(G) - theta_i <= p floor_rel lam_max in
 * exact arithmetic ("Block Rayleigh-Ritz").
 *   - lam (n, DEVICE): the R Ritz values, descending, then zeros.  W (DEVICE, n x min(k, R) row-major, leading dimension
 *     min(k, R); may be NULL when k = 0): column t pairs with lam[t].
 *   - resolved (HOST, 1 entry) = R; block_ranks (HOST, p entries) = rho_b; status (HOST int) = RT_EIG_BLOCKED_OK,
 *     RT_EIG_BLOCKED_NOT_REDUCIBLE when R > 2048 (lam and W are left untouched, block_ranks and resolved are filled, the
 *     call returns RT_OK; the pass over the blocks ends as soon as the eigenvalues above floor_rel max_b trace(G_bb), an
 *     upper bound of the floor, pass 2048, and block_ranks / resolved are then those lower bounds), or
 *     RT_EIG_BLOCKED_SOLVE_FAILED when an eigensolve reported a nonzero status of its own (a hand-off time-out: that
 *     status is 1 as well, hence a value of its own here; results invalid, the call returns RT_OK).
 *   - 2048 < n <= 16384, floor_rel > 0, 0 <= k <= n; n <= 2048 returns RT_ERR_ARG (rt_sym_eig_values takes those), n >
 *     16384 RT_ERR_UNSUPPORTED.
 *   - Synchronises the ctx stream (every block's spectrum is read on the host).  Work memory is taken from the device's
 *     stream-ordered pool for the duration of the call, the eigensolves use the ctx arenas as they always do.  No
 *     floating-point atomics, and every grid depends on the sizes alone.
 *   - Counters "eig_blocked", "eig_blocked_not_reducible", "eig_blocked_rank". */
int rt_sym_eig_blocked(rt_ctx* ctx, const double* G, int64_t n, double floor_rel, int64_t k, double* lam, double* W,
                       int64_t* resolved, int64_t* block_ranks, int* status);

/* ---- host-side small dense step --------------------------------------------------------- */
/* Cyclic two-sided Jacobi eigen-decomposition of a symmetric PSD n x n HOST matrix A (row-major,
 * destroyed): A = W diag(lam) W^T, lam descending, eigenvectors in the columns of W (row-major).
 * Relative stopping rule |a_pq| <= eps sqrt(a_pp a_qq): small eigenvalues of a graded matrix come
 * out to high relative accuracy (what dgesvd delivers on the snapshots themselves, pod.py:38).
 * HOST pointers; no ctx; used on the second-pass Gram matrix of rt_gram. */
int rt_host_jacobi_eigh(double* A, int64_t n, double* W, double* lam, int max_sweeps, int* sweeps_done);

/* ---- measurement helpers (not part of the reference surface) ------------------------------ */
/* Runs `iters` back-to-back v_mfma_f64_16x16x4_f64 per wave on a full-chip grid and returns
 * the achieved TFLOP/s in *tflops (synchronises). */
int rt_bench_mfma_f64(rt_ctx* ctx, int iters, double* tflops);
/* Device-to-device streaming copy of `bytes` bytes; returns GB/s (read+write) (synchronises). */
int rt_bench_copy(rt_ctx* ctx, void* dst, const void* src, int64_t bytes, int reps, double* gbps);

#ifdef __cplusplus
}
#endif
#endif /* ROMTIME_HIP_H */
