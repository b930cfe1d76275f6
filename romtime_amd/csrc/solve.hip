// Batched small dense solve: LU with partial pivoting, one workgroup per system, the whole
// r x r matrix resident in LDS (r <= 128 -> 128 KiB of the CU's 160 KiB).
// Stands in for np.linalg.solve (theta solve, deim.py:491-492) and for the GMRES(20) call on
// the dense reduced system (rom.py:36,492): a direct solve meets the reference's 1e-10
// residual target with margin (SURVEY.md hard part E).
//
// Latency-bound, so the elimination is organised around ONE workgroup barrier per column:
//   * rows are never swapped physically: a row that has served as pivot is retired (implicit permutation),
//   * thread (row, part) owns the columns j == part (mod parts) of its row for the whole factorisation, the
//     right-hand side rides along, and the multipliers are not stored (the factors are not an output),
//   * while a thread updates column c+1 of its row it already knows that row's candidate for the next pivot
//     search; the per-wave maxima (DPP reduction, no LDS shuffles) go to a double-buffered LDS slot, and after
//     the barrier every thread finishes the argmax redundantly instead of waiting for one wave to do it,
//   * the LDS reads of a batch of columns are all issued before the first write of the batch,
//   * back substitution runs in the first wave alone (no barriers).
#include "common.h"
#include "wave_ops.h"
#include "sweep_step.h"
#include "tile_layout.h"

namespace {

constexpr int SOLVE_THREADS = 256;
constexpr int SOLVE_WAVES = SOLVE_THREADS / 64;
constexpr int SOLVE_BATCH = 4;

// LU with partial pivoting of the r x r matrix A (LDS, leading dimension lda, overwritten) and the solve with the
// right-hand side b (LDS, overwritten); the solution goes to xout (global, r values).  NT threads, all of which must
// call it; `parts` threads share a row.  Returns 1 when a pivot was exactly zero.  The matrix and b must be in LDS
// and visible (barrier) on entry; xout is complete after the caller's next barrier.
// `perm_out` (LDS, r ints, optional): the pivot row of every column; with it the multipliers are kept in place of the
// eliminated entries (A[i][c] = l_ic for the rows i still live at column c), so that further right-hand sides can be
// solved against the factors (dense_solve_multi_kernel).
template <int NT>
__device__ __forceinline__ int lu_solve_lds(double* A, int lda, double* b, int r, int parts, double* rb,
                                            int* perm_out = nullptr) {
  constexpr int WAVES = NT / 64;
  __shared__ double s_pv[2][WAVES];
  __shared__ int s_pi[2][WAVES];
  __shared__ int s_perm[128];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int row = tid / parts, part = tid - row * parts;
  const bool owner = row < r;
  bool retired = !owner;
  double* Ar = A + (owner ? row : 0) * lda;
  int sing = 0;
  int cm = 1 % parts;  // (c + 1) mod parts
  double l_keep = 0.0;
  int c_keep = -1;

  double cand = (owner && part == 0) ? fabs(Ar[0]) : -1.0;  // candidates of column 0
  for (int c = 0; c < r; ++c) {
    int ci = row;
    rtw::wave_argmax(cand, ci);  // (|value| desc, row asc) over the wave's live rows
    if (lane == 0) {
      s_pv[c & 1][wid] = cand;
      s_pi[c & 1][wid] = ci;
    }
    __syncthreads();
    if (c_keep >= 0) {
      Ar[c_keep] = l_keep;
      c_keep = -1;
    }
    double best = s_pv[c & 1][0];
    int pr = s_pi[c & 1][0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) {
      const double ov = s_pv[c & 1][w];
      const int oi = s_pi[c & 1][w];
      if (ov > best || (ov == best && oi < pr)) {
        best = ov;
        pr = oi;
      }
    }
    if (best == 0.0) sing = 1;
    if (tid == 0) s_perm[c] = pr;
    cand = -1.0;
    if (row == pr) retired = true;
    if (!retired) {
      const double* Ap = A + pr * lda;
      const double l = Ar[c] / Ap[c];
      if (perm_out && part == 0) {   // written after the NEXT barrier: the row's other threads are reading Ar[c] now
        l_keep = l;
        c_keep = c;
      }
      // first owned column after c: c + 1 + ((part - (c + 1)) mod parts)
      int d = part - cm;
      if (d < 0) d += parts;
      for (int jb = c + 1 + d; jb < r; jb += SOLVE_BATCH * parts) {
        double pv[SOLVE_BATCH], av[SOLVE_BATCH];
#pragma unroll
        for (int u = 0; u < SOLVE_BATCH; ++u) {
          const int jj = jb + u * parts;
          const bool ok = jj < r;
          pv[u] = ok ? Ap[jj] : 0.0;
          av[u] = ok ? Ar[jj] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < SOLVE_BATCH; ++u) {
          const int jj = jb + u * parts;
          av[u] = fma(-l, pv[u], av[u]);
          if (jj < r) Ar[jj] = av[u];
        }
        if (jb == c + 1) cand = fabs(av[0]);  // this thread owns column c+1 of its row: next pivot candidate
      }
      if (part == 0) b[row] = fma(-l, b[pr], b[row]);
    }
    if (++cm == parts) cm = 0;
  }
  __syncthreads();
  if (perm_out) {
    if (c_keep >= 0) Ar[c_keep] = l_keep;
    for (int c = tid; c < r; c += NT) perm_out[c] = s_perm[c];
    __syncthreads();
  }

  // back substitution over the pivot order: x_c = b[p_c] / A[p_c][c];  b[p_k] -= A[p_k][c] x_c for k < c
  if (wid == 0) {
    // lane owns pivot positions k = lane and lane + 64
    const int p0 = (lane < r) ? s_perm[lane] : 0, p1 = (lane + 64 < r) ? s_perm[lane + 64] : 0;
    double b0 = (lane < r) ? b[p0] : 0.0, b1 = (lane + 64 < r) ? b[p1] : 0.0;
    // reciprocals of the diagonal up front (one division per lane instead of one per column on the serial path)
    const double rd0 = (lane < r) ? 1.0 / A[p0 * lda + lane] : 0.0, rd1 = (lane + 64 < r) ? 1.0 / A[p1 * lda + lane + 64] : 0.0;
    double d0 = A[p0 * lda + r - 1], d1 = A[p1 * lda + r - 1];  // column c of this lane's rows, one column ahead
    for (int c = r - 1; c >= 0; --c) {
      const int src = c & 63;
      const double n0 = (c > 0) ? A[p0 * lda + c - 1] : 0.0, n1 = (c > 0) ? A[p1 * lda + c - 1] : 0.0;
      const double xc = rtw::read_lane(c < 64 ? b0 * rd0 : b1 * rd1, src);
      if (lane < c) b0 = fma(-d0, xc, b0);
      if (lane + 64 < c) b1 = fma(-d1, xc, b1);
      if (lane == src) rb[c] = xc;
      d0 = n0;
      d1 = n1;
    }
  }
  return sing;
}

__global__ __launch_bounds__(SOLVE_THREADS) void dense_solve_kernel(const double* __restrict__ K,
                                                                    double* __restrict__ rhs, int r, int parts,
                                                                    int* info) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int lda = r | 1;  // odd leading dimension: column walks hit distinct banks
  double* A = sm;         // r x lda
  double* b = sm + (size_t)r * lda;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const double* Kb = K + (size_t)blockIdx.x * r * r;
  double* rb = rhs + (size_t)blockIdx.x * r;
  for (int i = wid; i < r; i += SOLVE_WAVES)
    for (int j = lane; j < r; j += 64) A[i * lda + j] = Kb[i * r + j];
  for (int e = tid; e < r; e += SOLVE_THREADS) b[e] = rb[e];
  __syncthreads();
  const int sing = lu_solve_lds<SOLVE_THREADS>(A, lda, b, r, parts, rb);
  if (info && tid == 0) info[blockIdx.x] = sing ? RT_WARN_SINGULAR : 0;
}

// K X = B for MANY right-hand sides against one matrix (folding an interpolation matrix PT_U into the expansion of a
// hyper-reduced operator, Z = basis_rom PT_U^-1: np.linalg.solve with r^2 right-hand sides in the reference's terms,
// deim.py:477-493 applied once to every column).  Every workgroup factorises K for itself in LDS (pivoted LU with the
// multipliers kept) and then gives each of its threads one right-hand side: forward and back substitution in pivot
// order, the column's intermediate values in the output array (coalesced across the threads: the right-hand-side index
// runs fastest), the factors broadcast out of LDS.
__global__ __launch_bounds__(SOLVE_THREADS) void dense_solve_multi_kernel(const double* __restrict__ K, int r, int parts,
                                                                          const double* __restrict__ B,
                                                                          double* __restrict__ X, long nrhs, int* info) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int lda = r | 1;
  double* A = sm;                                    // r x lda
  double* dummy = sm + (size_t)r * lda;              // r: the single right-hand side lu_solve_lds carries along
  int* perm = reinterpret_cast<int*>(dummy + r);     // r
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int i = wid; i < r; i += SOLVE_WAVES)
    for (int j = lane; j < r; j += 64) A[i * lda + j] = K[(size_t)i * r + j];
  for (int e = tid; e < r; e += SOLVE_THREADS) dummy[e] = 0.0;
  __syncthreads();
  const int sing = lu_solve_lds<SOLVE_THREADS>(A, lda, dummy, r, parts, dummy, perm);   // (its own solve goes to LDS, unused)
  __syncthreads();
  if (info && tid == 0 && blockIdx.x == 0) info[0] = sing ? RT_WARN_SINGULAR : 0;
  const long col = (long)blockIdx.x * SOLVE_THREADS + tid;
  if (col >= nrhs) return;
  // forward: y_c = b[p_c] - sum_{k<c} L[p_c][k] y_k   (row p_c was live at every column k < c: its multipliers sit there)
  for (int c = 0; c < r; ++c) {
    const double* row = A + perm[c] * lda;
    double acc = B[(size_t)perm[c] * nrhs + col];
    for (int k = 0; k < c; ++k) acc = fma(-row[k], X[(size_t)k * nrhs + col], acc);
    X[(size_t)c * nrhs + col] = acc;
  }
  // back: x_c = (y_c - sum_{k>c} U[p_c][k] x_k) / U[p_c][c]
  for (int c = r - 1; c >= 0; --c) {
    const double* row = A + perm[c] * lda;
    double acc = X[(size_t)c * nrhs + col];
    for (int k = c + 1; k < r; ++k) acc = fma(-row[k], X[(size_t)k * nrhs + col], acc);
    X[(size_t)c * nrhs + col] = acc / row[c];
  }
}

// ---------------------------------------------------------------------------------------------------------
// Inverse tracking for the online sweep.  Consecutive time steps solve with matrices that differ by O(dt), and
// pivoted LU of an 80 x 80 system is a chain of ~80 x 3500 dependent cycles no matter how many threads help.
// Newton-Schulz  X <- X (2 I - K X)  converges quadratically to K^-1 from the previous step's inverse
// (||I - K X|| ~ 1e-4 -> 1e-8 -> 1e-16) and is two small GEMMs on the matrix cores per iteration, all operands
// resident in LDS.  One workgroup per system: iterate until the residual before the last update was < 1e-6
// (so < 1e-12 after it), then x = X b with one step of iterative refinement against K itself, which makes the
// answer as accurate as the direct solve.  Without a usable start (first step, or ||I - K X|| > 0.7) it
// restarts from X = K^T / (||K||_1 ||K||_inf), which always converges for a nonsingular K.
constexpr int NS_THREADS = 512;
constexpr int NS_MAX_ITER = 100;
constexpr int NS_REFINE_MAX = 8;         // refinement steps tried with the carried inverse before Newton-Schulz takes over
constexpr int NS_REFRESH_AFTER = 5;      // more steps than this: the answer stands, and X is refreshed for the steps to come
constexpr double NS_REFINE_TOL = 2e-15;  // ||b - K x|| <= tol ||b||: the floor of a refinement in working precision
constexpr double NS_REFINE_RATE = 0.3;   // a step must shrink the residual at least this much, or X is not worth keeping

enum NsOp { NS_SUM, NS_MAX };
// Sum or maximum of x over the workgroup: the waves' partials go through s_red and every thread combines them in wave
// order.  The maximum starts from the first wave's partial; the sum starts from +0.0 and ADDS the first partial to it,
// an addition kept on purpose: it makes eight partials of -0.0 come out as +0.0, as they always have.  (A build with
// -fno-signed-zeros or -ffast-math would fold it away; the build's flags must stay without them.)
template <NsOp OP>
__device__ __forceinline__ double ns_block_reduce(double x, double* s_red, int tid) {
  x = OP == NS_MAX ? rtw::wave_max(x) : rtw::wave_sum(x);
  __syncthreads();
  if ((tid & 63) == 0) s_red[tid >> 6] = x;
  __syncthreads();
  double t = OP == NS_MAX ? s_red[0] : 0.0 + s_red[0];
#pragma unroll
  for (int w = 1; w < NS_THREADS / 64; ++w) t = OP == NS_MAX ? fmax(t, s_red[w]) : t + s_red[w];
  return t;
}

constexpr int NS_NBI = 2, NS_NBJ = 3;   // a wave's block of output tiles is at most 2 x 3 for r <= 80 (tile_layout.h)
typedef d4 NsAcc[NS_NBI][NS_NBJ];

// How a system's solve ended (NsGroup::finish closes the step for all four), and what Newton-Schulz reports
enum NsRoute {
  NS_KEPT,            // the refinement solved it and X is good for the steps to come
  NS_REFRESHED,       // Newton-Schulz converged: X goes back refreshed
  NS_REFRESH_FAILED,  // the refinement solved it, the refresh of X did not converge
  NS_LU               // neither did: pivoted LU of the workgroup's copy of K
};
struct NsOutcome { int status, iters, restarts; };

// One workgroup's view of its system: the three padded matrices in LDS, the four work vectors, the thread's place.
// The stages of newton_solve_kernel are its members; all threads call each of them.
struct NsGroup {
  double *sK, *sX, *sT;   // [rp][S] each; sK padded with the identity
  double (*s_vec)[96];    // 0: b, 1: x, 2 and 3: scratch
  double* s_red;
  int r, rp, S, tid, lane, wid;

  // out_i = sum_j A[i][j] v[j] for the r rows of an LDS matrix (A, v, out in LDS; out may not be v): eight lanes
  // share a row (columns j == lane mod 8) and add up with three butterfly steps, 64 rows per pass of the workgroup.
  // No LDS scratch: the three padded matrices leave 3 KB of the CU's 160.  (One thread per row walked r LDS round
  // trips one after the other, four times per solve.)
  __device__ __forceinline__ void matvec(const double* A, const double* v, double* out) const {
    const int sub = lane & 7;
    for (int i0 = 0; i0 < r; i0 += NS_THREADS / 8) {
      const int i = i0 + (tid >> 3);
      double acc = 0.0;
      if (i < r) {
        const double* row = A + i * S;
        for (int j = sub; j < r; j += 8) acc = fma(row[j], v[j], acc);
      }
      acc += __shfl_xor(acc, 1);
      acc += __shfl_xor(acc, 2);
      acc += __shfl_xor(acc, 4);
      if (i < r && sub == 0) out[i] = acc;
    }
    __syncthreads();
  }

  // K, the carried inverse and (when the right-hand side is formed here: Mb != nullptr) M_N come in together: one
  // round of global loads, M_N parked in sT until the first product needs the space.  `wide`: r is a multiple of 16
  // and the three operands are 16-byte aligned.  Ends without a barrier.
  __device__ __forceinline__ void load(const double* Kb, const double* Xb, const double* Mb, int have_prev,
                                       bool wide) const {
    if (wide) {
      // a row is r / 2 <= 40 pairs, one 16-byte load per lane and row; the <= 10 rows of a wave for all three
      // matrices are in flight together
      constexpr int QMAX = 10;
      d2 kv[QMAX], xv[QMAX], mv[QMAX];
      const int j = 2 * lane;
#pragma unroll
      for (int q = 0; q < QMAX; ++q) {
        const int i = wid + 8 * q;
        const bool in = i < r && j < r;
        kv[q] = in ? *reinterpret_cast<const d2*>(Kb + i * r + j) : d2{0.0, 0.0};
        xv[q] = (in && have_prev) ? *reinterpret_cast<const d2*>(Xb + i * r + j) : d2{i == j ? 1.0 : 0.0, i == j + 1 ? 1.0 : 0.0};
        mv[q] = (in && Mb) ? *reinterpret_cast<const d2*>(Mb + i * r + j) : d2{0.0, 0.0};
      }
#pragma unroll
      for (int q = 0; q < QMAX; ++q) {
        const int i = wid + 8 * q;
        if (i < r && j < r) {
          *reinterpret_cast<d2*>(sK + i * S + j) = kv[q];
          *reinterpret_cast<d2*>(sX + i * S + j) = xv[q];
          if (Mb) *reinterpret_cast<d2*>(sT + i * S + j) = mv[q];
        }
      }
    } else {
      // rp <= 80: a wave has at most 10 rows (i = wid + 8 q) of at most 2 x 64 columns.  Fixed trip counts, loads of
      // half the rows issued before any LDS store: a loop over runtime bounds went load - wait - store twenty times
      constexpr int QH = 5;
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        double kv[QH][2], xv[QH][2], mv[QH][2];
#pragma unroll
        for (int q = 0; q < QH; ++q)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int i = wid + 8 * (QH * half + q), j = lane + 64 * c;
            const bool in = i < r && j < r;
            const double eye = (i == j) ? 1.0 : 0.0;
            kv[q][c] = in ? Kb[i * r + j] : eye;
            xv[q][c] = (in && have_prev) ? Xb[i * r + j] : eye;
            mv[q][c] = (in && Mb) ? Mb[i * r + j] : 0.0;
          }
#pragma unroll
        for (int q = 0; q < QH; ++q)
#pragma unroll
          for (int c = 0; c < 2; ++c) {
            const int i = wid + 8 * (QH * half + q), j = lane + 64 * c;
            if (i < rp && j < rp) {
              sK[i * S + j] = kv[q][c];
              sX[i * S + j] = xv[q][c];
              if (Mb) sT[i * S + j] = mv[q][c];
            }
          }
      }
    }
  }

  // The refreshed inverse goes back the way it came: one 16-byte store per lane and row, or entry by entry
  __device__ __forceinline__ void store_X(double* Xb, bool wide) const {
    if (wide) {
      const int j = 2 * lane;
      d2 xv[10];
#pragma unroll
      for (int q = 0; q < 10; ++q) {
        const int i = wid + 8 * q;
        if (i < r && j < r) xv[q] = *reinterpret_cast<const d2*>(sX + i * S + j);
      }
#pragma unroll
      for (int q = 0; q < 10; ++q) {
        const int i = wid + 8 * q;
        if (i < r && j < r) *reinterpret_cast<d2*>(Xb + i * r + j) = xv[q];
      }
    } else {
      for (int i = wid; i < r; i += NS_THREADS / 64)
        for (int j = lane; j < r; j += 64) Xb[i * r + j] = sX[i * S + j];
    }
  }

  // b into s_vec[0], visible on return.  With a recipe: b = M_N (c0 u^n + c1 u^{n-1}) + dt Zf^T F_rhs, M_N out of sT
  // (also left in rb for the fallback); row i is thread i's: r FMAs out of LDS and mf independent loads - a wave per
  // row with a cross-lane sum took a chain of r / 8 global round trips per wave.  Without: rb is given.
  __device__ __forceinline__ void right_hand_side(const rt_step_rhs& rq, int b, double* rb) const {
    if (rq.MN) {
      if (tid < r) s_vec[1][tid] = step_rhs_state(rq, b, r, tid);
      __syncthreads();
      const double f = (tid < r) ? step_rhs_forcing(rq, step_rhs_forcing_rows(rq, b), r, tid) : 0.0;
      matvec(sT, s_vec[1], s_vec[2]);
      if (tid < r) {
        const double v = fma(rq.dt, f, s_vec[2][tid]);
        s_vec[0][tid] = v;
        rb[tid] = v;
      }
    } else if (tid < r) {
      s_vec[0][tid] = rb[tid];
    }
    __syncthreads();
  }

  // C(ti, tj) = sum_k A[16 ti + i][k] B[k][16 tj + j] on the matrix cores, operands out of LDS.  A wave owns one
  // rectangular block of tiles, so a k-step costs ni + nj LDS reads for ni nj MFMAs (scattered tiles t = wid + 8 q
  // read two operands per MFMA and took 9 us per 80^3 product).
  __device__ __forceinline__ void tiles_product(const Blk& bk, const double* A, const double* Bm, NsAcc& acc) const {
    const int l15 = lane & 15, l4 = lane >> 4;
    const double* ap[NS_NBI];
    const double* bp[NS_NBJ];
#pragma unroll
    for (int i = 0; i < NS_NBI; ++i) ap[i] = A + (16 * (bk.i0 + (i < bk.ni ? i : 0)) + l15) * S + l4;
#pragma unroll
    for (int j = 0; j < NS_NBJ; ++j) bp[j] = Bm + l4 * S + 16 * (bk.j0 + (j < bk.nj ? j : 0)) + l15;
#pragma unroll
    for (int i = 0; i < NS_NBI; ++i)
#pragma unroll
      for (int j = 0; j < NS_NBJ; ++j) acc[i][j] = d4{0.0, 0.0, 0.0, 0.0};
    for (int k16 = 0; k16 < rp / 16; ++k16)   // rp is a multiple of 16: four k-steps per trip, unrolled
#pragma unroll
    for (int ku = 0; ku < 4; ++ku) {
      const int k4 = 4 * k16 + ku;
      double a[NS_NBI], bq[NS_NBJ];
#pragma unroll
      for (int i = 0; i < NS_NBI; ++i) a[i] = ap[i][4 * k4];
#pragma unroll
      for (int j = 0; j < NS_NBJ; ++j) bq[j] = bp[j][4 * k4 * S];
#pragma unroll
      for (int i = 0; i < NS_NBI; ++i)
#pragma unroll
        for (int j = 0; j < NS_NBJ; ++j)
          if (i < bk.ni && j < bk.nj)  // wave-uniform
            acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], bq[j], acc[i][j], 0, 0, 0);
    }
  }

  __device__ __forceinline__ void restart() const {  // X = K^T / (||K||_1 ||K||_inf)
    double rs = 0.0, cs = 0.0;
    if (tid < r) {
      for (int j = 0; j < r; ++j) {
        rs += fabs(sK[tid * S + j]);
        cs += fabs(sK[j * S + tid]);
      }
    }
    const double ninf = ns_block_reduce<NS_MAX>(rs, s_red, tid);
    const double n1 = ns_block_reduce<NS_MAX>(cs, s_red, tid);
    const double sc = 1.0 / (n1 * ninf);
    for (int i = wid; i < rp; i += NS_THREADS / 64)
      for (int j = lane; j < rp; j += 64) sX[i * S + j] = (i < r && j < r) ? sK[j * S + i] * sc : ((i == j) ? 1.0 : 0.0);
    __syncthreads();
  }

  // Refinement before refreshment.  The carried inverse is a PRECONDITIONER: x <- x + X (b - K x) contracts the error
  // by ||I - X K|| per step, two r x r mat-vecs each, against the two r^3 products of a Newton-Schulz update.
  // X was exact to ~1e-8 when it was last refreshed and K has moved by O(dt) per time step since, so a few refinement
  // steps reach the residual floor for many time steps in a row; only when they take more than NS_REFRESH_AFTER steps
  // (or do not contract) is X refreshed - and in the first case the answer is already there, the refresh is for the
  // steps to come.  31 -> ~15 us per step for 32 systems of 80.  Returns whether x (s_vec[1]) is the answer, in `used` steps.
  __device__ __forceinline__ bool refine(int& used) const {
    double bpart = (tid < r) ? s_vec[0][tid] * s_vec[0][tid] : 0.0;
    const double bnorm2 = ns_block_reduce<NS_SUM>(bpart, s_red, tid);
    matvec(sX, s_vec[0], s_vec[1]);                        // x = X b
    double prev = 1e300;
    for (int it = 0; it <= NS_REFINE_MAX; ++it) {
      matvec(sK, s_vec[1], s_vec[2]);                      // K x
      double rr = 0.0;
      if (tid < r) {
        const double e = s_vec[0][tid] - s_vec[2][tid];
        s_vec[2][tid] = e;
        rr = e * e;
      }
      const double rn2 = ns_block_reduce<NS_SUM>(rr, s_red, tid);   // barriers inside: the residual vector is complete
      if (!(rn2 == rn2)) break;                             // NaN: leave it to the tracked route and its fallbacks
      if (rn2 <= NS_REFINE_TOL * NS_REFINE_TOL * bnorm2 || (it > 0 && rn2 >= 0.25 * prev && rn2 <= 1e-26 * bnorm2)) {
        used = it;                                          // at the floor (or within a hair of it and no longer moving)
        return true;
      }
      if (it == NS_REFINE_MAX || rn2 > NS_REFINE_RATE * NS_REFINE_RATE * prev) break;   // out of steps / no contraction
      prev = rn2;
      matvec(sX, s_vec[2], s_vec[3]);                      // X r
      if (tid < r) s_vec[1][tid] += s_vec[3][tid];
      __syncthreads();
    }
    return false;
  }

  // X <- X (2 I - K X) until the residual ||I - K X||_F before the last update was < 1e-6; `restarted`: X is the safe
  // start already.  status 0, or RT_WARN_SINGULAR: NaN, or no convergence in NS_MAX_ITER updates.  The wave's block
  // of tiles is looked up HERE: the look-up is a read of constant memory, and in front of the kernel's first loads,
  // where every route pays for it, it made the sweeps' step 0.3 us slower (with a late exit of the common route).
  __device__ __forceinline__ NsOutcome newton_schulz(bool restarted) const {
    const Blk bk = tile_block(rp / 16, wid);
    NsOutcome o{RT_WARN_SINGULAR, 0, 0};
    for (int it = 0; it < NS_MAX_ITER; ++it) {
      ++o.iters;
      // T = K X and the residual ||I - T||_F
      double part = 0.0;
      NsAcc acc;
      tiles_product(bk, sK, sX, acc);
      tile_block_entries<NS_NBI, NS_NBJ>(bk, lane, [&](int i, int j, int c, int row, int col) {
        sT[row * S + col] = acc[i][j][c];
        const double e = ((row == col) ? 1.0 : 0.0) - acc[i][j][c];
        part = fma(e, e, part);
      });
      const double res = sqrt(ns_block_reduce<NS_SUM>(part, s_red, tid));  // barriers inside: sT complete
      if (res != res) break;  // NaN: singular to working precision (or bad input)
      if (!restarted && !(res < 0.7)) {  // the carried inverse is no contraction for this K: safe start instead
        restarted = true;
        o.restarts = 1;
        restart();
        continue;
      }
      // X <- 2 X - X T
      tiles_product(bk, sX, sT, acc);
      __syncthreads();  // every wave has finished reading the old X
      tile_block_entries<NS_NBI, NS_NBJ>(bk, lane, [&](int i, int j, int c, int row, int col) {
        sX[row * S + col] = 2.0 * sX[row * S + col] - acc[i][j][c];
      });
      __syncthreads();
      if (res < 1e-6) {
        o.status = 0;
        break;
      }
    }
    return o;
  }

  // x = X b, one refinement step against K:  x += X (b - K x); the answer goes to rb
  __device__ __forceinline__ void solve_refined(double* rb) const {
    matvec(sX, s_vec[0], s_vec[1]);
    const double x = (tid < r) ? s_vec[1][tid] : 0.0;
    matvec(sK, s_vec[1], s_vec[2]);
    if (tid < r) s_vec[2][tid] = s_vec[0][tid] - s_vec[2][tid];
    __syncthreads();
    matvec(sX, s_vec[2], s_vec[1]);
    if (tid < r) rb[tid] = x + s_vec[1][tid];
  }

  // The tracking gave up on this system (singular to working precision, or no contraction even from the safe start):
  // pivoted LU right here, out of the copy of K this workgroup already holds.  Returns the info word.
  __device__ __forceinline__ int lu_fallback(double* rb) const {
    const int lu_parts = NS_THREADS / r > 8 ? 8 : NS_THREADS / r;
    __syncthreads();
    return lu_solve_lds<NS_THREADS>(sK, S, s_vec[0], r, lu_parts, rb) ? RT_WARN_SINGULAR : 0;
  }

  // The one end of every route: the sweep's counters (rt_last_sweep_stats), the carried inverse zeroed where the next
  // call has to start afresh, the info word, and the sweep's end of step for system b (x is in rhs).
  __device__ __forceinline__ void finish(NsRoute route, const NsOutcome& ns, int code, int b, double* Xb, double* rhs,
                                         int* info, long* counters, const rt_advance& adv) const {
    if (tid == 0) {
      auto bump = [&](int slot, int by) { atomicAdd(reinterpret_cast<unsigned long long*>(&counters[slot]), (unsigned long long)by); };
      if (route != NS_KEPT) {
        bump(RT_CNT_NS_ITER, ns.iters);
        bump(RT_CNT_NS_RESTART, ns.restarts);
      }
      bump(RT_CNT_SOLVES, 1);
      if (route == NS_LU) bump(RT_CNT_LU_FALLBACK, 1);
    }
    if (route == NS_REFRESH_FAILED || route == NS_LU)
      for (int i = wid; i < r; i += NS_THREADS / 64)
        for (int j = lane; j < r; j += 64) Xb[i * r + j] = 0.0;
    if (info && tid == 0) info[b] = code;
    if (adv.enabled) {
      __syncthreads();  // the answer is complete and visible in this workgroup
      hsweep_advance_rows(adv, b, r, rhs, 1, s_vec[1], tid, NS_THREADS);
    }
  }
};

__global__ __launch_bounds__(NS_THREADS) void newton_solve_kernel(
    const double* __restrict__ K, double* __restrict__ Xinv, double* __restrict__ rhs, int r, int S, int have_prev,
    int* __restrict__ info, const rt_step_rhs rq, long* counters, const rt_advance adv) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  __shared__ double s_red[NS_THREADS / 64];
  __shared__ double s_vec[4][96];   // r <= 80 here (three padded r x r matrices in the dynamic part)
  const int tr = (r + 15) / 16, rp = tr * 16, b = blockIdx.x;
  const int tid = threadIdx.x, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const NsGroup g{sm, sm + (size_t)rp * S, sm + 2 * (size_t)rp * S, s_vec, s_red, r, rp, S, tid, tid & 63, wid};
  const double* Kb = K + (size_t)b * r * r;
  double* Xb = Xinv + (size_t)b * r * r;
  double* rb = rhs + (size_t)b * r;
  const double* Mb = rq.MN ? step_rhs_mn(rq, b, r) : nullptr;
  const bool wide = (r == rp) && ((reinterpret_cast<size_t>(Kb) | reinterpret_cast<size_t>(Xb) | reinterpret_cast<size_t>(Mb)) & 15) == 0;

  g.load(Kb, Xb, Mb, have_prev, wide);
  g.right_hand_side(rq, b, rb);
  if (!have_prev) g.restart();

  // the carried inverse as a preconditioner first; X is refreshed when that took many steps, or did not get there
  int used = 0;
  const bool solved = have_prev && g.refine(used);
  if (solved && tid < r) rb[tid] = g.s_vec[1][tid];

  if (solved && used <= NS_REFRESH_AFTER) {   // nearly every step of a sweep ends here, so it leaves at once
    g.finish(NS_KEPT, NsOutcome{0, 0, 0}, 0, b, Xb, rhs, info, counters, adv);
    return;
  }
  const NsOutcome ns = g.newton_schulz(!have_prev);
  const NsRoute route = ns.status == 0 ? NS_REFRESHED : solved ? NS_REFRESH_FAILED : NS_LU;
  const int code = route == NS_LU ? g.lu_fallback(rb) : 0;
  if (route == NS_REFRESHED) {
    if (!solved) g.solve_refined(rb);
    g.store_X(Xb, wide);
  }   // NS_REFRESH_FAILED: the refinement had already delivered the answer
  g.finish(route, ns, code, b, Xb, rhs, info, counters, adv);
}

}  // namespace

extern "C" int rt_dense_solve_batched(rt_ctx* ctx, double* K, double* rhs, int64_t r, int64_t B, int* info) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, K && rhs && r >= 1 && B >= 1);
  if (r > 128) {
    ctx->err = "rt_dense_solve_batched: r > 128 not supported (matrix must fit the CU's LDS)";
    return RT_ERR_UNSUPPORTED;
  }
  const int lda = (int)r | 1;
  const size_t lds = sizeof(double) * ((size_t)r * lda + r);
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&dense_solve_kernel), 140 * 1024));
  int parts = SOLVE_THREADS / (int)r;  // threads per row
  if (parts > 8) parts = 8;
  hipLaunchKernelGGL(dense_solve_kernel, dim3((unsigned)B), dim3(SOLVE_THREADS), lds, ctx->stream, K, rhs, (int)r,
                     parts, info);
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

extern "C" int rt_dense_solve_multi(rt_ctx* ctx, const double* K, int64_t r, const double* B, double* X, int64_t nrhs,
                                   int* info) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, K && B && X && B != X && r >= 1 && nrhs >= 1);
  if (r > 128) {
    ctx->err = "rt_dense_solve_multi: r > 128 not supported (the factors must fit the CU's LDS)";
    return RT_ERR_UNSUPPORTED;
  }
  const int lda = (int)r | 1;
  const size_t lds = sizeof(double) * ((size_t)r * lda + r) + sizeof(int) * (size_t)r;
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&dense_solve_multi_kernel), 140 * 1024));
  int parts = SOLVE_THREADS / (int)r;
  if (parts > 8) parts = 8;
  const unsigned grid = (unsigned)((nrhs + SOLVE_THREADS - 1) / SOLVE_THREADS);
  hipLaunchKernelGGL(dense_solve_multi_kernel, dim3(grid), dim3(SOLVE_THREADS), lds, ctx->stream, K, (int)r, parts, B, X,
                     (long)nrhs, info);
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

// Internal (sweep.hip): solve K_b x_b = rhs_b while tracking K_b^-1 in Xinv (B x r x r, caller-owned, carried
// from call to call).  have_prev = 0 on the first call.  RT_ERR_UNSUPPORTED when three padded r x r matrices
// do not fit the LDS (r > 80): the caller uses rt_dense_solve_batched.  With `recipe` the kernel forms the
// right-hand side itself (and leaves it in rhs) instead of reading it.
int rt_newton_solve_batched(rt_ctx* ctx, const double* K, double* Xinv, double* rhs, int64_t r, int64_t B,
                            int have_prev, int* info, const rt_step_rhs* recipe, const rt_advance* advance) {
  const int rp = (int)((r + 15) / 16) * 16;
  int S = rp;
  while (S % 4 != 2) ++S;  // 2 S == 4 (mod 8): the 16 rows of an A-operand read fall in distinct LDS banks
  const size_t lds = sizeof(double) * 3 * (size_t)rp * S;
  if (lds > 155 * 1024) return RT_ERR_UNSUPPORTED;  // + 3.1 KB of static LDS <= the CU's 160 KB
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&newton_solve_kernel), 155 * 1024));
  hipLaunchKernelGGL(newton_solve_kernel, dim3((unsigned)B), dim3(NS_THREADS), lds, ctx->stream, K, Xinv, rhs, (int)r, S,
                     have_prev, info, recipe ? *recipe : rt_step_rhs{}, ctx->dev_counters, advance ? *advance : rt_advance{});
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

extern "C" int rt_tracked_solve_batched(rt_ctx* ctx, const double* K, double* Xinv, double* rhs, int64_t r, int64_t B,
                                        int have_prev, int* info) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, K && Xinv && rhs && r >= 1 && B >= 1);
  return rt_newton_solve_batched(ctx, K, Xinv, rhs, r, B, have_prev ? 1 : 0, info, nullptr, nullptr);
}
