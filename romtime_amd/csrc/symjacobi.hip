// Two-sided Jacobi eigensolver for a symmetric n x n matrix in device memory (1 <= n <= 2048): the second-pass Gram
// matrix of the POD (pod.py, passes=2), which is graded and nearly diagonal.  The rotations, the relative stopping rule
//     |a_pq| <= eps sqrt(|a_pp a_qq|)
// and what they do with non-positive diagonal entries are those of rt_host_jacobi_eigh (host_dense.cpp; Demmel & Veselic
// 1992); the order is not: a round-robin tournament in place of the cyclic-by-rows order.
//
//  * Order.  m = n rounded up to even, P = m / 2.  Round t (0 <= t < m - 1) seats player 0 at position 0 and player
//    ((k - 1 - t) mod (m - 1)) + 1 at position k >= 1; pair i < P is (position i, position m - 1 - i).  The P pairs of a
//    round are disjoint, a sweep of m - 1 rounds meets every pair once, and for odd n the pair that holds player n
//    idles.  A function of n alone.
//  * One launch per round, both sides at once.  The new 2 x 2 block at rows (p, q) of pair i and columns (r, s) of pair j
//    is R_i^T B R_j of the old block alone, so a thread owns a block: it reads it from the old work copy and writes it to
//    the new one (two copies, swapped every round: the diagonal blocks other workgroups take their rotations from stay
//    intact while the round runs).  No second pass, no grid barrier, no workgroup waits for another.
//  * Exactly symmetric.  Block (i, j) with i < j applies the column rotation first and the row rotation second; block
//    (j, i) holds the transpose and applies the row rotation first: the same operations on the same operands in the same
//    order, so a_kl and a_lk stay bit-identical.  A rotated pair's diagonal block is written as the host routine writes
//    it: a_pp - t a_pq, a_qq + t a_pq and exact zeros.  No contraction to FMA anywhere: NumPy reproduces the bits.
//  * Tiles.  Positions are consecutive players, so the columns r_j (ascending) and s_j (descending) of 64 consecutive
//    pairs are two contiguous 512-byte runs of a row (one wrap per round aside): a wave owns 64 column pairs, a workgroup
//    64 column pairs x 16 row pairs (4 per wave), and recomputes the 64 + 16 rotations it needs from the old diagonal
//    blocks (three doubles per pair) into LDS.  Further workgroups of the same launch rotate the columns of W (64 column
//    pairs x 32 rows), in place: every entry of W belongs to one thread.
//  * Convergence.  One integer counter of applied rotations, zeroed before every sweep and read by the host after it, is
//    the only atomic; a sweep without rotations ends the loop.
//  * Grids and every operation depend on n alone - not on the CU count, a CU mask or placement: every rank of a
//    row-sharded POD gets the same bits from the same all-reduced matrix.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int JAC_MAX_N = 2048;
constexpr int JAC_TJ = 64;    // column pairs of a tile: the lanes of a wave
constexpr int JAC_TI = 16;    // row pairs of a tile of the matrix: 4 per wave
constexpr int JAC_TW = 32;    // rows of a tile of W: 8 per wave
constexpr int JAC_T = 256;
constexpr double JAC_EPS = 1.1102230246251565e-16;

struct JacParams {
  const double* Aold;
  double* Anew;
  double* W;
  int* rotated;   // applied rotations of the running sweep
  int n, m, P, round;
  int tiles_a;    // blockIdx.y below this: tiles of the matrix; from it on: tiles of W
};

struct JacRot {
  double c, s, t;
  int on;
};

__device__ __forceinline__ int jac_player(int pos, int round, int m) {
  if (pos == 0) return 0;
  int v = (pos - 1 - round) % (m - 1);
  if (v < 0) v += m - 1;
  return v + 1;
}

// rotation of pair `pair` from the old diagonal block; identity for an idle pair and under the stopping rule
__device__ __forceinline__ JacRot jac_rotation(const JacParams& jp, int pair) {
  JacRot r{1.0, 0.0, 0.0, 0};
  if (pair >= jp.P) return r;
  const int p = jac_player(pair, jp.round, jp.m), q = jac_player(jp.m - 1 - pair, jp.round, jp.m);
  if (p >= jp.n || q >= jp.n) return r;
  const double app = jp.Aold[(long)p * jp.n + p], aqq = jp.Aold[(long)q * jp.n + q], apq = jp.Aold[(long)p * jp.n + q];
  if (apq == 0.0 || fabs(apq) <= JAC_EPS * sqrt(fabs(app) * fabs(aqq))) return r;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
  r.c = 1.0 / sqrt(t * t + 1.0);
  r.s = t * r.c;
  r.t = t;
  r.on = 1;
  return r;
}

// (x, y) <- (c x - s y, s x + c y): the update of rt_host_jacobi_eigh, on two rows or on two columns
__device__ __forceinline__ void jac_apply(double c, double s, double& x, double& y) {
  const double nx = c * x - s * y, ny = s * x + c * y;
  x = nx;
  y = ny;
}

__global__ __launch_bounds__(JAC_T) void symjacobi_round_kernel(JacParams jp) {
  __shared__ double col_c[JAC_TJ], col_s[JAC_TJ], row_c[JAC_TI], row_s[JAC_TI], row_t[JAC_TI];
  __shared__ int col_on[JAC_TJ], row_on[JAC_TI];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = jp.n, m = jp.m;
  const bool w_tile = (int)blockIdx.y >= jp.tiles_a;
  const int j0 = blockIdx.x * JAC_TJ;
  const int i0 = w_tile ? 0 : blockIdx.y * JAC_TI;
  if (tid < JAC_TJ) {
    const JacRot r = jac_rotation(jp, j0 + tid);
    col_c[tid] = r.c; col_s[tid] = r.s; col_on[tid] = r.on;
  } else if (!w_tile && tid < JAC_TJ + JAC_TI) {
    const int k = tid - JAC_TJ;
    const JacRot r = jac_rotation(jp, i0 + k);
    row_c[k] = r.c; row_s[k] = r.s; row_t[k] = r.t; row_on[k] = r.on;
  }
  __syncthreads();
  const int j = j0 + lane;
  if (j >= jp.P) return;
  const int r = jac_player(j, jp.round, m), s = jac_player(m - 1 - j, jp.round, m);
  const bool vr = r < n, vs = s < n;   // at most one of them is the idle player n
  const double cj = col_c[lane], sj = col_s[lane];
  const bool on_j = col_on[lane] != 0;

  if (w_tile) {
    if (!on_j) return;   // W is rotated in place: nothing to move
    const int k0 = ((int)blockIdx.y - jp.tiles_a) * JAC_TW + wave * (JAC_TW / 4);
    for (int e = 0; e < JAC_TW / 4; ++e) {
      const int k = k0 + e;
      if (k >= n) break;
      double x = jp.W[(long)k * n + r], y = jp.W[(long)k * n + s];
      jac_apply(cj, sj, x, y);
      jp.W[(long)k * n + r] = x;
      jp.W[(long)k * n + s] = y;
    }
    return;
  }

  for (int e = 0; e < JAC_TI / 4; ++e) {
    const int li = wave * (JAC_TI / 4) + e, i = i0 + li;
    if (i >= jp.P) break;
    const int p = jac_player(i, jp.round, m), q = jac_player(m - 1 - i, jp.round, m);
    const bool vp = p < n, vq = q < n;
    double bpr = (vp && vr) ? jp.Aold[(long)p * n + r] : 0.0, bps = (vp && vs) ? jp.Aold[(long)p * n + s] : 0.0;
    double bqr = (vq && vr) ? jp.Aold[(long)q * n + r] : 0.0, bqs = (vq && vs) ? jp.Aold[(long)q * n + s] : 0.0;
    const double ci = row_c[li], si = row_s[li];
    const bool on_i = row_on[li] != 0;
    if (i == j) {
      if (on_i) {   // r == p, s == q: the pair's own block
        const double tq = row_t[li] * bps;
        bpr = bpr - tq;
        bqs = bqs + tq;
        bps = 0.0;
        bqr = 0.0;
        atomicAdd(jp.rotated, 1);
      }
    } else if (i < j) {
      if (on_j) { jac_apply(cj, sj, bpr, bps); jac_apply(cj, sj, bqr, bqs); }
      if (on_i) { jac_apply(ci, si, bpr, bqr); jac_apply(ci, si, bps, bqs); }
    } else {
      if (on_i) { jac_apply(ci, si, bpr, bqr); jac_apply(ci, si, bps, bqs); }
      if (on_j) { jac_apply(cj, sj, bpr, bps); jac_apply(cj, sj, bqr, bqs); }
    }
    if (vp && vr) jp.Anew[(long)p * n + r] = bpr;
    if (vp && vs) jp.Anew[(long)p * n + s] = bps;
    if (vq && vr) jp.Anew[(long)q * n + r] = bqr;
    if (vq && vs) jp.Anew[(long)q * n + s] = bqs;
  }
}

// work copy <- the upper triangle of A mirrored (the triangle rt_host_jacobi_eigh takes its a_pq from), W <- I
__global__ __launch_bounds__(JAC_T) void symjacobi_load_kernel(const double* __restrict__ A, double* __restrict__ work,
                                                               double* __restrict__ W, int n) {
  const long idx = (long)blockIdx.x * JAC_T + threadIdx.x;
  if (idx >= (long)n * n) return;
  const int i = (int)(idx / n), j = (int)(idx % n);
  work[idx] = i <= j ? A[idx] : A[(long)j * n + i];
  W[idx] = i == j ? 1.0 : 0.0;
}

// descending order of the diagonal, stable on ties by index: perm[rank] = index, lam[rank] = value; the status word
__global__ __launch_bounds__(JAC_T) void symjacobi_rank_kernel(const double* __restrict__ work, int n, double* __restrict__ lam,
                                                               int* __restrict__ perm, int* status, int status_value) {
  const int i = blockIdx.x * JAC_T + threadIdx.x;
  if (i == 0) *status = status_value;
  if (i >= n) return;
  const double di = work[(long)i * n + i];
  int rank = 0;
  for (int k = 0; k < n; ++k) {
    const double dk = work[(long)k * n + k];
    rank += (dk > di || (dk == di && k < i)) ? 1 : 0;
  }
  if (di != di) return;   // a NaN has no place in the order (and none is produced from finite input)
  lam[rank] = di;
  perm[rank] = i;
}

__global__ __launch_bounds__(JAC_T) void symjacobi_permute_kernel(const double* __restrict__ Wwork, const int* __restrict__ perm,
                                                                  int n, double* __restrict__ W) {
  const long idx = (long)blockIdx.x * JAC_T + threadIdx.x;
  if (idx >= (long)n * n) return;
  const int k = (int)(idx / n), jcol = (int)(idx % n);
  const int src = perm[jcol];
  W[idx] = (src >= 0 && src < n) ? Wwork[(long)k * n + src] : 0.0;
}

}  // namespace

extern "C" int rt_sym_jacobi_eigh(rt_ctx* ctx, const double* A, int64_t n, double* lam, double* W, int max_sweeps,
                                  int* sweeps_done, int* status) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, A && lam && W && status && n >= 1 && max_sweeps >= 1);
  if (n > JAC_MAX_N) {
    ctx->err = "rt_sym_jacobi_eigh: n > 2048 not supported (the limit of the device eigensolver)";
    return RT_ERR_UNSUPPORTED;
  }
  // composite arena: work copy (x2) | rotations W | perm | counter
  rt_carver a;
  const size_t nn = sizeof(double) * (size_t)n * n;
  const size_t o0 = a.add(nn), o1 = a.add(nn), oW = a.add(nn), oP = a.add(sizeof(int) * n), oC = a.add(sizeof(int));
  void* base = nullptr;
  RT_TRY(rt_scratch2(ctx, a.total(), &base));
  double* work[2] = {a.at<double>(base, o0), a.at<double>(base, o1)};
  double* Ww = a.at<double>(base, oW);
  int* perm = a.at<int>(base, oP);
  int* counter = a.at<int>(base, oC);
  hipStream_t st = ctx->stream;
  const unsigned cells = (unsigned)(((long)n * n + JAC_T - 1) / JAC_T);
  RT_HIP_CHECK(ctx, hipMemsetAsync(perm, 0xff, sizeof(int) * n, st));
  hipLaunchKernelGGL(symjacobi_load_kernel, dim3(cells), dim3(JAC_T), 0, st, A, work[0], Ww, (int)n);
  RT_HIP_CHECK(ctx, hipGetLastError());

  JacParams jp;
  jp.W = Ww; jp.rotated = counter;
  jp.n = (int)n; jp.m = (int)(n + (n & 1)); jp.P = jp.m / 2;
  jp.tiles_a = (jp.P + JAC_TI - 1) / JAC_TI;
  const int rounds = jp.m - 1;
  const dim3 grid((unsigned)((jp.P + JAC_TJ - 1) / JAC_TJ), (unsigned)(jp.tiles_a + (n + JAC_TW - 1) / JAC_TW));
  int cur = 0, sweeps = 0, converged = 0;
  while (sweeps < max_sweeps) {
    RT_HIP_CHECK(ctx, hipMemsetAsync(counter, 0, sizeof(int), st));
    for (int t = 0; t < rounds; ++t) {
      jp.Aold = work[cur]; jp.Anew = work[cur ^ 1]; jp.round = t;
      hipLaunchKernelGGL(symjacobi_round_kernel, grid, dim3(JAC_T), 0, st, jp);
      cur ^= 1;
    }
    RT_HIP_CHECK(ctx, hipGetLastError());
    ++sweeps;
    int rotated = 0;
    RT_HIP_CHECK(ctx, hipMemcpyAsync(&rotated, counter, sizeof(int), hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (rotated == 0) { converged = 1; break; }
  }
  hipLaunchKernelGGL(symjacobi_rank_kernel, dim3((unsigned)((n + JAC_T - 1) / JAC_T)), dim3(JAC_T), 0, st, work[cur], (int)n, lam,
                     perm, status, converged ? 0 : 1);
  hipLaunchKernelGGL(symjacobi_permute_kernel, dim3(cells), dim3(JAC_T), 0, st, Ww, perm, (int)n, W);
  RT_HIP_CHECK(ctx, hipGetLastError());
  if (sweeps_done) *sweeps_done = sweeps;
  ctx->last_grid = sweeps;
  ctx->last_splits = rounds;
  ctx->last_tile = (int64_t)grid.x * grid.y;
  return RT_OK;
}
