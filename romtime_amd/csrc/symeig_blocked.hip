// rt_sym_eig_blocked: leading eigenpairs of a positive semi-definite Gram matrix of 2049 .. 16384 snapshots by a block
// Rayleigh-Ritz step, with the device eigensolver (symeig.hip) used only at the sizes it already takes (DESIGN.md,
// "Block Rayleigh-Ritz").
//
//   cut the columns into p = ceil(n / 2048) contiguous blocks -> eigenpairs of every diagonal block G_bb
//   (rt_sym_eig_values / rt_sym_eig_vectors) -> keep in each block the rho_b eigenvectors W_b above floor_rel lam_max ->
//   W = blockdiag(W_b), n x R -> G_M = sym(W^T G W), R x R -> its eigenpairs (theta, Y) -> Ritz pairs (theta, W Y) of G.
//
// lam_max is known only after the last block, while a block's eigenvectors must directly follow its eigenvalues (the
// reflectors live in the ctx's composite arena).  So block b asks for the vectors above floor_rel times the RUNNING
// maximum - a threshold that only grows, hence a superset - and the final rho_b takes the leading columns of those.
// The host work here is counting eigenvalues; everything of size n stays on the device.  The products use the block
// structure: G W is p panel GEMMs (column panel b of G times W_b), W^T (G W) and W Y likewise - rt_gemm_strided without
// contraction splits, so that every entry is one chain of MFMAs in index order whatever the ctx's CU count: the same
// bits on a CU-masked stream ("cu_limit") as on the whole chip.
#include <algorithm>
#include <vector>

#include "common.h"

namespace {

constexpr int64_t BLOCK_MAX = 2048;      // the device eigensolver's limit
constexpr int64_t BLOCKED_MAX_N = 16384;
constexpr int MAX_BLOCKS = 8;

// dst (rows x cols, leading dimension ldd) = src (rows x cols, lds): the gather of a diagonal block of G into a contiguous
// work matrix, and the scatter of a block's kept eigenvectors into the block-diagonal W.  One row per blockIdx.y; a thread
// moves two doubles that are 16-byte aligned in dst - the pairing of a row starts one element early where the row itself
// starts 8 bytes past such an address - as one 16-byte access on either side where the source pair is aligned as well, and
// as two 8-byte loads feeding one 16-byte store where it is not.  Lane i is at base + 16 i either way.
__global__ __launch_bounds__(256) void block_copy_kernel(const double* __restrict__ src, long lds, double* __restrict__ dst,
                                                         long ldd, int rows, int cols) {
  const int i = blockIdx.y;
  if (i >= rows) return;
  const double* s = src + (long)i * lds;
  double* d = dst + (long)i * ldd;
  const int shift = (int)((reinterpret_cast<uintptr_t>(d) >> 3) & 1);   // 1: d[0] sits 8 bytes past a 16-byte boundary
  const int j = 2 * (int)(blockIdx.x * blockDim.x + threadIdx.x) - shift;
  if (j >= cols) return;
  if (j >= 0 && j + 1 < cols) {
    d2 v;
    if (((reinterpret_cast<uintptr_t>(s + j) >> 3) & 1) == 0) {
      v = *reinterpret_cast<const d2*>(s + j);
    } else {
      v[0] = s[j];
      v[1] = s[j + 1];
    }
    *reinterpret_cast<d2*>(d + j) = v;
  } else {   // the first element of a shifted row, the last of a row that ends on an odd one
    if (j >= 0) d[j] = s[j];
    if (j + 1 >= 0 && j + 1 < cols) d[j + 1] = s[j + 1];
  }
}

// A <- (A + A^T) / 2 in place (R x R row-major): tile (bi, bj), bi <= bj, and its mirror image go through the LDS so that
// both are read and written along rows; a + b = b + a in IEEE arithmetic, so the result is exactly symmetric.
__global__ __launch_bounds__(256) void symmetrise_kernel(double* __restrict__ A, int R) {
  __shared__ double up[32][33], lo[32][33];
  const int bi = blockIdx.y, bj = blockIdx.x;
  if (bi > bj) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int rr = ty; rr < 32; rr += 8) {
    const int iu = bi * 32 + rr, ju = bj * 32 + tx;         // (iu, ju) in the upper tile
    const int il = bj * 32 + rr, jl = bi * 32 + tx;         // (il, jl) in the lower tile
    up[rr][tx] = (iu < R && ju < R) ? A[(long)iu * R + ju] : 0.0;
    lo[rr][tx] = (il < R && jl < R) ? A[(long)il * R + jl] : 0.0;
  }
  __syncthreads();
  for (int rr = ty; rr < 32; rr += 8) {
    const int iu = bi * 32 + rr, ju = bj * 32 + tx;
    const int il = bj * 32 + rr, jl = bi * 32 + tx;
    if (iu < R && ju < R) A[(long)iu * R + ju] = 0.5 * (up[rr][tx] + lo[tx][rr]);
    if (bi != bj && il < R && jl < R) A[(long)il * R + jl] = 0.5 * (lo[rr][tx] + up[tx][rr]);
  }
}

// Eigenpairs of a symmetric R x R matrix, R = 1 or 2, in closed form (one Jacobi rotation, the formulas of
// rt_host_jacobi_eigh): theta (R, descending), Y (R x kk row-major, kk <= R).
__global__ void tiny_eig_kernel(const double* __restrict__ A, int R, int kk, double* __restrict__ theta, double* __restrict__ Y) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (R == 1) {
    theta[0] = A[0];
    if (kk > 0) Y[0] = 1.0;
    return;
  }
  const double a = A[0], b = A[1], c = A[3];
  double cs = 1.0, sn = 0.0, l0 = a, l1 = c;
  if (b != 0.0) {
    const double zeta = (c - a) / (2.0 * b);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    cs = 1.0 / sqrt(1.0 + t * t);
    sn = cs * t;
    l0 = a - t * b;
    l1 = c + t * b;
  }
  // eigenvectors (cs, -sn) of l0 and (sn, cs) of l1
  double v[2][2] = {{cs, sn}, {-sn, cs}};   // v[row][column]
  const bool swap = l1 > l0;
  theta[0] = swap ? l1 : l0;
  theta[1] = swap ? l0 : l1;
  for (int t = 0; t < kk; ++t) {
    const int col = swap ? 1 - t : t;
    Y[0 * kk + t] = v[0][col];
    Y[1 * kk + t] = v[1][col];
  }
}

// The Ritz vectors W Y are products of two matrices with orthonormal columns, each orthonormal to its eigensolver's
// accuracy: their norms come out some tens of eps from one.  They are scaled to norm one as a direct solve's vectors are.
// Squares are summed per slice of NORM_ROWS rows (a thread takes every fourth row of its column, the four partial sums
// are added in a fixed order), the slices of a column in a fixed order again: no atomics, grids from the sizes alone.
constexpr int NORM_ROWS = 128;

__global__ __launch_bounds__(256) void colnorm_partial_kernel(const double* __restrict__ W, int n, int kk, double* __restrict__ part) {
  __shared__ double red[4][64];
  const int c = threadIdx.x & 63, l = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + c;
  const int row0 = blockIdx.y * NORM_ROWS;
  double acc = 0.0;
  if (col < kk)
    for (int r = l; r < NORM_ROWS && row0 + r < n; r += 4) {
      const double v = W[(long)(row0 + r) * kk + col];
      acc = fma(v, v, acc);
    }
  red[l][c] = acc;
  __syncthreads();
  if (l == 0 && col < kk) part[(long)blockIdx.y * kk + col] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

__global__ __launch_bounds__(256) void colnorm_scale_kernel(double* __restrict__ W, int n, int kk, const double* __restrict__ part,
                                                            int slices) {
  __shared__ double red[4][64];
  const int c = threadIdx.x & 63, l = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + c;
  const int row0 = blockIdx.y * NORM_ROWS;
  double acc = 0.0;
  if (col < kk)
    for (int sl = l; sl < slices; sl += 4) acc += part[(long)sl * kk + col];
  red[l][c] = acc;
  __syncthreads();
  if (col >= kk) return;
  const double tot = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
  const double inv = tot > 0.0 ? 1.0 / sqrt(tot) : 0.0;
  for (int r = l; r < NORM_ROWS && row0 + r < n; r += 4) W[(long)(row0 + r) * kk + col] *= inv;
}

__global__ void blocked_count_kernel(long* counters, int not_reducible, long R) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  counters[not_reducible ? RT_CNT_EIG_BLOCKED_NOT_REDUCIBLE : RT_CNT_EIG_BLOCKED] += 1;
  counters[RT_CNT_EIG_BLOCKED_RANK] = R;
}

int plan(int64_t n, int64_t block_max, int64_t* p_out, int64_t* widths) {
  if (!p_out || n < 1 || block_max < 1) return RT_ERR_ARG;
  const int64_t p = (n + block_max - 1) / block_max;
  *p_out = p;
  if (p > MAX_BLOCKS) return RT_ERR_UNSUPPORTED;
  if (widths)
    for (int64_t b = 0; b < p; ++b) widths[b] = n / p + (b < n % p ? 1 : 0);
  return RT_OK;
}

// device memory of one call, from the stream-ordered pool (as rt_pod_orth takes its own): the ctx arenas belong to the
// eigensolver and the GEMMs called below
struct Work {
  hipStream_t st;
  std::vector<void*> ptrs;
  ~Work() { for (void* p : ptrs) (void)hipFreeAsync(p, st); }
  double* get(size_t count) {
    void* p = nullptr;
    if (hipMallocAsync(&p, sizeof(double) * (count ? count : 1), st) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return static_cast<double*>(p);
  }
};

int copy_block(rt_ctx* ctx, const double* src, int64_t lds, double* dst, int64_t ldd, int64_t rows, int64_t cols) {
  const unsigned gx = (unsigned)((cols / 2 + 1 + 255) / 256);   // pairs of a row, one more for a shifted start
  hipLaunchKernelGGL(block_copy_kernel, dim3(gx, (unsigned)rows), dim3(256), 0, ctx->stream, src, (long)lds, dst, (long)ldd,
                     (int)rows, (int)cols);
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

}  // namespace

extern "C" int rt_sym_eig_blocked_plan_info(int64_t n, int64_t block_max, int64_t* p_out, int64_t* widths) {
  return plan(n, block_max, p_out, widths);
}

extern "C" int rt_sym_eig_blocked(rt_ctx* ctx, const double* G, int64_t n, double floor_rel, int64_t k, double* lam, double* W,
                                  int64_t* resolved, int64_t* block_ranks, int* status) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, G && lam && resolved && block_ranks && status);
  if (n <= BLOCK_MAX) {
    ctx->err = "rt_sym_eig_blocked: n <= 2048 (rt_sym_eig_values takes these sizes directly)";
    return RT_ERR_ARG;
  }
  if (n > BLOCKED_MAX_N) {
    ctx->err = "rt_sym_eig_blocked: n > 16384 not supported";
    return RT_ERR_UNSUPPORTED;
  }
  RT_ARG_CHECK(ctx, floor_rel > 0.0 && k >= 0 && k <= n && (W || k == 0));
  hipStream_t st = ctx->stream;
  int64_t p = 0, width[MAX_BLOCKS], off[MAX_BLOCKS + 1];
  RT_TRY(plan(n, BLOCK_MAX, &p, width));
  off[0] = 0;
  for (int64_t b = 0; b < p; ++b) off[b + 1] = off[b] + width[b];
  *status = 0;
  *resolved = 0;
  for (int64_t b = 0; b < p; ++b) block_ranks[b] = 0;

  Work wk{st};
  const int64_t wmax = width[0];
  double* Gb = wk.get((size_t)wmax * wmax);   // the diagonal block, contiguous
  double* lam_b = wk.get(wmax);
  int* flag = reinterpret_cast<int*>(wk.get(1));
  if (!Gb || !lam_b || !flag) { ctx->err = "rt_sym_eig_blocked: hipMallocAsync failed"; return RT_ERR_HIP; }

  // trace(G_bb) >= lam_1(G_bb): floor_rel max_b trace(G_bb) is an upper bound of the final floor, so the eigenvalues above
  // it are a lower bound of the final ranks - once those pass 2048 the set is known not to be reducible
  std::vector<double> diag(n);
  RT_HIP_CHECK(ctx, hipMemcpy2DAsync(diag.data(), sizeof(double), G, sizeof(double) * (n + 1), sizeof(double), n,
                                     hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
  double trace_max = 0.0;
  for (int64_t b = 0; b < p; ++b) {
    double t = 0.0;
    for (int64_t i = off[b]; i < off[b + 1]; ++i) t += diag[i];
    trace_max = std::max(trace_max, t);
  }

  std::vector<std::vector<double>> spectra(p);
  std::vector<double*> Wb(p, nullptr);      // block b's vectors: width[b] x asked[b] row-major
  std::vector<int64_t> asked(p, 0);
  double run_max = 0.0;
  int64_t sure = 0;                         // lower bound of R from the blocks seen so far
  bool not_reducible = false;
  for (int64_t b = 0; b < p && !not_reducible; ++b) {
    const int64_t nb = width[b];
    RT_TRY(copy_block(ctx, G + off[b] * n + off[b], n, Gb, nb, nb, nb));
    RT_TRY(rt_sym_eig_values(ctx, Gb, nb, lam_b, flag));
    spectra[b].assign(nb, 0.0);
    int st_b = 0;
    RT_HIP_CHECK(ctx, hipMemcpyAsync(spectra[b].data(), lam_b, sizeof(double) * nb, hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipMemcpyAsync(&st_b, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (st_b != 0) {
      *status = RT_EIG_BLOCKED_SOLVE_FAILED;
      ctx->err = "rt_sym_eig_blocked: the eigensolve of a diagonal block timed out";
      return RT_OK;
    }
    const std::vector<double>& l = spectra[b];
    run_max = std::max(run_max, l[0]);
    int64_t superset = 0;
    for (int64_t i = 0; i < nb; ++i) {
      if (l[i] > floor_rel * run_max) ++superset;
      if (l[i] > floor_rel * trace_max) ++sure;
    }
    if (sure > BLOCK_MAX) { not_reducible = true; break; }
    asked[b] = superset;
    if (superset > 0) {
      Wb[b] = wk.get((size_t)nb * superset);
      if (!Wb[b]) { ctx->err = "rt_sym_eig_blocked: hipMallocAsync failed"; return RT_ERR_HIP; }
      RT_TRY(rt_sym_eig_vectors(ctx, nb, superset, lam_b, Wb[b]));
      // lam_b and the arena are reused by the next block: stream order keeps this block's kernels ahead of them
    }
  }

  int64_t R = 0, rho[MAX_BLOCKS], coff[MAX_BLOCKS + 1];
  coff[0] = 0;
  for (int64_t b = 0; b < p; ++b) {
    rho[b] = 0;
    // after the early exit above the ranks are the lower bounds that ended the pass (nothing for a block not reached)
    for (double v : spectra[b])
      if (v > floor_rel * (not_reducible ? trace_max : run_max)) ++rho[b];
    block_ranks[b] = rho[b];
    coff[b + 1] = coff[b] + rho[b];
    R += rho[b];
  }
  *resolved = R;
  if (R > BLOCK_MAX) not_reducible = true;
  if (not_reducible) {
    *status = 1;
    hipLaunchKernelGGL(blocked_count_kernel, dim3(1), dim3(64), 0, st, ctx->dev_counters, 1, (long)*resolved);
    RT_HIP_CHECK(ctx, hipGetLastError());
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return RT_OK;
  }

  const int64_t kk = std::min<int64_t>(k, R);
  RT_HIP_CHECK(ctx, hipMemsetAsync(lam, 0, sizeof(double) * n, st));
  if (R == 0) {   // G has no positive block eigenvalue: nothing resolved, lam is zero, W has no column
    hipLaunchKernelGGL(blocked_count_kernel, dim3(1), dim3(64), 0, st, ctx->dev_counters, 0, 0L);
    RT_HIP_CHECK(ctx, hipGetLastError());
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return RT_OK;
  }

  // W = blockdiag(W_b) (n x R), GW = G W (n x R), G_M = W^T GW (R x R)
  double* Wd = wk.get((size_t)n * R);
  double* GW = wk.get((size_t)n * R);
  double* GM = wk.get((size_t)R * R);
  double* Y = wk.get((size_t)R * std::max<int64_t>(kk, 1));
  if (!Wd || !GW || !GM || !Y) { ctx->err = "rt_sym_eig_blocked: hipMallocAsync failed"; return RT_ERR_HIP; }
  RT_HIP_CHECK(ctx, hipMemsetAsync(Wd, 0, sizeof(double) * (size_t)n * R, st));
  for (int64_t b = 0; b < p; ++b)
    if (rho[b] > 0) RT_TRY(copy_block(ctx, Wb[b], asked[b], Wd + off[b] * R + coff[b], R, width[b], rho[b]));
  for (int64_t b = 0; b < p; ++b)
    if (rho[b] > 0)   // GW[:, cols_b] = G[:, rows_b] W_b
      RT_TRY(rt_gemm_strided(ctx, G + off[b], 1, n, Wd + off[b] * R + coff[b], R, 1, width[b], n, rho[b], GW + coff[b], R, 1,
                             false, false));
  for (int64_t b = 0; b < p; ++b)
    if (rho[b] > 0)   // G_M[cols_b, :] = W_b^T GW[rows_b, :]
      RT_TRY(rt_gemm_strided(ctx, Wd + off[b] * R + coff[b], R, 1, GW + off[b] * R, R, 1, width[b], rho[b], R, GM + coff[b] * R,
                             R, 1, false, false));
  hipLaunchKernelGGL(symmetrise_kernel, dim3((unsigned)((R + 31) / 32), (unsigned)((R + 31) / 32)), dim3(256), 0, st, GM, (int)R);
  RT_HIP_CHECK(ctx, hipGetLastError());

  if (R >= 3) {
    RT_TRY(rt_sym_eig_values(ctx, GM, R, lam, flag));
    if (kk > 0) RT_TRY(rt_sym_eig_vectors(ctx, R, kk, lam, Y));
    int st_m = 0;
    RT_HIP_CHECK(ctx, hipMemcpyAsync(&st_m, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (st_m != 0) {
      *status = RT_EIG_BLOCKED_SOLVE_FAILED;
      ctx->err = "rt_sym_eig_blocked: the eigensolve of the projected matrix timed out";
      return RT_OK;
    }
  } else {
    hipLaunchKernelGGL(tiny_eig_kernel, dim3(1), dim3(64), 0, st, GM, (int)R, (int)kk, lam, Y);
    RT_HIP_CHECK(ctx, hipGetLastError());
  }
  for (int64_t b = 0; b < p && kk > 0; ++b) {
    if (rho[b] > 0) {   // (W Y)[rows_b, :] = W_b Y[cols_b, :]
      RT_TRY(rt_gemm_strided(ctx, Wd + off[b] * R + coff[b], 1, R, Y + coff[b] * kk, kk, 1, rho[b], width[b], kk,
                             W + off[b] * kk, kk, 1, false, false));
    } else {
      RT_HIP_CHECK(ctx, hipMemsetAsync(W + off[b] * kk, 0, sizeof(double) * (size_t)width[b] * kk, st));
    }
  }
  if (kk > 0) {
    const int slices = (int)((n + NORM_ROWS - 1) / NORM_ROWS);
    double* part = wk.get((size_t)slices * kk);
    if (!part) { ctx->err = "rt_sym_eig_blocked: hipMallocAsync failed"; return RT_ERR_HIP; }
    const dim3 grid((unsigned)((kk + 63) / 64), (unsigned)slices);
    hipLaunchKernelGGL(colnorm_partial_kernel, grid, dim3(256), 0, st, W, (int)n, (int)kk, part);
    hipLaunchKernelGGL(colnorm_scale_kernel, grid, dim3(256), 0, st, W, (int)n, (int)kk, part, slices);
    RT_HIP_CHECK(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(blocked_count_kernel, dim3(1), dim3(64), 0, st, ctx->dev_counters, 0, (long)R);
  RT_HIP_CHECK(ctx, hipGetLastError());
  RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
  return RT_OK;
}
