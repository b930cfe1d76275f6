// Rectangular least squares against ONE matrix for many right-hand sides: Householder QR in LDS.
//
// The interpolation matrix of oversampled (M)DEIM, PT_U = basis_fom[dofs, :], is m_s x m with m_s >= m.  Its theta fit
// (trans = 0: min ||A x - b||) and the folds of sweep.py and interpolation.py (trans = 1: the minimum-norm solution of
// A^T x = b, x = (A^+)^T b) both go through A = Q R; the normal equations would square cond(PT_U), which is the number
// oversampling exists to keep small.
//
// Every workgroup factorises A for itself, as dense_solve_multi_kernel does (solve.hip): reflector k is
//     v = x - alpha e_1,  x = A[k:, k],  alpha = -sign(x_0) ||x||,  H_k = I - v v^T / den,  den = ||x||^2 - alpha x_0,
// v kept in place below the diagonal (its head v_0, R's diagonal alpha and 1 / den in three short arrays), R above.
// Thread (column j, part) owns the rows k + part, k + part + parts, ... of column j: the partial sums x^T a_j meet in LDS
// and are added in a fixed order by every thread that needs them - two barriers per column.  The factor of column j is
// the QUOTIENT (x^T a_j - alpha a_kj) / den with den formed by the same expression from x^T x, so a column that equals
// column k bit for bit gets the factor 1.0 and is annihilated exactly: an exactly repeated column ends in an exactly
// zero diagonal of R (RT_WARN_SINGULAR).
// Then each thread takes one right-hand side; its vector lives in global memory with the right-hand-side index
// running fastest (coalesced), the factors are broadcast out of LDS.  A column's result depends on nothing but A and
// that column.
#include "common.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_MAX_ROWS = 256, LS_MAX_COLS = 128, LS_MAX_PARTS = 16;
constexpr long LS_MAX_WORDS = 18432;   // rows x (cols | 1) doubles of LDS for A: 144 KiB of the CU's 160

__host__ __device__ inline size_t ls_lds_bytes(int rows, int cols) {
  return sizeof(double) * ((size_t)rows * (cols | 1) + 4 * (size_t)cols + LS_THREADS);
}

__global__ __launch_bounds__(LS_THREADS) void dense_lstsq_kernel(const double* __restrict__ Ag, int rows, int cols, int parts,
                                                                 int trans, const double* __restrict__ B,
                                                                 double* __restrict__ X, double* __restrict__ work,
                                                                 long nrhs, int* info) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  const int lda = cols | 1;   // odd leading dimension: column walks hit distinct banks
  double* A = sm;                          // rows x lda
  double* s_v0 = A + (size_t)rows * lda;   // cols: head of every reflector
  double* s_diag = s_v0 + cols;            // cols: diagonal of R
  double* s_tinv = s_diag + cols;          // cols: 1 / den, 0 for a reflector that is the identity
  double* s_row = s_tinv + cols;           // cols: row k as it stood before reflector k
  double* s_part = s_row + cols;           // LS_THREADS >= parts x cols
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int i = wid; i < rows; i += LS_THREADS / 64)
    for (int j = lane; j < cols; j += 64) A[i * lda + j] = Ag[(size_t)i * cols + j];
  __syncthreads();

  const int j = tid % cols, part = tid / cols;
  const bool act = part < parts;
  int sing = 0;
  for (int k = 0; k < cols; ++k) {
    if (act) {
      double acc = 0.0;
      if (j >= k)
        for (int i = k + part; i < rows; i += parts) acc = fma(A[i * lda + k], A[i * lda + j], acc);
      s_part[part * cols + j] = acc;
      if (part == 0 && j >= k) s_row[j] = A[k * lda + j];   // its owner overwrites it below while others still need it
    }
    __syncthreads();
    double nrm2 = 0.0, d = 0.0;
    for (int q = 0; q < parts; ++q) nrm2 += s_part[q * cols + k];
    if (act && j > k)
      for (int q = 0; q < parts; ++q) d += s_part[q * cols + j];
    const double x0 = s_row[k];
    const double norm = sqrt(nrm2);
    const double alpha = (x0 >= 0.0) ? -norm : norm;
    const double v0 = x0 - alpha;
    const double den = fma(-alpha, x0, nrm2);
    const bool zero = !(den > 0.0) || !(nrm2 > 0.0);
    if (nrm2 == 0.0) sing = 1;
    if (act && j > k && !zero) {
      const double f = fma(-alpha, s_row[j], d) / den;
      for (int i = k + part; i < rows; i += parts) {
        const double vi = (i == k) ? v0 : A[i * lda + k];
        A[i * lda + j] = fma(-f, vi, A[i * lda + j]);
      }
    }
    if (tid == 0) {
      s_v0[k] = zero ? 0.0 : v0;
      s_diag[k] = zero ? 0.0 : alpha;
      s_tinv[k] = zero ? 0.0 : 1.0 / den;
    }
    __syncthreads();
  }
  if (info && tid == 0 && blockIdx.x == 0) info[0] = sing ? RT_WARN_SINGULAR : 0;

  const long col = (long)blockIdx.x * LS_THREADS + tid;
  if (col >= nrhs) return;
  // y <- H_k y for the vector Y[i * nrhs + col], i < rows
  auto reflect = [&](double* Y, int k) {
    double s = s_v0[k] * Y[(size_t)k * nrhs + col];
    for (int i = k + 1; i < rows; ++i) s = fma(A[i * lda + k], Y[(size_t)i * nrhs + col], s);
    s *= s_tinv[k];
    Y[(size_t)k * nrhs + col] = fma(-s, s_v0[k], Y[(size_t)k * nrhs + col]);
    for (int i = k + 1; i < rows; ++i) Y[(size_t)i * nrhs + col] = fma(-s, A[i * lda + k], Y[(size_t)i * nrhs + col]);
  };
  if (trans == 0) {
    // x = R^-1 (Q^T b)[:cols]:  y = H_{cols-1} .. H_0 b in the work array, then back substitution into X
    for (int i = 0; i < rows; ++i) work[(size_t)i * nrhs + col] = B[(size_t)i * nrhs + col];
    for (int k = 0; k < cols; ++k) reflect(work, k);
    for (int c = cols - 1; c >= 0; --c) {
      double acc = work[(size_t)c * nrhs + col];
      for (int q = c + 1; q < cols; ++q) acc = fma(-A[c * lda + q], X[(size_t)q * nrhs + col], acc);
      X[(size_t)c * nrhs + col] = acc / s_diag[c];
    }
  } else {
    // x = Q R^-T b:  forward substitution with R^T into the head of X, zeros below, then H_0 .. H_{cols-1} in reverse
    for (int c = 0; c < cols; ++c) {
      double acc = B[(size_t)c * nrhs + col];
      for (int q = 0; q < c; ++q) acc = fma(-A[q * lda + c], X[(size_t)q * nrhs + col], acc);
      X[(size_t)c * nrhs + col] = acc / s_diag[c];
    }
    for (int i = cols; i < rows; ++i) X[(size_t)i * nrhs + col] = 0.0;
    for (int k = cols - 1; k >= 0; --k) reflect(X, k);
  }
}

struct LsPlan {
  long grid;
  int parts;
  size_t lds;
};

int ls_plan(const double* A, int64_t rows, int64_t cols, int trans, const double* B, const double* X, int64_t nrhs, LsPlan* plan,
            const char** why) {
#define LS_ARG(cond)                                     \
  do {                                                   \
    if (!(cond)) {                                       \
      *why = "bad argument: " #cond;                     \
      return RT_ERR_ARG;                                 \
    }                                                    \
  } while (0)
  LS_ARG(A && B && X && B != X);
  LS_ARG(rows >= 1 && cols >= 1 && nrhs >= 1);
  LS_ARG(rows >= cols);
  LS_ARG(trans == 0 || trans == 1);
#undef LS_ARG
  if (cols > LS_MAX_COLS || rows > LS_MAX_ROWS || rows * (cols | 1) > LS_MAX_WORDS) {
    *why = "rt_dense_lstsq_multi: cols > 128, rows > 256 or rows x (cols | 1) > 18432 (the factors must fit the CU's LDS)";
    return RT_ERR_UNSUPPORTED;
  }
  const int64_t grid = (nrhs + LS_THREADS - 1) / LS_THREADS;
  if (grid >= ((int64_t)1 << 31)) {
    *why = "rt_dense_lstsq_multi: more than 2^31 workgroups";
    return RT_ERR_UNSUPPORTED;
  }
  int parts = LS_THREADS / (int)cols;   // threads per column
  if (parts > LS_MAX_PARTS) parts = LS_MAX_PARTS;
  *plan = LsPlan{(long)grid, parts, ls_lds_bytes((int)rows, (int)cols)};
  return RT_OK;
}

}  // namespace

int rt_dense_lstsq_multi_plan_info(const double* A, int64_t rows, int64_t cols, int trans, const double* B, const double* X,
                                   int64_t nrhs, int64_t* info3) {
  LsPlan plan;
  const char* why = nullptr;
  RT_TRY(ls_plan(A, rows, cols, trans, B, X, nrhs, &plan, &why));
  if (info3) {
    info3[0] = plan.grid;
    info3[1] = LS_THREADS;
    info3[2] = (int64_t)plan.lds;
  }
  return RT_OK;
}

int rt_dense_lstsq_multi(rt_ctx* ctx, const double* A, int64_t rows, int64_t cols, int trans, const double* B, double* X,
                         int64_t nrhs, int* info) {
  if (!ctx) return RT_ERR_ARG;
  LsPlan plan;
  const char* why = nullptr;
  const int rc = ls_plan(A, rows, cols, trans, B, X, nrhs, &plan, &why);
  if (rc != RT_OK) {
    ctx->err = why;
    return rc;
  }
  void* work = nullptr;
  if (trans == 0) RT_TRY(rt_scratch(ctx, sizeof(double) * (size_t)rows * (size_t)nrhs, &work));
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&dense_lstsq_kernel), (int)(sizeof(double) * (LS_MAX_WORDS + 4 * LS_MAX_COLS + LS_THREADS))));
  hipLaunchKernelGGL(dense_lstsq_kernel, dim3((unsigned)plan.grid), dim3(LS_THREADS), plan.lds, ctx->stream, A, (int)rows,
                     (int)cols, plan.parts, trans, B, X, static_cast<double*>(work), (long)nrhs, info);
  RT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_grid = plan.grid;
  ctx->last_splits = plan.parts;
  ctx->last_tile = LS_THREADS;
  return RT_OK;
}
