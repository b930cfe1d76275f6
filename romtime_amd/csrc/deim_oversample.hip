// One selection step of oversampled (M)DEIM (GappyPOD+E: Peherstorfer, Drmac, Gugercin, SIAM J. Sci. Comput. 42, 2020).
//
// With A = Phi[p, :] the rows picked so far, g = sigma_{m-1}^2 - sigma_m^2 the gap of its two smallest singular values
// and w the right singular vector of sigma_m (both from the host's tiny SVD), every row i of Phi gets
//     rho_i = ||Phi[i, :]||^2,  c_i = Phi[i, :] . w,  a_i = g + rho_i,  q_i = 4 g c_i^2,
//     score_i = q_i / (a_i + sqrt(max(a_i^2 - q_i, 0)))          (= a_i - sqrt(a_i^2 - q_i), without the cancellation),
// half of which is a lower bound on the growth of sigma_min^2 when row i joins, and the step returns the argmax over the
// rows whose byte in `taken` is zero (first maximum on ties) with the two largest scores.
//
// One pass over Phi, 8 N m bytes, nothing of size N stored: rho and c come from the row while it is in registers.
//   * column-major: lanes along the rows, two adjacent rows per thread (one 16-byte load per column where the basis is
//     aligned for it), the m columns in order - a wave's load is 1 KiB contiguous;
//   * row-major: L = 2 .. 16 lanes share a row (L the power of two covering min(m, 16)), lane s takes the entries
//     s, s + L, ... in order - a row's load is 8 L contiguous bytes, 128 at L = 16 - and the L partial sums meet on the
//     DPP path in the tree of rtw::wave_sum cut off at L lanes.
// The order of the sums of a row depends on the layout and m alone.  Each workgroup of OS_ROWS rows reduces its scores
// to (top1, index, top2) in the lexicographic order (score descending, index ascending) and a second launch of one
// workgroup merges the partials: no floating-point atomics, and the grid depends on N alone, so pick and top2 have the
// same bits on any CU share.
#include <cmath>

#include "common.h"
#include "top2.h"
#include "wave_ops.h"

namespace {

constexpr int OS_THREADS = 256;
constexpr int OS_ROWS = 2 * OS_THREADS;   // rows per workgroup, both layouts
constexpr int OS_MAX_M = 1024;            // w is staged in LDS (rt_deim_greedy's bound on m)
constexpr int64_t OS_MAX_N = (int64_t)0x7fffffff * 512;   // rt_deim_greedy counts its 512-row workgroups in an int

__device__ __forceinline__ double os_score(double rho, double c, double g) {
  const double a = g + rho;
  const double q = 4.0 * g * (c * c);
  if (!(q > 0.0)) return 0.0;            // g == 0 or c == 0: no growth (and a may be 0)
  const double rad = fmax(fma(a, a, -q), 0.0);
  return q / (a + sqrt(rad));
}

// the workgroup's Top2 to its slot of the partials
__device__ __forceinline__ void os_store_partial(Top2 best, double* pv1, long* pi1, double* pv2) {
  __shared__ Top2 s_red[OS_THREADS / 64];
  const int tid = threadIdx.x;
  best = top2_wave(best);
  if ((tid & 63) == 0) s_red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    Top2 t = s_red[0];
    for (int w = 1; w < OS_THREADS / 64; ++w) t = top2_merge(t, s_red[w]);
    pv1[blockIdx.x] = t.v1;
    pi1[blockIdx.x] = t.i1;
    pv2[blockIdx.x] = t.v2;
  }
}

__device__ __forceinline__ void os_stage_w(double* s_w, const double* __restrict__ w, int m) {
  for (int j = threadIdx.x; j < m; j += OS_THREADS) s_w[j] = w[j];
  __syncthreads();
}

// WIDE: ld is even and Phi 16-byte aligned, so rows (2 t, 2 t + 1) of a column are one aligned 16-byte word
template <bool WIDE>
__global__ __launch_bounds__(OS_THREADS) void os_col_major_kernel(const double* __restrict__ Phi, long N, int m, long ld,
                                                                  const double* __restrict__ w, double g,
                                                                  const unsigned char* __restrict__ taken,
                                                                  double* pv1, long* pi1, double* pv2) {
  __shared__ double s_w[OS_MAX_M];
  os_stage_w(s_w, w, m);
  const long row = (long)blockIdx.x * OS_ROWS + 2 * threadIdx.x;
  Top2 best = top2_none();
  if (row < N) {
    const bool two = row + 1 < N;   // the pair is read only where its second row exists: ld may equal N
    double r0 = 0.0, r1 = 0.0, c0 = 0.0, c1 = 0.0;
    const double* col = Phi + row;
#pragma unroll 8
    for (int j = 0; j < m; ++j) {
      double x0, x1;
      if (WIDE && two) {
        const d2 x = *reinterpret_cast<const d2*>(col + (long)j * ld);
        x0 = x.x;
        x1 = x.y;
      } else {
        x0 = col[(long)j * ld];
        x1 = two ? col[(long)j * ld + 1] : 0.0;
      }
      const double wj = s_w[j];
      r0 = fma(x0, x0, r0);
      c0 = fma(x0, wj, c0);
      r1 = fma(x1, x1, r1);
      c1 = fma(x1, wj, c1);
    }
    if (!taken[row]) best = Top2{os_score(r0, c0, g), row, -1.0};
    if (two && !taken[row + 1]) best = top2_merge(best, Top2{os_score(r1, c1, g), row + 1, -1.0});
  }
  os_store_partial(best, pv1, pi1, pv2);
}

// the sum over the L lanes of a row group (L consecutive lanes, L | 16), valid in the group's LAST lane: the first
// log2 L steps of rtw::wave_sum
template <int L>
__device__ __forceinline__ double os_group_sum(double x) {
  if (L >= 2) x += rtw::dpp_f64<0xb1>(x);    // quad_perm:[1,0,3,2]
  if (L >= 4) x += rtw::dpp_f64<0x4e>(x);    // quad_perm:[2,3,0,1]
  if (L >= 8) x += rtw::dpp_f64<0x114>(x);   // row_shr:4
  if (L >= 16) x += rtw::dpp_f64<0x118>(x);  // row_shr:8
  return x;
}

template <int L>
__global__ __launch_bounds__(OS_THREADS) void os_row_major_kernel(const double* __restrict__ Phi, long N, int m, long ld,
                                                                  const double* __restrict__ w, double g,
                                                                  const unsigned char* __restrict__ taken,
                                                                  double* pv1, long* pi1, double* pv2) {
  __shared__ double s_w[OS_MAX_M];
  os_stage_w(s_w, w, m);
  constexpr int GROUPS = OS_THREADS / L;   // rows per pass
  const int sub = threadIdx.x % L, grp = threadIdx.x / L;
  Top2 best = top2_none();
  for (int pass = 0; pass < OS_ROWS / GROUPS; ++pass) {
    const long row = (long)blockIdx.x * OS_ROWS + pass * GROUPS + grp;
    double r = 0.0, c = 0.0;
    if (row < N) {
      const double* src = Phi + row * ld;
#pragma unroll 4
      for (int j = sub; j < m; j += L) {
        const double x = src[j];
        r = fma(x, x, r);
        c = fma(x, s_w[j], c);
      }
    }
    r = os_group_sum<L>(r);   // all lanes take part: DPP reads its neighbours whether their row exists or not
    c = os_group_sum<L>(c);
    if (row < N && sub == L - 1 && !taken[row]) best = top2_merge(best, Top2{os_score(r, c, g), row, -1.0});
  }
  os_store_partial(best, pv1, pi1, pv2);
}

// the partials in lexicographic order -> pick (-1: every row is taken) and the two largest scores
__global__ __launch_bounds__(OS_THREADS) void os_finish_kernel(const double* __restrict__ pv1, const long* __restrict__ pi1,
                                                               const double* __restrict__ pv2, long nparts, long* pick,
                                                               double* top2) {
  __shared__ Top2 s_red[OS_THREADS / 64];
  const int tid = threadIdx.x;
  Top2 best = top2_none();
  for (long q = tid; q < nparts; q += OS_THREADS) best = top2_merge(best, Top2{pv1[q], pi1[q], pv2[q]});
  best = top2_wave(best);
  if ((tid & 63) == 0) s_red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    Top2 t = s_red[0];
    for (int w = 1; w < OS_THREADS / 64; ++w) t = top2_merge(t, s_red[w]);
    const bool none = t.v1 < 0.0;
    pick[0] = none ? -1 : t.i1;
    top2[0] = none ? -1.0 : t.v1;
    top2[1] = none ? -1.0 : t.v2;
  }
}

struct OsPlan {
  long nparts;
  int lanes;   // lanes per row (row-major), 1 for column-major
};

int os_plan(const double* Phi, int64_t N, int64_t m, int64_t ld, int layout, const double* w, double g, const void* taken,
            const void* pick, const void* top2, OsPlan* plan, const char** why) {
#define OS_ARG(cond)                                     \
  do {                                                   \
    if (!(cond)) {                                       \
      *why = "bad argument: " #cond;                     \
      return RT_ERR_ARG;                                 \
    }                                                    \
  } while (0)
  OS_ARG(Phi && w && taken && pick && top2);
  OS_ARG(N >= 1 && m >= 2);
  OS_ARG(layout == RT_ROW_MAJOR || layout == RT_COL_MAJOR);
  OS_ARG(ld >= (layout == RT_COL_MAJOR ? N : m));
  OS_ARG(std::isfinite(g) && g >= 0.0);
#undef OS_ARG
  if (N > OS_MAX_N || m > OS_MAX_M) {
    *why = "rt_deim_oversample_step: N or m beyond what rt_deim_greedy accepts (m <= 1024)";
    return RT_ERR_UNSUPPORTED;
  }
  int lanes = 1;
  if (layout == RT_ROW_MAJOR) {
    lanes = 2;
    while (lanes < 16 && lanes < m) lanes *= 2;
  }
  *plan = OsPlan{(long)((N + OS_ROWS - 1) / OS_ROWS), lanes};
  return RT_OK;
}

}  // namespace

int rt_deim_oversample_step_plan_info(const double* Phi, int64_t N, int64_t m, int64_t ld, int layout, const double* w, double g,
                                      const uint8_t* taken, const int64_t* pick, const double* top2, int64_t* info3) {
  OsPlan plan;
  const char* why = nullptr;
  RT_TRY(os_plan(Phi, N, m, ld, layout, w, g, taken, pick, top2, &plan, &why));
  if (info3) {
    info3[0] = plan.nparts;
    info3[1] = OS_ROWS;
    info3[2] = plan.lanes;
  }
  return RT_OK;
}

int rt_deim_oversample_step(rt_ctx* ctx, const double* Phi, int64_t N, int64_t m, int64_t ld, int layout, const double* w,
                            double g, const uint8_t* taken, int64_t* pick, double* top2) {
  if (!ctx) return RT_ERR_ARG;
  OsPlan plan;
  const char* why = nullptr;
  const int rc = os_plan(Phi, N, m, ld, layout, w, g, taken, pick, top2, &plan, &why);
  if (rc != RT_OK) {
    ctx->err = why;
    return rc;
  }
  rt_carver carve;
  const size_t o_v1 = carve.add(sizeof(double) * plan.nparts), o_v2 = carve.add(sizeof(double) * plan.nparts),
               o_i1 = carve.add(sizeof(long) * plan.nparts);
  void* scratch = nullptr;
  RT_TRY(rt_scratch(ctx, carve.total(), &scratch));
  double* pv1 = rt_carver::at<double>(scratch, o_v1);
  double* pv2 = rt_carver::at<double>(scratch, o_v2);
  long* pi1 = rt_carver::at<long>(scratch, o_i1);
  const dim3 grid((unsigned)plan.nparts), block(OS_THREADS);
  hipStream_t st = ctx->stream;
#define OS_LAUNCH(kernel) hipLaunchKernelGGL(kernel, grid, block, 0, st, Phi, (long)N, (int)m, (long)ld, w, g, taken, pv1, pi1, pv2)
  if (layout == RT_COL_MAJOR) {
    if ((ld & 1) == 0 && (reinterpret_cast<size_t>(Phi) & 15) == 0)
      OS_LAUNCH(os_col_major_kernel<true>);
    else
      OS_LAUNCH(os_col_major_kernel<false>);
  } else {
    switch (plan.lanes) {
      case 2: OS_LAUNCH(os_row_major_kernel<2>); break;
      case 4: OS_LAUNCH(os_row_major_kernel<4>); break;
      case 8: OS_LAUNCH(os_row_major_kernel<8>); break;
      default: OS_LAUNCH(os_row_major_kernel<16>); break;
    }
  }
#undef OS_LAUNCH
  RT_HIP_CHECK(ctx, hipGetLastError());
  hipLaunchKernelGGL(os_finish_kernel, dim3(1), block, 0, st, pv1, pi1, pv2, plan.nparts, reinterpret_cast<long*>(pick), top2);
  RT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_grid = plan.nparts;
  ctx->last_splits = plan.lanes;
  ctx->last_tile = OS_ROWS * 1000;
  return RT_OK;
}
