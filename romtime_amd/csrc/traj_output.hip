// Integrals of a pointwise function of whole reduced trajectories, without storing the lifted trajectory:
//   out[j][t] = scale[j][t] * sum_i w_i f(E_i . a_j[t])
// (the mass  int rho(u) dx  on the moving mesh per time step, compute_mass_conservation, fom/nonlinear.py:627-683: E is
// the basis evaluated at the quadrature points, w the quadrature weights of the unit interval, scale the domain length).
//
// traj_error.hip's structure with another epilogue: a workgroup (4 waves) owns 64 steps and walks down a slice of rows
// in stages of 32, the 64 x k coefficient block stays in LDS, the 32 x k stages of E go global -> registers -> LDS with
// the next stage in flight (traj_stage.h, shared with traj_error.hip), a stage's 32 weights travel with its rows, each
// wave multiplies one 16-row block by two 16-step tiles in the tile[row][step] orientation (steps along lane & 15), and
// folds w f(c0 + c1 z) into per-lane column sums that stay in registers until the slice is done.  Per accumulator word:
// one fma for the base, f, one multiply by the weight, one add - and one select, because rows past n_pts are predicated
// out: their operands are zero, so they evaluate f(c0), which is inf for c0 = 0 and p < 0, and inf * 0 would poison a
// finite sum.  Steps past nt also evaluate f(c0); they sit in lanes of their own and are never written.  With a general
// exponent the vector ALU's pow is what the kernel waits for, not the matrix cores: the MFMA stream of a stage is kp / 2
// instructions per wave against 8 pow.
//
// Nothing is accumulated with atomics: a workgroup writes its 64 partial sums to [trajectory][row slice][step], a second
// kernel adds the slices in order and applies scale.  The slicing is rt_trajectory_errors': it depends on n_pts, nt and
// the CU count only, so a trajectory's bits depend neither on n_traj nor on its place in the batch.
#include <cmath>

#include "common.h"
#include "traj_stage.h"

// the base is one explicit fma; the power, the weight and the sums are separate IEEE operations, as NumPy's are
#pragma clang fp contract(off)

namespace {

struct ToParams {
  const double *E, *A, *W;                                // W may be null (weights 1)
  double* part;                                           // partial sums [trajectory][slice][step]
  long lde, lda, stride_a, n_pts, nt, slice_rows;
  double c0, c1, pw;
  int k, kp, slices, step_blocks, ip;                     // ip: the exponent where it is an integer in 1 .. 8, else 0 (pow)
};

// b^n for n = 1 .. 8 (uniform), in the association the header states: b2 = b b, b4 = b2 b2, then
// b, b2, b2 b, b4, b4 b, b4 b2, (b4 b2) b, b4 b4
__device__ __forceinline__ double to_int_power(double b, int n) {
  const double b2 = b * b, b4 = b2 * b2;
  switch (n) {
    case 1: return b;
    case 2: return b2;
    case 3: return b2 * b;
    case 4: return b4;
    case 5: return b4 * b;
    case 6: return b4 * b2;
    case 7: return (b4 * b2) * b;
    default: return b4 * b4;
  }
}

__global__ __launch_bounds__(TE_THREADS, 2) void traj_output_kernel(const ToParams p) {
  extern __shared__ __attribute__((aligned(16))) double to_smem[];
  const int S = p.kp + 2;                                 // S / 2 odd: the 16 rows of an operand read fall in distinct banks
  const int hp = p.kp >> 1;
  double* sC = to_smem;                                   // [64 steps][S] coefficients
  double* sB = sC + TE_TB * S;                            // [32 rows][S] current stage of E
  double* sW = sB + TE_RS * S;                            // [32] its weights
  double* sRed = sW + TE_RS;                              // [wave][32 steps]
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rb = wid & 1, tg = wid >> 1;
  unsigned bid = blockIdx.x;
  const int sb = (int)(bid % (unsigned)p.step_blocks);
  bid /= (unsigned)p.step_blocks;
  const int slice = (int)(bid % (unsigned)p.slices);
  const long traj = (long)(bid / (unsigned)p.slices);
  const long t0 = (long)sb * TE_TB;
  const long row_lo = (long)slice * p.slice_rows;
  const long row_hi = row_lo + p.slice_rows < p.n_pts ? row_lo + p.slice_rows : p.n_pts;
  const double* A = p.A + traj * p.stride_a;

  te_load_coefficients(sC, A, p.lda, t0, p.nt, p.k, hp, S, tid);
  TeStageLoader stage;
  stage.init(p.E, p.lde, p.n_pts, p.k, hp, S, sB, tid);
  double wreg = 1.0;                                      // threads 0 .. 31: the weight of row r0 + tid
  auto fetch = [&](long r0) {
    stage.fetch(r0);
    if (p.W && tid < TE_RS) wreg = r0 + tid < p.n_pts ? p.W[r0 + tid] : 0.0;
  };
  auto commit = [&]() {
    stage.commit();
    if (tid < TE_RS) sW[tid] = wreg;
  };

  double sum[TE_TW][4];
#pragma unroll
  for (int j = 0; j < TE_TW; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) sum[j][c] = 0.0;

  fetch(row_lo);
  commit();
  __syncthreads();
  const double* fb = sB + (16 * rb + l15) * S + l4;       // operand words: index lane & 15, k = 4 k4 + (lane >> 4)
  const double* fc = sC + (16 * TE_TW * tg + l15) * S + l4;
  const double* fw = sW + 16 * rb + l4;                   // accumulator word c: row (lane >> 4) + 4 c of the block
  for (long r0 = row_lo; r0 < row_hi; r0 += TE_RS) {
    const bool more = r0 + TE_RS < row_hi;
    if (more) fetch(r0 + TE_RS);
    double wv[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) wv[c] = fw[4 * c];
    d4 acc[TE_TW];
#pragma unroll
    for (int j = 0; j < TE_TW; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    auto mma = [&](int k4) {
      const double b = fb[k4];
#pragma unroll
      for (int j = 0; j < TE_TW; ++j) {
        const double a = fc[16 * j * S + k4];
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, a, acc[j], 0, 0, 0);   // tile[row][step]
      }
    };
    int k4 = 0;
    for (; k4 + 16 <= p.kp; k4 += 16) {                   // four k-steps at a time: their operand reads go out together
#pragma unroll
      for (int i = 0; i < 4; ++i) mma(k4 + 4 * i);
    }
    for (; k4 < p.kp; k4 += 4) mma(k4);
    const long left = p.n_pts - r0 - 16 * rb - l4;        // word c is a row of E where 4 c < left
    if (p.ip) {
#pragma unroll
      for (int j = 0; j < TE_TW; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double f = to_int_power(__builtin_fma(p.c1, acc[j][c], p.c0), p.ip);
          const double term = wv[c] * f;
          sum[j][c] += 4 * c < left ? term : 0.0;
        }
    } else {
#pragma unroll
      for (int j = 0; j < TE_TW; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double f = pow(__builtin_fma(p.c1, acc[j][c], p.c0), p.pw);
          const double term = wv[c] * f;
          sum[j][c] += 4 * c < left ? term : 0.0;
        }
    }
    __syncthreads();
    if (more) commit();
    __syncthreads();
  }

  // column sums: over this lane's registers and the lanes that hold other rows of the same step, then over the two row
  // blocks, always in the same order
  double* red = sRed + wid * 32;
#pragma unroll
  for (int j = 0; j < TE_TW; ++j) {
    double v = (sum[j][0] + sum[j][1]) + (sum[j][2] + sum[j][3]);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (l4 == 0) red[16 * j + l15] = v;
  }
  __syncthreads();
  if (tid < TE_TB && t0 + tid < p.nt) {
    const int w0 = 2 * (tid >> 5), s = tid & 31;          // the waves of tile group tid / 32: row blocks 0 and 1
    p.part[(traj * p.slices + slice) * p.nt + t0 + tid] = sRed[w0 * 32 + s] + sRed[(w0 + 1) * 32 + s];
  }
}

__global__ __launch_bounds__(256) void traj_output_finish_kernel(const double* part, const double* scale, double* out, long nt,
                                                                 int slices, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long traj = idx / nt, t = idx - traj * nt;
  const long first = traj * slices * nt + t;
  double s = 0.0;
  for (int i = 0; i < slices; ++i) s += part[first + i * nt];
  out[idx] = scale ? scale[idx] * s : s;
}

struct ToPlan {
  long step_blocks, slices, slice_rows, grid;
};

// Argument checks and the slicing: host logic only, shared by the entry point and rt_trajectory_integrals_plan_info
int to_plan(int num_cus, const double* E, int64_t lde, const double* A, int64_t lda, int64_t n_pts, int64_t k, int64_t nt,
            int64_t n_traj, int fn, const double* par, const double* out, ToPlan* plan, const char** why) {
#define TO_ARG(cond)                       \
  do {                                     \
    if (!(cond)) {                         \
      *why = "bad argument: " #cond;       \
      return RT_ERR_ARG;                   \
    }                                      \
  } while (0)
  TO_ARG(num_cus > 0);
  TO_ARG(E && A && par && out);
  TO_ARG(n_pts > 0 && k > 0 && nt > 0 && n_traj > 0);
  TO_ARG(lde >= k && lda >= k);
  TO_ARG(fn == RT_FN_POWER);
#undef TO_ARG
  if (k > 128) {
    *why = "rt_trajectory_integrals: k > 128";
    return RT_ERR_UNSUPPORTED;
  }
  const long step_blocks = (nt + TE_TB - 1) / TE_TB;
  // row slices as rt_trajectory_errors cuts them: enough workgroups for four per CU where n_pts allows (whole stages)
  long slices = (4L * num_cus + step_blocks - 1) / step_blocks;
  const long most = (n_pts + TE_SLICE_ROWS - 1) / TE_SLICE_ROWS;
  if (slices > most) slices = most;
  if (slices < 1) slices = 1;
  const long slice_rows = ((n_pts + slices - 1) / slices + TE_RS - 1) / TE_RS * TE_RS;
  slices = (n_pts + slice_rows - 1) / slice_rows;
  const long grid = step_blocks * slices * n_traj;
  if (grid >= (1L << 31)) {
    *why = "rt_trajectory_integrals: more than 2^31 workgroups";
    return RT_ERR_UNSUPPORTED;
  }
  *plan = ToPlan{step_blocks, slices, slice_rows, grid};
  return RT_OK;
}

}  // namespace

int rt_trajectory_integrals_plan_info(int num_cus, const double* E, int64_t lde, const double* w, const double* A, int64_t lda,
                                      int64_t stride_a, const double* scale, int64_t n_pts, int64_t k, int64_t nt,
                                      int64_t n_traj, int fn, const double* par, const double* out, int64_t* info3) {
  (void)w;
  (void)stride_a;
  (void)scale;
  ToPlan plan;
  const char* why = nullptr;
  RT_TRY(to_plan(num_cus, E, lde, A, lda, n_pts, k, nt, n_traj, fn, par, out, &plan, &why));
  if (info3) {
    info3[0] = plan.grid;
    info3[1] = plan.slices;
    info3[2] = TE_RS * 1000 + TE_TB;
  }
  return RT_OK;
}

int rt_trajectory_integrals(rt_ctx* ctx, const double* E, int64_t lde, const double* w, const double* A, int64_t lda,
                            int64_t stride_a, const double* scale, int64_t n_pts, int64_t k, int64_t nt, int64_t n_traj,
                            int fn, const double* par, double* out) {
  if (!ctx) return RT_ERR_ARG;
  ToPlan plan;
  const char* why = nullptr;
  const int rc = to_plan(ctx->num_cus, E, lde, A, lda, n_pts, k, nt, n_traj, fn, par, out, &plan, &why);
  if (rc != RT_OK) {
    ctx->err = why;
    return rc;
  }
  const size_t part = (size_t)n_traj * plan.slices * nt;
  void* scratch = nullptr;
  RT_TRY(rt_scratch(ctx, part * 8, &scratch));
  const int kp = (int)((k + 3) / 4 * 4);
  const double pw = par[2];
  const int ip = (pw >= 1.0 && pw <= 8.0 && pw == std::floor(pw)) ? (int)pw : 0;
  ToParams p{E, A, w, static_cast<double*>(scratch), (long)lde, (long)lda, (long)stride_a, (long)n_pts, (long)nt,
             plan.slice_rows, par[0], par[1], pw, (int)k, kp, (int)plan.slices, (int)plan.step_blocks, ip};
  const int lds = ((TE_TB + TE_RS) * (kp + 2) + TE_RS + 4 * 32) * 8;
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&traj_output_kernel), ((TE_TB + TE_RS) * 130 + TE_RS + 4 * 32) * 8));
  hipLaunchKernelGGL(traj_output_kernel, dim3((unsigned)plan.grid), dim3(TE_THREADS), lds, ctx->stream, p);
  RT_HIP_CHECK(ctx, hipGetLastError());
  const long total = n_traj * nt;
  hipLaunchKernelGGL(traj_output_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, p.part, scale,
                     out, (long)nt, (int)plan.slices, total);
  RT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_grid = plan.grid;
  ctx->last_splits = plan.slices;
  ctx->last_tile = TE_RS * 1000 + TE_TB;
  return RT_OK;
}
