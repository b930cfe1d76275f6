// Full-order residual curves of whole reduced trajectories, without a full-order solve and without storing the lifted
// trajectory: with x^t = B a_j[t] (nodes 0 and nx taken as 0), step s of trajectory j is held against the step system of
// the full-order sweep (rt_p1_fom_bdf_sweep; the time loop of OneDimensionalSolver.solve, fom/base.py:693-831),
//   r_i = fma(-u_i, x_i+1, fma(-d_i, x_i, fma(-l_i, x_i-1, rhs_i))),   s_i = |l_i x_i-1| + |d_i x_i| + |u_i x_i+1| + |rhs_i|,
//   res[j][s] = sqrt(sum_i r_i^2),   scale[j][s] = sqrt(sum_i s_i^2)       over the interior rows i = 1 .. nx-1,
// the rows formed by p1_rows.h from the lifted states of the steps s-1 and s-2: pass D of the certified sweep, summed in
// the 2-norm and evaluated at a trajectory that is not the system's solution.
//
// The lift is traj_error.hip's: a workgroup (4 waves) holds a 64-step coefficient block in LDS and walks down a slice of
// rows in 32-row stages of B (global -> registers -> LDS with the next stage in flight, traj_stage.h); each wave
// multiplies one 16-row block by two 16-step tiles on the f64 matrix cores.  What is new is the epilogue: a row of a
// step needs the lifted values of the rows i-1, i, i+1 at the steps s, s-1, s-2.  The accumulators therefore go to a
// 32 x 64 LDS tile (every lifted value is computed once per stage and read from there), and the halo is OVERLAP, not
// carry: a stage evaluates its inner 30 rows and a block its last 62 steps, so consecutive stages share two rows of B
// and consecutive blocks two rows of coefficients (1/15 and 1/31 more MFMA work).  The two steps before a call's first
// are the coefficient rows a_init (or zero).  Nothing crosses a stage, slice or block seam, and every lifted value -
// halo or not - is the same chain of MFMAs over k, so its bits do not depend on where a seam falls.
//
// Epilogue: lane = step (the step's scalars, fom_step, sit in its registers from the start of the workgroup), wave w =
// rows 1 + 8 w .. of the stage, walked downwards with w and past of the two upper neighbours kept in registers: three LDS
// reads (conflict-free: a wave reads 64 consecutive words), two fom_w / fom_past and one fom_row per row and step.  It
// runs between the stage's two barriers, after the next stage's registers have gone to LDS; the stage loop itself holds
// no address arithmetic beyond the loader's.
//
// No floating-point atomics: the per-lane sums stay in registers down the slice, the four waves are added in order, the
// workgroup writes its 62 partial sums to [trajectory][row slice][step] and a second kernel adds the slices in order and
// takes the correctly rounded square root.  The slicing depends on nx and the CU count only.
#include <cmath>

#include "common.h"
#include "p1_rows.h"
#include "traj_stage.h"

namespace {

constexpr int TR_EV_ROWS = TE_RS - 2;                     // rows a stage evaluates (its first and last row are neighbours only)
constexpr int TR_EV_STEPS = TE_TB - 2;                    // steps a block evaluates (its first two are the older states)
constexpr int TR_SX = 80;                                 // words per row of the lifted tile: rows 4 apart fall 32 banks apart
constexpr int TR_CROWS = TE_TB + 2;                       // the first block loads its 64 steps below the two rows of a_init
constexpr long TR_SLICE_ROWS = 34 * TR_EV_ROWS;           // shortest row slice: whole stages
constexpr long TR_MAX_NX = 1L << 22;                      // the limit of rt_p1_fom_bdf_sweep

constexpr int tr_lds_bytes(int kp) { return ((TR_CROWS + TE_RS) * (kp + 2) + TE_RS * TR_SX + 2 * 4 * TE_TB) * 8; }

struct TrParams {
  const double *B, *A, *a_init, *tab;
  double *pres, *pscale;                                  // partial sums [trajectory][slice][step]; pscale may be null
  long ldb, lda, stride_a, nx, nt, n_mu, first_step, slice_rows;
  double dt;
  int k, kp, slices, step_blocks, bdf2, state_in_w;
};

struct TrPlan {
  long step_blocks, slices, slice_rows, grid;
};

__global__ __launch_bounds__(TE_THREADS, 2) void traj_residual_kernel(const TrParams p) {
  extern __shared__ __attribute__((aligned(16))) double tr_smem[];
  const int S = p.kp + 2;                                 // S / 2 odd: the 16 rows of an operand read fall in distinct banks
  const int hp = p.kp >> 1;
  double* sC = tr_smem;                                   // [66][S] coefficients: row c = step t0 + c of this call
  double* sB = sC + TR_CROWS * S;                         // [32 rows][S] current stage of B
  double* sX = sB + TE_RS * S;                            // [32 rows][TR_SX] lifted values of the stage, 64 steps
  double* sRed = sX + TE_RS * TR_SX;                      // [res | scale][wave][64 steps]
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rb = wid & 1, tg = wid >> 1;
  unsigned bid = blockIdx.x;
  const int sb = (int)(bid % (unsigned)p.step_blocks);
  bid /= (unsigned)p.step_blocks;
  const int slice = (int)(bid % (unsigned)p.slices);
  const long traj = (long)(bid / (unsigned)p.slices);
  const long t0 = (long)sb * TR_EV_STEPS - 2;             // step of the tile's first column; -1 and -2: the call's older states
  const int nx = (int)p.nx;
  const int e_lo = 1 + slice * (int)p.slice_rows;         // nodes e_lo .. e_hi - 1 are this slice's rows
  const int e_hi = e_lo + (int)p.slice_rows < nx ? e_lo + (int)p.slice_rows : nx;
  const double* A = p.A + traj * p.stride_a;
  const bool want_scale = p.pscale != nullptr;

  if (sb == 0) {
    te_load_coefficients(sC + 2 * S, A, p.lda, 0, p.nt, p.k, hp, S, tid);     // rows 2 .. 65; the tile reads 0 .. 63
    for (int q = tid; q < 2 * p.kp; q += TE_THREADS) {
      const int r = q / p.kp, c = q - r * p.kp;           // row 1 = a^n (step -1), row 0 = a^{n-1} (step -2)
      sC[r * S + c] = (p.a_init && c < p.k) ? p.a_init[(traj * 2 + (1 - r)) * p.k + c] : 0.0;
    }
  } else {
    te_load_coefficients(sC, A, p.lda, t0, p.nt, p.k, hp, S, tid);
  }
  TeStageLoader stage;
  stage.init(p.B, p.ldb, p.nx + 1, p.k, hp, S, sB, tid);

  // this lane's step: column `lane` of the tile
  const long t = t0 + lane;
  const bool valid = lane >= 2 && t < p.nt;
  FomStep T{};
  if (valid)
    T = fom_step(p.tab + ((size_t)t * p.n_mu + traj) * 7, p.dt, 1.0 / (double)p.nx, p.state_in_w ? 1.0 : 0.0,
                 p.bdf2 && p.first_step + t > 0);
  double sr = 0.0, ss = 0.0;

  stage.fetch(e_lo - 1);
  stage.commit();
  __syncthreads();
  const double* fb = sB + (16 * rb + l15) * S + l4;       // operand words: index lane & 15, k = 4 k4 + (lane >> 4)
  const double* fc = sC + (16 * TE_TW * tg + l15) * S + l4;
  double* xw = sX + (16 * rb + l4) * TR_SX + 16 * TE_TW * tg + l15;   // accumulator word (tile j, register c): + 4 c rows, + 16 j
  const double* xr = sX + lane;
  const int q_lo = 1 + 8 * wid, q_hi = q_lo + 8 < TE_RS - 1 ? q_lo + 8 : TE_RS - 1;   // this wave's rows of a stage
  for (int r0 = e_lo - 1; r0 + 1 < e_hi; r0 += TR_EV_ROWS) {
    const bool more = r0 + TR_EV_ROWS + 1 < e_hi;
    if (more) stage.fetch(r0 + TR_EV_ROWS);
    d4 acc[TE_TW];
#pragma unroll
    for (int j = 0; j < TE_TW; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    auto mma = [&](int k4) {
      const double b = fb[k4];
#pragma unroll
      for (int j = 0; j < TE_TW; ++j) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(b, fc[16 * j * S + k4], acc[j], 0, 0, 0);   // tile[row][step]
    };
    int k4 = 0;
    for (; k4 + 16 <= p.kp; k4 += 16) {                   // four k-steps at a time: their operand reads go out together
#pragma unroll
      for (int i = 0; i < 4; ++i) mma(k4 + 4 * i);
    }
    for (; k4 < p.kp; k4 += 4) mma(k4);
    // the Dirichlet nodes are zero whatever B holds there; rows past nx come out of the loader as zeros
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int node = r0 + 16 * rb + l4 + 4 * c;
      const bool inner = node > 0 && node < nx;
#pragma unroll
      for (int j = 0; j < TE_TW; ++j) xw[4 * c * TR_SX + 16 * j] = inner ? acc[j][c] : 0.0;
    }
    __syncthreads();
    if (more) stage.commit();
    if (valid && r0 + q_lo < e_hi) {
      const double* x = xr + (q_lo - 1) * TR_SX;
      double xl = x[0], unL = x[-1], vnL = x[-2];
      x += TR_SX;
      double xc = x[0], unC = x[-1], vnC = x[-2];
      double wL = fom_w(T, unL, vnL, r0 + q_lo - 1), wC = fom_w(T, unC, vnC, r0 + q_lo);
      double pL = fom_past(T, unL, vnL), pC = fom_past(T, unC, vnC);
      const int i_end = r0 + q_hi < e_hi ? r0 + q_hi : e_hi;
#pragma unroll
      for (int qq = 0; qq < 8; ++qq) {
        const int i = r0 + q_lo + qq;                     // node of this row
        if (i >= i_end) break;
        x += TR_SX;
        const double xR = x[0], unR = x[-1], vnR = x[-2];
        const double wR = fom_w(T, unR, vnR, i + 1), pR = fom_past(T, unR, vnR);
        double l, d, u, rhs;
        fom_row(T, wL, wC, wR, pL, pC, pR, i, l, d, u, rhs);
        if (i == 1) l = 0.0;                              // u_0 = u_nx = 0
        if (i == nx - 1) u = 0.0;
        const double res = fma(-u, xR, fma(-d, xc, fma(-l, xl, rhs)));
        sr += res * res;
        if (want_scale) {
          const double den = fabs(l * xl) + fabs(d * xc) + fabs(u * xR) + fabs(rhs);
          ss += den * den;
        }
        wL = wC, wC = wR, pL = pC, pC = pR, xl = xc, xc = xR;
      }
    }
    __syncthreads();
  }

  // the four waves hold different rows of the same steps: added in wave order
  sRed[wid * TE_TB + lane] = sr;
  sRed[(4 + wid) * TE_TB + lane] = ss;
  __syncthreads();
  if (tid < TE_TB && valid) {
    const long out = (traj * p.slices + slice) * p.nt + t;
    p.pres[out] = ((sRed[tid] + sRed[TE_TB + tid]) + sRed[2 * TE_TB + tid]) + sRed[3 * TE_TB + tid];
    if (want_scale)
      p.pscale[out] = ((sRed[4 * TE_TB + tid] + sRed[5 * TE_TB + tid]) + sRed[6 * TE_TB + tid]) + sRed[7 * TE_TB + tid];
  }
}

__global__ __launch_bounds__(256) void traj_residual_finish_kernel(const double* pres, const double* pscale, double* res,
                                                                   double* scale, long nt, int slices, long total) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long traj = idx / nt, t = idx - traj * nt;
  const long first = traj * slices * nt + t;
  double s = 0.0;
  for (int i = 0; i < slices; ++i) s += pres[first + i * nt];
  res[idx] = __dsqrt_rn(s);
  if (scale) {
    double q = 0.0;
    for (int i = 0; i < slices; ++i) q += pscale[first + i * nt];
    scale[idx] = __dsqrt_rn(q);
  }
}

// Argument checks and the slicing: host logic only, shared by the entry point and the plan query.  No pointer but desc is
// followed.
int tr_plan(int num_cus, const rt_fom_desc* d, const double* B, int64_t ldb, int64_t k, const double* A, int64_t lda,
            const double* a_init, const double* res, TrPlan* plan, const char** why) {
#define TR_ARG(cond)                       \
  do {                                     \
    if (!(cond)) {                         \
      *why = "bad argument: " #cond;       \
      return RT_ERR_ARG;                   \
    }                                      \
  } while (0)
  TR_ARG(num_cus > 0);
  TR_ARG(d && B && A && res);
  TR_ARG(d->tab);
  TR_ARG(d->u_init == nullptr);                           // the older states come as coefficients (a_init)
  TR_ARG(d->nx >= 2 && d->n_mu >= 1 && d->nt >= 1 && d->first_step >= 0 && k >= 1);
  TR_ARG(ldb >= k && lda >= k);
  TR_ARG(a_init || d->first_step == 0);
  TR_ARG(d->n_mu < (1L << 31) && d->nt < (1L << 40) && d->first_step < (1L << 30));
#undef TR_ARG
  if (d->nx > TR_MAX_NX) {
    *why = "rt_trajectory_residuals: nx > 2^22";
    return RT_ERR_UNSUPPORTED;
  }
  if (k > 128) {
    *why = "rt_trajectory_residuals: k > 128";
    return RT_ERR_UNSUPPORTED;
  }
  const long n = d->nx - 1;                               // interior rows
  const long step_blocks = (d->nt + TR_EV_STEPS - 1) / TR_EV_STEPS;
  // row slices: up to four workgroups per CU for ONE step block, never fewer than TR_SLICE_ROWS rows each (whole stages).
  // nt is not looked at: a step's bits are then the same however the horizon is cut into calls.
  long slices = 4L * num_cus;
  const long most = (n + TR_SLICE_ROWS - 1) / TR_SLICE_ROWS;
  if (slices > most) slices = most;
  if (slices < 1) slices = 1;
  const long slice_rows = ((n + slices - 1) / slices + TR_EV_ROWS - 1) / TR_EV_ROWS * TR_EV_ROWS;
  slices = (n + slice_rows - 1) / slice_rows;
  const long grid = step_blocks * slices * d->n_mu;
  if (grid >= (1L << 31)) {
    *why = "rt_trajectory_residuals: more than 2^31 workgroups";
    return RT_ERR_UNSUPPORTED;
  }
  *plan = TrPlan{step_blocks, slices, slice_rows, grid};
  return RT_OK;
}

}  // namespace

int rt_trajectory_residuals_plan_info(int num_cus, const rt_fom_desc* desc, const double* B, int64_t ldb, int64_t k,
                                      const double* A, int64_t lda, int64_t stride_a, const double* a_init, const double* res,
                                      const double* scale, int64_t* info3) {
  (void)stride_a;
  (void)scale;
  TrPlan plan;
  const char* why = nullptr;
  RT_TRY(tr_plan(num_cus, desc, B, ldb, k, A, lda, a_init, res, &plan, &why));
  if (info3) {
    info3[0] = plan.grid;
    info3[1] = plan.slices;
    info3[2] = TR_EV_ROWS * 1000 + TR_EV_STEPS;
  }
  return RT_OK;
}

int rt_trajectory_residuals(rt_ctx* ctx, const rt_fom_desc* desc, const double* B, int64_t ldb, int64_t k, const double* A,
                            int64_t lda, int64_t stride_a, const double* a_init, double* res, double* scale) {
  if (!ctx) return RT_ERR_ARG;
  TrPlan plan;
  const char* why = nullptr;
  const int rc = tr_plan(ctx->num_cus, desc, B, ldb, k, A, lda, a_init, res, &plan, &why);
  if (rc != RT_OK) {
    ctx->err = why;
    return rc;
  }
  const size_t part = (size_t)desc->n_mu * plan.slices * desc->nt;
  void* scratch = nullptr;
  RT_TRY(rt_scratch(ctx, part * 8 * (scale ? 2 : 1), &scratch));
  const int kp = (int)((k + 3) / 4 * 4);
  TrParams p{B, A, a_init, desc->tab, static_cast<double*>(scratch), scale ? static_cast<double*>(scratch) + part : nullptr,
             (long)ldb, (long)lda, (long)stride_a, (long)desc->nx, (long)desc->nt, (long)desc->n_mu, (long)desc->first_step,
             plan.slice_rows, desc->dt, (int)k, kp, (int)plan.slices, (int)plan.step_blocks, desc->bdf2 != 0,
             desc->state_in_w != 0};
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&traj_residual_kernel), tr_lds_bytes(128)));
  hipLaunchKernelGGL(traj_residual_kernel, dim3((unsigned)plan.grid), dim3(TE_THREADS), tr_lds_bytes(kp), ctx->stream, p);
  RT_HIP_CHECK(ctx, hipGetLastError());
  const long total = desc->n_mu * desc->nt;
  hipLaunchKernelGGL(traj_residual_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, p.pres,
                     p.pscale, res, scale, (long)desc->nt, (int)plan.slices, total);
  RT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_grid = plan.grid;
  ctx->last_splits = plan.slices;
  ctx->last_tile = TR_EV_ROWS * 1000 + TR_EV_STEPS;
  return RT_OK;
}
