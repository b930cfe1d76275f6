// Restarted GMRES on B independent dense r x r systems, x0 = 0, no preconditioner: the reduced solve of the reference's
// online loop, scipy.sparse.linalg.gmres(K_N, b_N, atol=1e-10, tol=1e-10, maxiter=1e6) (rom.py:36,414-425,492), restated
// from the control flow of SciPy 1.15.3's gmres (sparse/linalg/_isolve/iterative.py), so that the stopping decisions and
// the returned iterate are SciPy's up to rounding:
//   bnrm2 = |b|, atol = max(atol, rtol bnrm2); bnrm2 == 0 -> x = b; |b| < atol -> x = 0;
//   ptol = bnrm2 min(1, atol / bnrm2); per cycle v_0 = res / |res|, S = [|res|, 0, ...], then for col < restart:
//     w = K v_col, h0 = |w|, modified Gram-Schmidt, h1 = |w|, breakdown if h1 <= eps h0, the earlier rotations, a new
//     one with LAPACK dlartg semantics, S[col+1] = -s S[col], S[col] = c S[col], presid = |S[col+1]|; the inner loop
//     ends on presid <= ptol or a breakdown;
//   back substitution in SciPy's form (zero entries of y skipped), x += y V, res = b - K x, the outer test and the
//   ptol_max_factor update of gh-8400;
//   info = 0 if |res| <= atol else maxiter; iters = inner iterations (the count of SciPy's "pr_norm" callback).
//
// Layout: ONE wave64 per system, so that every norm and dot product of the Arnoldi chain is a wave reduction
// (rtw::wave_sum, fixed order: a system's result does not depend on B or on its place in the batch) and no step waits
// for other waves.  Lane l holds entries l and l + 64 of every r-vector (NV = 1 for r <= 64, 2 beyond).  K sits in LDS
// with an odd leading dimension; the vector a mat-vec multiplies goes through a small LDS buffer.  The Krylov basis and
// the triangular factor R (the rotated Hessenberg columns) are stored lane-distributed, so that every lane reads back
// only what it wrote itself: in LDS behind K when they fit (restart 20: r <= 121), otherwise in a global work area
// (r near 128, or a restart near r).  The Hessenberg column being built, the rotations and S are lane-distributed
// registers whose entries come out wave-uniform through readlane.  Elementwise steps are evaluated as NumPy evaluates
// them (no contraction: #pragma below); the BLAS-like sums (mat-vec, dot products, y V) use fused multiply-adds.
#include "common.h"
#include "sweep_step.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace {

constexpr int GM_THREADS = 64;
constexpr double GM_EPS = 2.220446049250313e-16;   // np.finfo(np.float64).eps
constexpr size_t GM_LDS_MAX = 156 * 1024;          // dynamic LDS of one workgroup (the CU has 160 KB)

struct gm_params {
  double rtol, atol;
  int restart;     // min(restart, r)
  long maxiter;    // outer cycles
};

// entry i (wave-uniform, 0 <= i < 64 NV) of a lane-distributed vector, wave-uniform
template <int NV>
__device__ __forceinline__ double lget(const double (&a)[NV], int i) {
  if (NV == 1 || i < 64) return rtw::read_lane(a[0], i & 63);
  return rtw::read_lane(a[NV - 1], i & 63);
}
template <int NV>
__device__ __forceinline__ void lset(double (&a)[NV], int i, double v, int lane) {
#pragma unroll
  for (int q = 0; q < NV; ++q)
    if (lane + 64 * q == i) a[q] = v;
}
template <int NV>
__device__ __forceinline__ double wdot(const double (&a)[NV], const double (&b)[NV]) {
  double p = a[0] * b[0];
#pragma unroll
  for (int q = 1; q < NV; ++q) p = fma(a[q], b[q], p);
  return rtw::wave_sum(p);
}
template <int NV>
__device__ __forceinline__ double wnorm(const double (&a)[NV]) {
  return sqrt(wdot<NV>(a, a));
}

// LAPACK dlartg (3.10 and later): r takes the sign of f; f == 0 gives c = 0, s = sign(g); g == 0 gives c = 1, s = 0
__device__ __forceinline__ void lartg(double f, double g, double& c, double& s, double& r) {
  const double safmin = 0x1p-1022, safmax = 0x1p+1022;
  const double rtmin = 0x1p-511, rtmax = 0x1.6a09e667f3bcdp+510;   // sqrt(safmin), sqrt(safmax / 2)
  const double f1 = fabs(f), g1 = fabs(g);
  if (g == 0.0) {
    c = 1.0; s = 0.0; r = f;
  } else if (f == 0.0) {
    c = 0.0; s = copysign(1.0, g); r = g1;
  } else if (f1 > rtmin && f1 < rtmax && g1 > rtmin && g1 < rtmax) {
    const double d = sqrt(f * f + g * g);
    c = f1 / d;
    r = copysign(d, f);
    s = g / r;
  } else {
    const double u = fmin(safmax, fmax(safmin, fmax(f1, g1)));
    const double fs = f / u, gs = g / u;
    const double d = sqrt(fs * fs + gs * gs);
    c = fabs(fs) / d;
    r = copysign(d, f);
    s = gs / r;
    r = r * u;
  }
}

// out (lane-distributed) = K v for the LDS matrix sK (leading dimension lda) and the LDS vector sv; rows >= r give 0
template <int NV>
__device__ __forceinline__ void gm_matvec(const double* sK, int lda, const double* sv, int r, int lane, double (&out)[NV]) {
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int i = lane + 64 * q;
    const double* row = sK + (i < r ? i : r - 1) * lda;
    double acc = 0.0;
    int j = 0;
    for (; j + 4 <= r; j += 4) {
      const double k0 = row[j], k1 = row[j + 1], k2 = row[j + 2], k3 = row[j + 3];
      const double v0 = sv[j], v1 = sv[j + 1], v2 = sv[j + 2], v3 = sv[j + 3];
      acc = fma(k0, v0, acc);
      acc = fma(k1, v1, acc);
      acc = fma(k2, v2, acc);
      acc = fma(k3, v3, acc);
    }
    for (; j < r; ++j) acc = fma(row[j], sv[j], acc);
    out[q] = (i < r) ? acc : 0.0;
  }
}

// the lane-distributed vector a -> the LDS buffer sv (visible to the whole wave on return)
template <int NV>
__device__ __forceinline__ void gm_to_lds(double* sv, const double (&a)[NV], int r, int lane) {
  __syncthreads();   // every lane is done with the previous contents
#pragma unroll
  for (int q = 0; q < NV; ++q)
    if (lane + 64 * q < r) sv[lane + 64 * q] = a[q];
  __syncthreads();
}

// One workgroup (one wave) per system.  b from bsrc, or formed from the sweep's recipe (rq.MN != nullptr); x to xout.
// LDSB: Krylov basis and R in LDS behind K; otherwise in `work` ((2 restart + 1) 64 NV doubles per system).
template <int NV, bool LDSB>
__global__ __launch_bounds__(GM_THREADS) void gmres_kernel(const double* __restrict__ K, const double* __restrict__ bsrc,
                                                           double* __restrict__ xout, int r, const gm_params p,
                                                           int64_t* __restrict__ info, int* __restrict__ iters,
                                                           double* __restrict__ work, const rt_step_rhs rq,
                                                           long* __restrict__ counters, const rt_advance adv) {
  extern __shared__ __attribute__((aligned(16))) double gm_sm[];
  constexpr int ST = 64 * NV;   // stride of a lane-distributed vector in the basis / R storage
  const int lane = threadIdx.x, sys = blockIdx.x;
  const int lda = r | 1, m = p.restart;
  double* sv = gm_sm;          // 128: the operand of a mat-vec
  double* sK = gm_sm + 128;    // r x lda
  double* Vs = LDSB ? sK + (((size_t)r * lda + 1) & ~(size_t)1) : work + (size_t)sys * (2 * m + 1) * ST;
  double* Rs = Vs + (size_t)(m + 1) * ST;   // m columns of R
  const double* Kb = K + (size_t)sys * r * r;

  // K -> LDS, eight rows in flight per pass
  for (int i0 = 0; i0 < r; i0 += 8) {
    double kv[8][2];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int i = i0 + u, j = lane + 64 * c;
        kv[u][c] = (i < r && j < r) ? Kb[(size_t)i * r + j] : 0.0;
      }
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const int i = i0 + u, j = lane + 64 * c;
        if (i < r && j < r) sK[i * lda + j] = kv[u][c];
      }
  }

  // right-hand side
  double bv[NV];
  if (rq.MN) {   // the sweeps: b = M_N (c0 u^n + c1 u^{n-1}) + dt Zf^T F_rhs
    double su[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int i = lane + 64 * q;
      su[q] = (i < r) ? step_rhs_state(rq, sys, r, i) : 0.0;
    }
    gm_to_lds<NV>(sv, su, r, lane);
    const double* Mb = step_rhs_mn(rq, sys, r);
    const double* Ff = step_rhs_forcing_rows(rq, sys);
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int i = lane + 64 * q;
      bv[q] = (i < r) ? step_rhs_row(rq, Mb, Ff, r, i, sv) : 0.0;
    }
  } else {
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      const int i = lane + 64 * q;
      bv[q] = (i < r) ? bsrc[(size_t)sys * r + i] : 0.0;
    }
  }
  __syncthreads();   // K is in LDS

  double xv[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) xv[q] = 0.0;
  int n_inner = 0;
  long status = 0;
  const double bnrm2 = wnorm<NV>(bv);
  const double atol = fmax(p.atol, p.rtol * bnrm2);
  if (bnrm2 == 0.0) {
#pragma unroll
    for (int q = 0; q < NV; ++q) xv[q] = bv[q];   // SciPy returns b itself
  } else if (!(bnrm2 < atol)) {                    // else |b| < atol: x = 0 (the test before SciPy's first cycle)
    double ptol_max_factor = 1.0;
    double ptol = bnrm2 * fmin(ptol_max_factor, atol / bnrm2);
    double presid = 0.0, rnorm = bnrm2;
    double res[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) res[q] = bv[q];
    for (long iteration = 0; iteration < p.maxiter; ++iteration) {
      const double inv0 = 1.0 / rnorm;   // |res|: the sum that produced rnorm (bnrm2 in the first cycle)
      double v[NV], Sv[NV], gc[NV], gs[NV], hc[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        v[q] = res[q] * inv0;
        Sv[q] = 0.0;
        gc[q] = 0.0;
        gs[q] = 0.0;
        Vs[lane + 64 * q] = v[q];
      }
      double Scur = rnorm;   // S[col] at the start of column col (S[col+1] lives here, not in Sv)
      bool breakdown = false;
      int col = 0;
      for (col = 0; col < m; ++col) {
        gm_to_lds<NV>(sv, v, r, lane);
        double w[NV];
        gm_matvec<NV>(sK, lda, sv, r, lane, w);
        const double h0 = wnorm<NV>(w);
#pragma unroll
        for (int q = 0; q < NV; ++q) hc[q] = 0.0;
        for (int k = 0; k <= col; ++k) {   // modified Gram-Schmidt
          double vk[NV];
#pragma unroll
          for (int q = 0; q < NV; ++q) vk[q] = Vs[(size_t)k * ST + lane + 64 * q];
          const double hk = wdot<NV>(vk, w);
          lset<NV>(hc, k, hk, lane);
#pragma unroll
          for (int q = 0; q < NV; ++q) w[q] = w[q] - hk * vk[q];
        }
        double h1 = wnorm<NV>(w);
        if (h1 <= GM_EPS * h0) {   // exact solution indicator: w is kept unnormalised
          h1 = 0.0;
          breakdown = true;
#pragma unroll
          for (int q = 0; q < NV; ++q) v[q] = w[q];
        } else {
          const double inv = 1.0 / h1;
#pragma unroll
          for (int q = 0; q < NV; ++q) v[q] = w[q] * inv;
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) Vs[(size_t)(col + 1) * ST + lane + 64 * q] = v[q];
        // the earlier rotations on the new column; the running entry h[col][k] stays wave-uniform
        double hk = lget<NV>(hc, 0);
        for (int k = 0; k < col; ++k) {
          const double c = lget<NV>(gc, k), s = lget<NV>(gs, k);
          const double n0 = hk, n1 = lget<NV>(hc, k + 1);
          lset<NV>(hc, k, c * n0 + s * n1, lane);
          hk = -s * n0 + c * n1;
        }
        double c, s, mag;
        lartg(hk, h1, c, s, mag);
        lset<NV>(gc, col, c, lane);
        lset<NV>(gs, col, s, lane);
        lset<NV>(hc, col, mag, lane);
        const double tmp = -s * Scur;
        lset<NV>(Sv, col, c * Scur, lane);
        Scur = tmp;
        presid = fabs(tmp);
        ++n_inner;
#pragma unroll
        for (int q = 0; q < NV; ++q) Rs[(size_t)col * ST + lane + 64 * q] = hc[q];
        if (presid <= ptol || breakdown) break;
      }
      if (col == m) col = m - 1;   // the inner loop ran its course
      if (lget<NV>(hc, col) == 0.0) lset<NV>(Sv, col, 0.0, lane);
      // y = R^-1 S[:col+1] in SciPy's form; column k of R (entries 0 .. k) is Rs[k]
      double y[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) y[q] = (lane + 64 * q <= col) ? Sv[q] : 0.0;
      for (int k = col; k >= 0; --k) {
        double yk = lget<NV>(y, k);
        if (yk != 0.0) {
          double Rk[NV];
#pragma unroll
          for (int q = 0; q < NV; ++q) Rk[q] = Rs[(size_t)k * ST + lane + 64 * q];
          yk = yk / lget<NV>(Rk, k);
          lset<NV>(y, k, yk, lane);
#pragma unroll
          for (int q = 0; q < NV; ++q)
            if (lane + 64 * q < k) y[q] = y[q] - yk * Rk[q];
        }
      }
      // x += y @ V[:col+1]
      double acc[NV];
#pragma unroll
      for (int q = 0; q < NV; ++q) acc[q] = 0.0;
      for (int k = 0; k <= col; ++k) {
        const double yk = lget<NV>(y, k);
#pragma unroll
        for (int q = 0; q < NV; ++q) acc[q] = fma(yk, Vs[(size_t)k * ST + lane + 64 * q], acc[q]);
      }
#pragma unroll
      for (int q = 0; q < NV; ++q) xv[q] = xv[q] + acc[q];
      // res = b - K x
      gm_to_lds<NV>(sv, xv, r, lane);
      double kx[NV];
      gm_matvec<NV>(sK, lda, sv, r, lane, kx);
#pragma unroll
      for (int q = 0; q < NV; ++q) res[q] = bv[q] - kx[q];
      rnorm = wnorm<NV>(res);
      if (rnorm <= atol) break;
      if (breakdown) break;   // exact solution indicated but the outer test failed: SciPy gives up
      if (presid <= ptol)
        ptol_max_factor = fmax(GM_EPS, 0.25 * ptol_max_factor);
      else
        ptol_max_factor = fmin(1.0, 1.5 * ptol_max_factor);
      ptol = presid * fmin(ptol_max_factor, atol / rnorm);
    }
    status = (rnorm <= atol) ? 0 : p.maxiter;
  }

  double* xb = xout + (size_t)sys * r;
#pragma unroll
  for (int q = 0; q < NV; ++q)
    if (lane + 64 * q < r) xb[lane + 64 * q] = xv[q];
  if (lane == 0) {
    if (info) info[sys] = status;
    if (iters) iters[sys] = n_inner;
    if (counters) {   // the sweeps' statistics (rt_ctx_get_counter)
      atomicAdd(reinterpret_cast<unsigned long long*>(&counters[RT_CNT_GMRES_ITER]), (unsigned long long)n_inner);
      atomicAdd(reinterpret_cast<unsigned long long*>(&counters[RT_CNT_SOLVES]), 1ull);
      if (status != 0) atomicAdd(reinterpret_cast<unsigned long long*>(&counters[RT_CNT_GMRES_UNCONVERGED]), 1ull);
    }
  }
  if (adv.enabled) {   // the sweep's end of step for this system
    __syncthreads();   // x is complete and visible in this workgroup
    hsweep_advance_rows(adv, sys, r, xout, 1, sv, lane, GM_THREADS);
  }
}

size_t gm_lds_k(int64_t r) { return sizeof(double) * (128 + (((size_t)r * (size_t)(r | 1) + 1) & ~(size_t)1)); }
size_t gm_vec_bytes(int64_t r, int64_t m) { return sizeof(double) * (size_t)(2 * m + 1) * (r > 64 ? 128 : 64); }
int64_t gm_restart(int64_t r, const rt_gmres_opts* o) { return o->restart < r ? o->restart : r; }

}  // namespace

int rt_gmres_check_opts(rt_ctx* ctx, const rt_gmres_opts* o) {
  RT_ARG_CHECK(ctx, o != nullptr);
  RT_ARG_CHECK(ctx, o->rtol >= 0.0 && o->atol >= 0.0 && o->rtol <= 1e300 && o->atol <= 1e300);   // NaN fails too
  RT_ARG_CHECK(ctx, o->restart >= 1 && o->maxiter >= 1);
  return RT_OK;
}

size_t rt_gmres_work_bytes(int64_t r, int64_t B, const rt_gmres_opts* o) {
  const int64_t m = gm_restart(r, o);
  if (gm_lds_k(r) + gm_vec_bytes(r, m) <= GM_LDS_MAX) return 0;
  return (size_t)B * gm_vec_bytes(r, m);
}

int rt_gmres_launch(rt_ctx* ctx, const double* K, const double* b, double* x, int64_t r, int64_t B, const rt_gmres_opts* o,
                    int64_t* info, int* iters, double* work, const rt_step_rhs* recipe, const rt_advance* advance,
                    bool count) {
  RT_TRY(rt_gmres_check_opts(ctx, o));
  if (r > 128) {
    ctx->err = "rt_gmres_batched: r > 128 not supported (K must fit the CU's LDS)";
    return RT_ERR_UNSUPPORTED;
  }
  RT_ARG_CHECK(ctx, r >= 1 && B >= 1 && B <= 0x7fffffff);
  const int64_t m = gm_restart(r, o);
  const gm_params p{o->rtol, o->atol, (int)m, (long)o->maxiter};
  const bool in_lds = gm_lds_k(r) + gm_vec_bytes(r, m) <= GM_LDS_MAX;
  const size_t lds = gm_lds_k(r) + (in_lds ? gm_vec_bytes(r, m) : 0);
  if (!in_lds && !work) {
    void* w = nullptr;
    RT_TRY(rt_scratch(ctx, (size_t)B * gm_vec_bytes(r, m), &w));
    work = static_cast<double*>(w);
  }
  const rt_step_rhs rq = recipe ? *recipe : rt_step_rhs{};
  const rt_advance adv = advance ? *advance : rt_advance{};
  long* counters = count ? ctx->dev_counters : nullptr;
  double* wk = in_lds ? nullptr : work;
#define GM_LAUNCH(NV_, L_)                                                                                            \
  {                                                                                                                   \
    RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&gmres_kernel<NV_, L_>), (int)GM_LDS_MAX));                \
    hipLaunchKernelGGL((gmres_kernel<NV_, L_>), dim3((unsigned)B), dim3(GM_THREADS), lds, ctx->stream, K, b, x, (int)r, \
                       p, info, iters, wk, rq, counters, adv);                                                        \
  }
  if (r <= 64) {
    if (in_lds) GM_LAUNCH(1, true) else GM_LAUNCH(1, false)
  } else {
    if (in_lds) GM_LAUNCH(2, true) else GM_LAUNCH(2, false)
  }
#undef GM_LAUNCH
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

extern "C" int rt_gmres_batched(rt_ctx* ctx, const double* K, const double* b, double* x, int64_t r, int64_t B,
                                const rt_gmres_opts* opts, int64_t* info, int* iters) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, K && b && x);
  return rt_gmres_launch(ctx, K, b, x, r, B, opts, info, iters, nullptr, nullptr, nullptr, false);
}

extern "C" int rt_ctx_set_reduced_solver(rt_ctx* ctx, int kind, const rt_gmres_opts* opts) {
  if (!ctx) return RT_ERR_ARG;
  if (kind == RT_SOLVER_DIRECT) {
    ctx->reduced_solver = RT_SOLVER_DIRECT;
    return RT_OK;
  }
  if (kind != RT_SOLVER_GMRES) {
    ctx->err = "rt_ctx_set_reduced_solver: kind must be RT_SOLVER_DIRECT or RT_SOLVER_GMRES";
    return RT_ERR_ARG;
  }
  RT_TRY(rt_gmres_check_opts(ctx, opts));
  ctx->reduced_solver = RT_SOLVER_GMRES;
  ctx->gmres_opts = *opts;
  return RT_OK;
}
