// Full-order BDF sweeps of the closed-form 1-D P1 models (testing/mock.py: MockHeatEquation.solve, MockBurgers.solve;
// the reference's OneDimensionalSolver.solve, fom/base.py:693-831) for a batch of parameter points, the whole time loop in
// one launch.
//
// Every operator of the two problems has a closed form per row (p1_assembly.hip), and every convective operator is the
// trilinear form int w u' v of a nodal function  w_i = s u*_i + c0 + c1 i/nx  (s = 1: Burgers, the state convects; c0 = -1
// MockSolver's constant convection; c1 the ALE ramp of the moving heat problem or the lifting ramp of the piston).  A step is
// therefore ONE tridiagonal system per parameter point, interior rows i = 1 .. nx-1:
//
//   a_e = (2 w_e + w_e+1)/6,  b_e = (w_e + 2 w_e+1)/6                                   per cell e
//   l_i = bdf h/6 + dt(-alpha/h - b_i-1)
//   d_i = bdf 4h/6 + dt(2 alpha/h + b_i-1 - a_i)
//   u_i = bdf h/6 + dt(-alpha/h + a_i)
//   rhs_i = h/6 (past_i-1 + 4 past_i + past_i+1) + dt h/3 (f(x_i - h/2) + f(x_i) + f(x_i + h/2)),  f = a0 + a1 x + a2 x^2
//
// with bdf = 1.5, u* = 2u^n - u^n-1, past = 2u^n - u^n-1/2 from global step 1 on under BDF2, else 1, u^n, u^n.
//
// One workgroup of 1024 threads per parameter point; no workgroup ever waits for another, so there is no co-residency
// requirement, n_mu may exceed the CU count and a CU-masked stream gives the same bits.  The rows are never stored: each
// thread owns a partition of m = ceil((nx-1)/1024) consecutive rows and forms them on the fly (Wang's partition method,
// no pivoting - the rows are diagonally dominant, which info reports):
//
//   A  downward elimination inside the partition:   x_k + c_k x_k+1 + f_k xL = y_k      (xL: last unknown of partition p-1)
//      and, in the same pass, the partition's first unknown  x_0 = Y - G xB - F xL       (xB: its own last unknown)
//      as running sums with the products pi_k+1 = -c_k pi_k
//   B  the partitions' last unknowns satisfy a tridiagonal system of <= 1024 rows:
//        f_last xB_p-1 + (1 - c_last F_p+1) xB_p - c_last G_p+1 xB_p+1 = y_last - c_last Y_p+1
//      solved in LDS by parallel cyclic reduction, log2 steps, every thread one row
//   C  upwards, x_k = y_k - c_k x_k+1 - f_k xL from x_last = xB, written to the new state and, through an LDS tile, to U_out
//
// A step moves ten arrays of N_h words through its CU (two states in, three factors out and in again, the new state and
// U_out), and a workgroup has the vector memory path of one CU for it.
//
// The two states and the three factor arrays of a point live in the ctx's leaf arena as [row of partition][partition]:
// lane p reads and writes element p of a row, so every access of A and C is coalesced, and the neighbours across a
// partition edge are lane p-1's last and lane p+1's first row.  Only U_out and u_init have the natural layout: they pass
// through an LDS tile of 8 rows of every partition (64-byte runs in memory).
//
// The certified mode (rt_p1_fom_bdf_sweep_certified, the CERT instantiation) runs the same passes A, B and C - the same
// bits in U_out - and does not look at dominance.  Pass C writes the new state to a third state array (six arrays per
// point instead of five), so that u^n and u^n-1 are still there for
//
//   D  the rows once more (fom_row, the function pass A forms them with) against the new state: the componentwise
//      backward error  omega = max_i |rhs_i - (l_i x_i-1 + d_i x_i + u_i x_i+1)| / (|l_i x_i-1| + |d_i x_i| + |u_i x_i+1| + |rhs_i|)
//      of the step, reduced over the wave (wave_ops.h) and over the workgroup through LDS; a non-finite pivot, xB, state
//      value, residual or denominator makes it +inf (fmax drops NaNs: "non-finite seen" is a flag of its own).
//
// D reads three arrays more per step (thirteen instead of ten).
#include <cmath>

#include "common.h"
#include "p1_rows.h"
#include "wave_ops.h"

namespace {

constexpr int FOM_THREADS = 1024;            // partitions of a system at most: one per thread
constexpr int FOM_KT = 8;                    // rows of every partition in one LDS tile
constexpr int FOM_TILE_LD = FOM_KT + 1;
constexpr int FOM_KB = 8;                    // rows of pass A whose loads are issued together
constexpr long FOM_MAX_NX = 1L << 22;        // stated in the header
constexpr size_t FOM_MAX_SCRATCH = (size_t)1 << 36;
constexpr int FOM_LDS_BYTES = (FOM_THREADS * FOM_TILE_LD + FOM_THREADS) * 8;   // tile (the PCR rows alias it) + xB

struct FomParams {
  long nx, n_mu, nt, first_step, m, parts, ld_step, stride_mu;
  double dt;
  int bdf2, state_in_w;
  const double* tab;
  const double* u_init;
  double* U;
  int* info;
  double* arena;
  double defect_tol;   // certified mode only
  double* defect;
};

struct FomPlan {
  long m, parts;
  size_t scratch, per_point;
};

// The scalars of one step's rows and the rows themselves (FomStep, fom_step, fom_w, fom_past, fom_row) are stated once, in
// p1_rows.h, for pass A, for the defect pass D and for traj_residual.hip.

// rows k0 .. k0+KT-1 of every partition between the LDS tile and a state in its natural layout (node = 1 + p m + k)
__device__ __forceinline__ void fom_tile_to_global(const double* tile, double* dst, int k0, int m, int n) {
  for (int it = 0; it < FOM_KT; ++it) {
    const int idx = threadIdx.x + it * FOM_THREADS;
    const int q = idx / FOM_KT, kk = idx % FOM_KT;
    const int k = k0 + kk, row = q * m + k;
    if (k < m && row < n) dst[1 + row] = tile[q * FOM_TILE_LD + kk];
  }
}

__device__ __forceinline__ void fom_global_to_tile(double* tile, const double* src, int k0, int m, int n) {
  for (int it = 0; it < FOM_KT; ++it) {
    const int idx = threadIdx.x + it * FOM_THREADS;
    const int q = idx / FOM_KT, kk = idx % FOM_KT;
    const int k = k0 + kk, row = q * m + k;
    if (k < m && row < n) tile[q * FOM_TILE_LD + kk] = src[1 + row];
  }
}

// nx <= 2^22: node numbers and the offsets inside a point's arrays (m x 1024 <= 2^22 words) fit 32 bits
template <bool CERT>
__global__ __launch_bounds__(FOM_THREADS) void p1_fom_kernel(const FomParams P) {
  extern __shared__ double fom_lds[];
  double* tile = fom_lds;                               // FOM_THREADS x FOM_TILE_LD
  double* pcr = fom_lds;                                // 4 x FOM_THREADS, while no tile is in flight
  double* shb = fom_lds + FOM_THREADS * FOM_TILE_LD;    // FOM_THREADS: xB of every partition
  constexpr int NT = FOM_THREADS;
  const int p = threadIdx.x;
  const long j = blockIdx.x;
  const int m = (int)P.m, n = (int)P.nx - 1;
  const int r0 = p * m;
  const int mp = n - r0 > m ? m : (n - r0 < 0 ? 0 : n - r0);   // rows of this partition (only the last active one may be short)
  const bool active = mp > 0;
  const bool last_part = active && (r0 + mp == n);
  double* base = P.arena + (size_t)j * (CERT ? 6 : 5) * m * NT;
  double* S0 = base;                                    // u^n
  double* S1 = base + (size_t)m * NT;                   // u^{n-1}; the new state is written over it, or (CERT) to S2
  double* S2 = CERT ? base + (size_t)5 * m * NT : nullptr;
  double* const fc = base + (size_t)2 * m * NT;
  double* const ff = base + (size_t)3 * m * NT;
  double* const fy = base + (size_t)4 * m * NT;

  if (P.u_init) {
    for (int which = 0; which < 2; ++which) {
      const double* src = P.u_init + ((size_t)j * 2 + which) * (P.nx + 1);
      double* S = which ? S1 : S0;
      for (int k0 = 0; k0 < m; k0 += FOM_KT) {
        fom_global_to_tile(tile, src, k0, m, n);
        __syncthreads();
        for (int kk = 0; kk < FOM_KT; ++kk)
          if (k0 + kk < mp) S[(k0 + kk) * NT + p] = tile[p * FOM_TILE_LD + kk];
        __syncthreads();
      }
    }
  } else {
    for (int k = 0; k < mp; ++k) S0[k * NT + p] = S1[k * NT + p] = 0.0;
    __syncthreads();
  }

  const double dt = P.dt, inv_nx = 1.0 / (double)P.nx;
  const double ws = P.state_in_w ? 1.0 : 0.0;
  int info = 0;
  for (long s = 0; s < P.nt; ++s) {
    const long g = P.first_step + s;
    const bool two = P.bdf2 && g > 0;
    const double* tb = P.tab + ((size_t)s * P.n_mu + j) * 7;
    const FomStep T = fom_step(tb, dt, inv_nx, ws, two);
    double* const Sn = CERT ? S2 : S1;     // the new state
    bool bad = false;                      // a row not dominant or a pivot not finite; CERT: a pivot or xB not finite
    double cl = 0.0, fl = 0.0, yl = 0.0;   // the partition's last row after A
    double Y = 0.0, G = 0.0, F = 0.0;      // its first unknown in terms of xB and xL

    if (active) {
      // ---- A: rows formed from a sliding window of three nodes and eliminated downwards.  The first unknown follows
      // from the same pass: x_0 = sum_k pi_k (y_k - f_k xL) + pi_last xB with pi_0 = 1, pi_k+1 = -c_k pi_k.
      double unL = 0.0, vnL = 0.0;
      if (p > 0) {
        unL = S0[(m - 1) * NT + p - 1];
        if (two) vnL = S1[(m - 1) * NT + p - 1];
      }
      const double unC = S0[p], vnC = two ? S1[p] : 0.0;
      double wL = fom_w(T, unL, vnL, r0), wC = fom_w(T, unC, vnC, r0 + 1);
      double pL = fom_past(T, unL, vnL), pC = fom_past(T, unC, vnC);
      double cprev = 0.0, fprev = -1.0, yprev = 0.0, pi = 1.0;
      for (int kb = 0; kb < mp; kb += FOM_KB) {
        // the right-hand neighbours of FOM_KB rows are asked for together: the elimination below is one dependent chain,
        // and a load per row inside it would put a trip to the L2 on that chain
        double ur[FOM_KB], vr[FOM_KB];
#pragma unroll
        for (int q = 0; q < FOM_KB; ++q) {
          const int k = kb + q;
          ur[q] = vr[q] = 0.0;
          if (k + 1 < mp) {
            ur[q] = S0[(k + 1) * NT + p];
            if (two) vr[q] = S1[(k + 1) * NT + p];
          } else if (k + 1 == mp && !last_part) {
            ur[q] = S0[p + 1];
            if (two) vr[q] = S1[p + 1];
          }
        }
#pragma unroll
        for (int q = 0; q < FOM_KB; ++q) {
          const int k = kb + q;
          if (k >= mp) break;
          const int i = r0 + k + 1;         // node of this row
          const double unR = ur[q], vnR = vr[q];
          const double wR = fom_w(T, unR, vnR, i + 1), pR = fom_past(T, unR, vnR);
          double l, d, u, rhs;
          fom_row(T, wL, wC, wR, pL, pC, pR, i, l, d, u, rhs);
          if constexpr (!CERT) bad |= fabs(d) < fabs(l) + fabs(u);
          if (i == 1) l = 0.0;              // u_0 = u_nx = 0
          if (i == n) u = 0.0;
          const double r = 1.0 / (d - l * cprev);
          bad |= !std::isfinite(r);
          const double c = u * r, f = -l * fprev * r, y = (rhs - l * yprev) * r;
          fc[k * NT + p] = c;
          ff[k * NT + p] = f;
          fy[k * NT + p] = y;
          if (k + 1 < mp) {
            Y += pi * y;
            F += pi * f;
            pi = -c * pi;
          }
          cprev = c, fprev = f, yprev = y;
          wL = wC, wC = wR, pL = pC, pC = pR;
        }
      }
      cl = cprev, fl = fprev, yl = yprev;
      G = -pi;
    }

    // ---- B: the system of the partitions' last unknowns
    pcr[p] = Y;
    pcr[NT + p] = G;
    pcr[2 * NT + p] = F;
    __syncthreads();
    const bool nb = p + 1 < FOM_THREADS;
    const double Yn = nb ? pcr[p + 1] : 0.0, Gn = nb ? pcr[NT + p + 1] : 0.0, Fn = nb ? pcr[2 * NT + p + 1] : 0.0;
    __syncthreads();
    double A = active ? fl : 0.0, B = active ? 1.0 - cl * Fn : 1.0, C = active ? -cl * Gn : 0.0, D = active ? yl - cl * Yn : 0.0;
    for (int st = 1; st < P.parts; st <<= 1) {
      pcr[p] = A;
      pcr[NT + p] = B;
      pcr[2 * NT + p] = C;
      pcr[3 * NT + p] = D;
      __syncthreads();
      const int im = p - st, ip = p + st;
      const bool hm = im >= 0, hp = ip < FOM_THREADS;
      const double Am = hm ? pcr[im] : 0.0, Bm = hm ? pcr[NT + im] : 1.0, Cm = hm ? pcr[2 * NT + im] : 0.0, Dm = hm ? pcr[3 * NT + im] : 0.0;
      const double Ap = hp ? pcr[ip] : 0.0, Bp = hp ? pcr[NT + ip] : 1.0, Cp = hp ? pcr[2 * NT + ip] : 0.0, Dp = hp ? pcr[3 * NT + ip] : 0.0;
      const double k1 = A / Bm, k2 = C / Bp;
      const double nA = -Am * k1, nC = -Cp * k2, nB = B - Cm * k1 - Ap * k2, nD = D - Dm * k1 - Dp * k2;
      __syncthreads();
      A = nA, B = nB, C = nC, D = nD;
    }
    const double xB = D / B;
    bad |= active && !std::isfinite(1.0 / B);
    if constexpr (CERT) bad |= active && !std::isfinite(xB);
    shb[p] = xB;
    const bool any_bad = __syncthreads_or(bad);
    if (!CERT && any_bad && info == 0) info = (int)(1 + g);

    // ---- C: upwards inside the partition, x_k = y_k - c_k x_k+1 - f_k xL from x_last = xB, tile by tile
    const double xL = p > 0 ? shb[p - 1] : 0.0;
    double* out = P.U + (size_t)j * P.stride_mu + (size_t)s * P.ld_step;
    double xnext = xB;
    for (int k0 = (m - 1) / FOM_KT * FOM_KT; k0 >= 0; k0 -= FOM_KT) {
      double cq[FOM_KT], fq[FOM_KT], yq[FOM_KT];
#pragma unroll
      for (int kk = 0; kk < FOM_KT; ++kk) {
        const int k = k0 + kk;
        cq[kk] = fq[kk] = yq[kk] = 0.0;
        if (k + 1 < mp) {
          cq[kk] = fc[k * NT + p];
          fq[kk] = ff[k * NT + p];
          yq[kk] = fy[k * NT + p];
        }
      }
#pragma unroll
      for (int kk = FOM_KT - 1; kk >= 0; --kk) {
        const int k = k0 + kk;
        if (k < mp) {
          const double x = k + 1 == mp ? xB : yq[kk] - cq[kk] * xnext - fq[kk] * xL;
          xnext = x;
          Sn[k * NT + p] = x;
          tile[p * FOM_TILE_LD + kk] = x;
        }
      }
      __syncthreads();
      fom_tile_to_global(tile, out, k0, m, n);
      __syncthreads();
    }
    if (p == 0) {
      out[0] = 0.0;
      out[P.nx] = 0.0;
    }

    if constexpr (CERT) {
      // ---- D: the rows again, from the same two older states, against the new state (every lane's rows of Sn are
      // visible: the tiles of pass C end with a barrier).  xB (shb) is no longer read: the wave maxima go there.
      double om = 0.0;
      bool nf = false;
      if (active) {
        double unL = 0.0, vnL = 0.0, xl = 0.0;
        if (p > 0) {
          unL = S0[(m - 1) * NT + p - 1];
          if (two) vnL = S1[(m - 1) * NT + p - 1];
          xl = Sn[(m - 1) * NT + p - 1];
        }
        const double unC = S0[p], vnC = two ? S1[p] : 0.0;
        double xc = Sn[p];
        double wL = fom_w(T, unL, vnL, r0), wC = fom_w(T, unC, vnC, r0 + 1);
        double pL = fom_past(T, unL, vnL), pC = fom_past(T, unC, vnC);
        for (int kb = 0; kb < mp; kb += FOM_KB) {
          double ur[FOM_KB], vr[FOM_KB], xr[FOM_KB];
#pragma unroll
          for (int q = 0; q < FOM_KB; ++q) {
            const int k = kb + q;
            ur[q] = vr[q] = xr[q] = 0.0;
            if (k + 1 < mp) {
              ur[q] = S0[(k + 1) * NT + p];
              if (two) vr[q] = S1[(k + 1) * NT + p];
              xr[q] = Sn[(k + 1) * NT + p];
            } else if (k + 1 == mp && !last_part) {
              ur[q] = S0[p + 1];
              if (two) vr[q] = S1[p + 1];
              xr[q] = Sn[p + 1];
            }
          }
#pragma unroll
          for (int q = 0; q < FOM_KB; ++q) {
            const int k = kb + q;
            if (k >= mp) break;
            const int i = r0 + k + 1;
            const double unR = ur[q], vnR = vr[q], xR = xr[q];
            const double wR = fom_w(T, unR, vnR, i + 1), pR = fom_past(T, unR, vnR);
            double l, d, u, rhs;
            fom_row(T, wL, wC, wR, pL, pC, pR, i, l, d, u, rhs);
            if (i == 1) l = 0.0;
            if (i == n) u = 0.0;
            const double res = fma(-u, xR, fma(-d, xc, fma(-l, xl, rhs)));
            const double den = fabs(l * xl) + fabs(d * xc) + fabs(u * xR) + fabs(rhs);
            nf |= !std::isfinite(xc) || !std::isfinite(res) || !std::isfinite(den);
            // den == 0 (finite): every term is zero and so is the residual
            om = fmax(om, den > 0.0 ? fabs(res) / den : 0.0);
            wL = wC, wC = wR, pL = pC, pC = pR, xl = xc, xc = xR;
          }
        }
      }
      om = rtw::wave_max(om);
      if ((p & 63) == 0) shb[p >> 6] = om;
      const bool any_nf = __syncthreads_or(nf) || any_bad;
      double omega = shb[0];
      for (int q = 1; q < FOM_THREADS / 64; ++q) omega = fmax(omega, shb[q]);
      if (any_nf) omega = INFINITY;
      if (p == 0) P.defect[(size_t)j * P.nt + s] = omega;
      if (omega > P.defect_tol && info == 0) info = (int)(1 + g);   // +inf is above every tolerance
      double* t = S0;
      S0 = S2;
      S2 = S1;
      S1 = t;
    } else {
      double* t = S0;
      S0 = S1;
      S1 = t;
    }
  }
  if (p == 0) P.info[j] = info;
}

// Argument checks and the partitioning: host logic only, shared by the entry point and the plan query.
int fom_plan(const rt_fom_desc* d, const double* U_out, int64_t ld_step, int64_t stride_mu, const int* info, bool certified,
             FomPlan* plan, const char** why) {
#define FOM_ARG(cond)                      \
  do {                                     \
    if (!(cond)) {                         \
      *why = "bad argument: " #cond;       \
      return RT_ERR_ARG;                   \
    }                                      \
  } while (0)
  FOM_ARG(d && U_out && info);
  FOM_ARG(d->tab);
  FOM_ARG(d->nx >= 2 && d->n_mu >= 1 && d->nt >= 1 && d->first_step >= 0);
  FOM_ARG(d->u_init || d->first_step == 0);
  FOM_ARG(d->n_mu < (1L << 31) && d->nt < (1L << 40) && d->first_step < (1L << 30));
  if (d->nx > FOM_MAX_NX) {
    *why = "rt_p1_fom_bdf_sweep: nx > 2^22";
    return RT_ERR_UNSUPPORTED;
  }
  const int64_t Nh = d->nx + 1;
  FOM_ARG(ld_step >= Nh);
  FOM_ARG(ld_step < (1L << 40) && stride_mu < (1L << 60) / d->n_mu);
  FOM_ARG(d->n_mu == 1 || stride_mu >= (d->nt - 1) * ld_step + Nh);   // trajectories do not overlap
#undef FOM_ARG
  const long n = d->nx - 1;
  const long m = (n + FOM_THREADS - 1) / FOM_THREADS;
  const long parts = (n + m - 1) / m;
  const size_t per_point = (size_t)(certified ? 6 : 5) * m * FOM_THREADS * 8;   // the certified mode keeps a third state
  const size_t scratch = (size_t)d->n_mu * per_point;
  if (scratch > FOM_MAX_SCRATCH) {
    *why = certified ? "rt_p1_fom_bdf_sweep_certified: more than 64 GiB of states and factors (48 KiB x ceil((nx-1)/1024) per point): sweep fewer points per call"
                     : "rt_p1_fom_bdf_sweep: more than 64 GiB of states and factors (40 KiB x ceil((nx-1)/1024) per point): sweep fewer points per call";
    return RT_ERR_UNSUPPORTED;
  }
  *plan = FomPlan{m, parts, scratch, per_point};
  return RT_OK;
}

int fom_plan_info(int num_cus, const rt_fom_desc* desc, int64_t ld_step, int64_t stride_mu, bool certified, int64_t* out) {
  if (num_cus <= 0) return RT_ERR_ARG;
  FomPlan plan;
  const char* why = nullptr;
  static const double some_out = 0.0;   // the plan query has no output buffers: the checks only see that they are not null
  static const int some_info = 0;
  RT_TRY(fom_plan(desc, &some_out, ld_step, stride_mu, &some_info, certified, &plan, &why));
  if (out) {
    out[0] = desc->n_mu;
    out[1] = plan.parts;
    out[2] = plan.m;
    if (certified) out[3] = (int64_t)plan.per_point;
  }
  return RT_OK;
}

template <bool CERT>
int fom_launch(rt_ctx* ctx, const rt_fom_desc* desc, double* U_out, int64_t ld_step, int64_t stride_mu, double defect_tol,
               double* defect, int* info) {
  if (!ctx) return RT_ERR_ARG;
  FomPlan plan;
  const char* why = nullptr;
  const int rc = fom_plan(desc, U_out, ld_step, stride_mu, info, CERT, &plan, &why);
  if (rc != RT_OK) {
    ctx->err = why;
    return rc;
  }
  if (CERT && (!defect || !(defect_tol >= 0.0))) {   // a NaN tolerance fails the comparison too
    ctx->err = "bad argument: defect && defect_tol >= 0";
    return RT_ERR_ARG;
  }
  void* scratch = nullptr;
  RT_TRY(rt_scratch(ctx, plan.scratch, &scratch));
  FomParams p;
  p.nx = desc->nx;
  p.n_mu = desc->n_mu;
  p.nt = desc->nt;
  p.first_step = desc->first_step;
  p.m = plan.m;
  p.parts = plan.parts;
  p.ld_step = ld_step;
  p.stride_mu = stride_mu;
  p.dt = desc->dt;
  p.bdf2 = desc->bdf2 != 0;
  p.state_in_w = desc->state_in_w != 0;
  p.tab = desc->tab;
  p.u_init = desc->u_init;
  p.U = U_out;
  p.info = info;
  p.arena = static_cast<double*>(scratch);
  p.defect_tol = defect_tol;
  p.defect = defect;
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&p1_fom_kernel<CERT>), FOM_LDS_BYTES));
  hipLaunchKernelGGL(p1_fom_kernel<CERT>, dim3((unsigned)desc->n_mu), dim3(FOM_THREADS), FOM_LDS_BYTES, ctx->stream, p);
  RT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_grid = desc->n_mu;
  ctx->last_splits = plan.parts;
  ctx->last_tile = plan.m;
  return RT_OK;
}

}  // namespace

int rt_p1_fom_bdf_sweep_plan_info(int num_cus, const rt_fom_desc* desc, int64_t ld_step, int64_t stride_mu, int64_t* info3) {
  return fom_plan_info(num_cus, desc, ld_step, stride_mu, false, info3);
}

int rt_p1_fom_bdf_sweep_certified_plan_info(int num_cus, const rt_fom_desc* desc, int64_t ld_step, int64_t stride_mu,
                                            int64_t* info4) {
  return fom_plan_info(num_cus, desc, ld_step, stride_mu, true, info4);
}

int rt_p1_fom_bdf_sweep(rt_ctx* ctx, const rt_fom_desc* desc, double* U_out, int64_t ld_step, int64_t stride_mu, int* info) {
  return fom_launch<false>(ctx, desc, U_out, ld_step, stride_mu, 0.0, nullptr, info);
}

int rt_p1_fom_bdf_sweep_certified(rt_ctx* ctx, const rt_fom_desc* desc, double* U_out, int64_t ld_step, int64_t stride_mu,
                                  double defect_tol, double* defect, int* info) {
  return fom_launch<true>(ctx, desc, U_out, ld_step, stride_mu, defect_tol, defect, info);
}
