// One step of an online sweep, described by value for the kernels that run it: how the right-hand side is formed
// (rt_step_rhs) and how the step is closed once the systems are solved (rt_advance: state, previous state,
// trajectory row, the coefficient rows of the next step, the state transposed for the direct sweep's lift).
// The recipe's evaluation lives here too (step_rhs_*), for the three kernels that form a right-hand side:
// newton_solve_kernel (solve.hip), gmres_kernel (gmres.hip), step_rhs_kernel (sweep.hip).  hsweep_advance_rows closes
// the step for ONE parameter point.  It runs as the tail of newton_solve_kernel and of gmres_kernel, so that a step is
// expansion + solve instead of four launches (the host of the pool's boxes sustains only about one launch per 20 us),
// and in the stand-alone hsweep_advance_kernel (sweep.hip) before the first step and after the plain LU of r > 80.
#pragma once

// b = M_N (c0 u^n + c1 u^{n-1}) + dt Zf^T F_rhs, per system; MN == nullptr: rhs is given
struct rt_step_rhs {
  const double* MN;    // B x r x r
  const double* un;    // B x r
  const double* unm1;  // B x r
  double c0, c1, dt;
  const double* Ff;    // B x mf
  const double* Zf;    // mf x r
  int mf;
  long mn_stride = -1;        // doubles between the M_N of consecutive systems (-1: r * r; 0: one M_N for all)
  const long* ctr = nullptr;  // device step counter: Ff is the table base and the step's rows start at *ctr * ff_stride
  long ff_stride = 0;         // (graph replay of a sweep: the launch parameters cannot carry the step)
};

// The pieces of the recipe for system b and entry i: M_N of the system, its forcing rows of this step (nullptr without
// forcing terms), the state mix, the forcing sum.  Every sum is a chain of fma in index order.
__device__ __forceinline__ const double* step_rhs_mn(const rt_step_rhs& q, long b, int r) {
  return q.MN + b * (q.mn_stride < 0 ? (long)r * r : q.mn_stride);
}
__device__ __forceinline__ const double* step_rhs_forcing_rows(const rt_step_rhs& q, long b) {
  return q.mf ? (q.ctr ? q.Ff + *q.ctr * q.ff_stride : q.Ff) + b * q.mf : nullptr;
}
// The fma is spelled out so that the result does not depend on the contraction mode of the file that includes this
// header (gmres.hip turns contraction off).  The sweeps pass (c0, c1) = (2, -0.5) or (1, 0): both products are exact,
// so one rounding either way, and the same bits as a separate multiply and add.
__device__ __forceinline__ double step_rhs_state(const rt_step_rhs& q, long b, int r, int i) {
  return fma(q.c0, q.un[b * r + i], q.c1 * q.unm1[b * r + i]);
}
__device__ __forceinline__ double step_rhs_forcing(const rt_step_rhs& q, const double* Ff, int r, int i) {
  double f = 0.0;
  for (int e = 0; e < q.mf; ++e) f = fma(Ff[e], q.Zf[(long)e * r + i], f);
  return f;
}
// Row i of b with the system's M_N (Mb) read from global memory and the state mix s (r values) from LDS, one thread per
// row.  Mb and Ff are the two bases above, which a caller with several rows per thread takes once.
__device__ __forceinline__ double step_rhs_row(const rt_step_rhs& q, const double* Mb, const double* Ff, int r, int i,
                                               const double* s) {
  const double* Mrow = Mb + (long)i * r;
  double acc = 0.0;
  for (int j = 0; j < r; ++j) acc = fma(Mrow[j], s[j], acc);
  return fma(q.dt, step_rhs_forcing(q, Ff, r, i), acc);
}

struct rt_advance {
  double* un;            // B x r   u^n            (updated)
  double* unm1;          // B x r   u^{n-1}        (updated when keep_prev)
  double* out;           // B x nt x r trajectory
  long step_done, nt;    // the step being closed; with ctr: taken from the device counter
  int keep_prev, do_coef;
  const double* Fm;      // tables of the NEXT step (or their bases, with ctr)
  const double* Fl;
  const double* W;
  const double* Cn;
  const double* Sn;
  int extrapolate, mm, ml, mn;
  double bdf, dt;
  double* G;             // 2 B x (mm + ml + mn) coefficient rows of the next step
  const long* ctr;       // graph replay: device step counter (or nullptr)
  int B;
  double* xT;            // r x B: the new u^n transposed as well (direct sweep: operand of the lift), or nullptr
  int enabled;           // 0: the solver kernels leave the step alone
};

// x: the step's solution for parameter point b (r values, global memory; visible to every thread of the workgroup);
// su: r doubles of LDS; t / nthreads: this thread and the workgroup's size.  Ends without a barrier.
__device__ __forceinline__ void hsweep_advance_rows(rt_advance a, int b, int r, const double* x, int do_store,
                                                    double* su, int t, int nthreads) {
  const int M = a.mm + a.ml + a.mn;
  if (a.ctr) {
    // graph replay: the step comes from the device counter; Fm / Fl / Cn / Sn are the table bases, bdf is that of
    // every step after the first
    a.step_done = *a.ctr;
    const long next = a.step_done + 1;
    a.do_coef = next < a.nt;
    const long s2 = a.do_coef ? next : 0;
    a.Fm += s2 * a.B * a.mm;
    if (a.Fl) a.Fl += s2 * a.B * a.ml;
    if (a.Cn) a.Cn += s2 * a.B * a.mn;
    if (a.Sn) a.Sn += s2 * a.B;
  }
  for (int j = t; j < r; j += nthreads) {
    double u = a.un[(long)b * r + j], up = a.unm1[(long)b * r + j];
    if (do_store) {
      const double v = x[(long)b * r + j];
      if (a.keep_prev) {
        a.unm1[(long)b * r + j] = u;
        up = u;
      }
      a.un[(long)b * r + j] = v;
      if (a.xT) a.xT[(long)j * a.B + b] = v;
      a.out[((long)b * a.nt + a.step_done) * r + j] = v;
      u = v;
    }
    su[j] = a.extrapolate ? 2.0 * u - up : u;
  }
  if (!a.do_coef) return;
  __syncthreads();
  const double sc = a.Sn ? a.Sn[b] : 1.0;
  for (int e = t; e < M; e += nthreads) {
    double g;
    if (e < a.mm) {
      g = a.bdf * a.Fm[(long)b * a.mm + e];
    } else if (e < a.mm + a.ml) {
      g = a.dt * a.Fl[(long)b * a.ml + (e - a.mm)];
    } else {
      const int q = e - a.mm - a.ml;
      double acc = a.Cn ? a.Cn[(long)b * a.mn + q] : 0.0;
      const double* w = a.W + (long)q * r;
      for (int j = 0; j < r; ++j) acc = fma(w[j], su[j], acc);
      g = a.dt * sc * acc;
    }
    a.G[(long)b * M + e] = g;
    a.G[(long)(a.B + b) * M + e] = (e < a.mm) ? a.Fm[(long)b * a.mm + e] : 0.0;
  }
}
