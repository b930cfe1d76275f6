// The value of one entry of a closed-form 1-D P1 operator: the formulas stated at the top of p1_assembly.hip, in ONE place.
// rt_p1_local_assembly (p1_assembly.hip: one nodal function per output column) and rt_p1_snapshot_sets (p1_snapshots.hip:
// parameter rows x shared nodal functions) both call p1_entry_value, so for the same kind, entry, h, coef and nodal
// function the two return the same bits: the same expressions in the same order, nothing restated.
#pragma once
#include "common.h"

// The nodal function of the kinds that integrate one (w of the trilinear form, f of the loads), for ONE column.
struct P1Nodal {
  int mode;         // 0 none, 1 nodal values, 2 ramp  amp * node / nx, 3 polynomial  a0 + a1 x + a2 x^2  (load_p2 only)
  long nx;
  const double* v;  // mode 1: nx + 1 values (2 nx + 1 for load_p2); mode 2: the amplitude; mode 3: the three coefficients
};

__device__ __forceinline__ double p1_nodal(const P1Nodal& f, long k) {
  if (f.mode == 1) return f.v[k];
  return f.v[0] * ((double)k / (double)f.nx);
}

// load_p2: value k of the P2 function (k = 2 * vertex, odd k = cell midpoints; x = k h / 2)
__device__ __forceinline__ double p1_nodal_p2(const P1Nodal& f, long k, double h) {
  if (f.mode == 1) return f.v[k];
  const double x = 0.5 * h * (double)k;
  const double* a = f.v;
  return fma(fma(a[2], x, a[1]), x, a[0]);
}

// Entry (i, j) of the (nx + 1) x (nx + 1) operator `kind` (j = i for the load kinds) for cell size h and factor c.
__device__ __forceinline__ double p1_entry_value(int kind, long nx, long i, long j, double h, double c, const P1Nodal& f) {
  const bool dirichlet = (i == 0) || (i == nx);
  const long d = j - i;
  double v = 0.0;
  if (kind == RT_P1_LOAD) {
    if (!dirichlet) v = c * h / 6.0 * (p1_nodal(f, i - 1) + 4.0 * p1_nodal(f, i) + p1_nodal(f, i + 1));
  } else if (kind == RT_P1_LOAD_P2) {
    if (!dirichlet) v = c * h / 3.0 * (p1_nodal_p2(f, 2 * i - 1, h) + p1_nodal_p2(f, 2 * i, h) + p1_nodal_p2(f, 2 * i + 1, h));
  } else if (dirichlet) {
    v = (d == 0) ? 1.0 : 0.0;
  } else if (d >= -1 && d <= 1) {
    switch (kind) {
      case RT_P1_MASS: v = c * h * (d == 0 ? 4.0 / 6.0 : 1.0 / 6.0); break;
      case RT_P1_STIFFNESS: v = c / h * (d == 0 ? 2.0 : -1.0); break;
      case RT_P1_CONVECTION: v = c * (d == 0 ? 0.0 : (d == 1 ? -0.5 : 0.5)); break;
      default: {  // RT_P1_TRILINEAR
        const double wm = p1_nodal(f, i - 1), w0 = p1_nodal(f, i), wp = p1_nodal(f, i + 1);
        const double b_prev = (wm + 2.0 * w0) / 6.0, a_here = (2.0 * w0 + wp) / 6.0;
        v = c * (d == -1 ? -b_prev : (d == 0 ? b_prev - a_here : a_here));
      }
    }
  }
  return v;
}

// Values per column of a nodal function handed over in `mode` for `kind`.
__host__ __device__ inline long p1_nodal_width(int kind, int mode, long nx) {
  return mode == 1 ? (kind == RT_P1_LOAD_P2 ? 2 * nx + 1 : nx + 1) : (mode == 3 ? 3 : 1);
}
