// The rows of one BDF step of the closed-form 1-D P1 models, stated once: for the elimination and the defect pass of the
// full-order sweep (p1_fom.hip) and for the residuals of lifted reduced trajectories (traj_residual.hip).  The formulas
// are those of include/romtime_hip.h (rt_fom_desc); the functions compile under the translation unit's default
// floating-point contraction, the same in every file that includes them, so that a row has the same bits wherever it is
// formed.
#pragma once
#include "common.h"

namespace {

// The scalars of one step's rows, and the rows themselves.
struct FomStep {
  double dt, ws, c0, c1n, h, mo, md, ah, h6, dth, a0, a1, a2, a2h;
  bool two;
};

__device__ __forceinline__ FomStep fom_step(const double* tb, double dt, double inv_nx, double ws, bool two) {
  FomStep S;
  const double h = tb[0], alpha = tb[1], c1 = tb[3];
  const double bdf = two ? 1.5 : 1.0;
  S.dt = dt, S.ws = ws, S.two = two, S.h = h, S.c0 = tb[2], S.a0 = tb[4], S.a1 = tb[5], S.a2 = tb[6];
  S.mo = bdf * h / 6.0, S.md = bdf * 4.0 * h / 6.0, S.ah = alpha / h, S.h6 = h / 6.0, S.dth = dt * h;
  S.c1n = c1 * inv_nx, S.a2h = S.a2 * h * h / 6.0;
  return S;
}

// w and past of a node from its two older values
__device__ __forceinline__ double fom_w(const FomStep& S, double un, double vn, int node) {
  return S.ws * (S.two ? 2.0 * un - vn : un) + S.c0 + S.c1n * (double)node;
}

__device__ __forceinline__ double fom_past(const FomStep& S, double un, double vn) { return S.two ? 2.0 * un - 0.5 * vn : un; }

// row of node i from w and past of the nodes i-1, i, i+1; l_1 and u_nx-1 are NOT yet zeroed (dominance looks at them)
__device__ __forceinline__ void fom_row(const FomStep& S, double wL, double wC, double wR, double pL, double pC, double pR, int i,
                                        double& l, double& d, double& u, double& rhs) {
  constexpr double sixth = 1.0 / 6.0;
  const double bp = (wL + 2.0 * wC) * sixth, ai = (2.0 * wC + wR) * sixth;
  l = S.mo + S.dt * (-S.ah - bp);
  d = S.md + S.dt * (2.0 * S.ah + bp - ai);
  u = S.mo + S.dt * (-S.ah + ai);
  // h/3 (f(x - h/2) + f(x) + f(x + h/2)) = h (f(x) + a2 h^2 / 6) for the quadratic f
  const double x = (double)i * S.h;
  rhs = S.h6 * (pL + 4.0 * pC + pR) + S.dth * (fma(fma(S.a2, x, S.a1), x, S.a0) + S.a2h);
}

}  // namespace
