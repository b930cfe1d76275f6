// Snapshot sets of the closed-form 1-D P1 operators over a product grid (the first half of run_offline_hyperreduction,
// rom/hrom.py:419-448, 1092-1146: what the six (M)DEIM objects are trained on).
//
// The offline walks assemble one whole operator per sample: per (mu, t) for DEIM / MDEIM (deim/deim.py:384-389), per
// (mu, t, psi) for N-MDEIM (deim/nonlinear.py:437-443).  rt_p1_local_assembly takes one nodal function per output
// column, which fits the online tables (few entries, many states) but not the N-MDEIM sets: those are a product grid,
// the (t) scalars times the (psi) functions, and serving them would mean copying the N_psi x N_h block of states once
// per instant.  Here a column is the pair (p, f) of a parameter row p - h[p], coef[p], and for the kinds whose nodal
// function is a ramp or a polynomial its amplitude / coefficients - and a nodal function f shared by every parameter
// row, and the whole  (n_par n_fun) x m  table is one launch:
//
//   out[(p n_fun + f) m + e] = beta out_old + (zero_first && e == 0 ? 0 : v(kind; rows[e], cols[e]; h[p], coef[p]; function))
//
// with v from p1_entry.h, the function rt_p1_local_assembly calls.  Column (p, f) is contiguous: the table is the
// RT_COL_MAJOR m x S snapshot set that rt_gram and rt_pod_orth take as it stands.
//
// Work: one flat index over (column, entry), entry fastest, walked with a grid stride.  Consecutive lanes hold
// consecutive entries of a column - and run on into the next column - so every wave stores 512 contiguous bytes
// whatever m is (a set of 2 x 10^5 columns of 3 entries fills its waves like one of 3 columns of 2 x 10^5).  rows / cols
// are read along the lanes, h / coef / par are one address per column, and the three nodal values of an entry sit next
// to those of the lanes beside it (the topology is sorted by row).  Vector stores only, no atomics: every word of
// `out` has one writer.
#include "common.h"
#include "p1_entry.h"

namespace {

constexpr int SS_THREADS = 256;
constexpr long SS_WG_PER_CU = 32;           // grid cap: enough waves to hide the gathers, the rest is the stride loop
constexpr long SS_MAX_NX = 1L << 22;        // the family's limit (p1_fom.hip)
constexpr long SS_MAX_COUNT = 1L << 62;

struct SsParams {
  int kind, par_mode, zero_first, read_old;
  long nx, m, n_fun, fun_width, total;     // total = n_par n_fun m
  const long* rows;
  const long* cols;        // nullptr for the load kinds
  const double* h;         // n_par
  const double* coef;      // n_par or nullptr (= 1)
  const double* par;       // par_mode 2: n_par amplitudes; 3: n_par x 3 coefficients; 0: nullptr
  const double* fun;       // n_fun x fun_width nodal values, or nullptr
  double beta;
  double* out;
};

// (column, entry) of flat index t; 32-bit division where the whole table has fewer than 2^32 words
template <class U>
__device__ __forceinline__ void ss_split(U t, U m, U n_fun, long& p, long& f, long& e) {
  const U col = t / m;
  e = (long)(t - col * m);
  const U pp = col / n_fun;
  p = (long)pp;
  f = (long)(col - pp * n_fun);
}

template <class U>
__global__ void __launch_bounds__(SS_THREADS) p1_snapshot_sets_kernel(const SsParams q) {
  const long stride = (long)gridDim.x * SS_THREADS;
  for (long t = (long)blockIdx.x * SS_THREADS + threadIdx.x; t < q.total; t += stride) {
    long p, f, e;
    ss_split<U>((U)t, (U)q.m, (U)q.n_fun, p, f, e);
    const long i = q.rows[e], j = q.cols ? q.cols[e] : i;
    double v = 0.0;
    if (!(q.zero_first && e == 0) && i >= 0 && i <= q.nx) {   // a row outside the mesh has no entry (and no nodal value)
      const double h = q.h[p], c = q.coef ? q.coef[p] : 1.0;
      const P1Nodal fn = q.fun ? P1Nodal{1, q.nx, q.fun + f * q.fun_width}
                               : P1Nodal{q.par_mode, q.nx, q.par ? q.par + p * (q.par_mode == 3 ? 3 : 1) : nullptr};
      v = p1_entry_value(q.kind, q.nx, i, j, h, c, fn);
    }
    // beta = 0 never reads out; otherwise v is a rounded double before it is added (two roundings, no fused form)
    q.out[t] = q.read_old ? __dadd_rn(__dmul_rn(q.beta, q.out[t]), v) : v;
  }
}

struct SsPlan {
  long total, workgroups;
  bool narrow;
};

// Argument checks and the launch plan: host logic only, shared by the entry point and its _plan_info twin.  No pointer
// is followed.
int ss_plan(int num_cus, int kind, int64_t nx, const int64_t* rows, const int64_t* cols, int64_t m, int64_t n_par,
            const double* h, int par_mode, const double* par, int64_t n_fun, const double* fun, const double* out, SsPlan* plan,
            const char** why) {
#define SS_ARG(cond)                   \
  do {                                 \
    if (!(cond)) {                     \
      *why = "bad argument: " #cond;   \
      return RT_ERR_ARG;               \
    }                                  \
  } while (0)
  SS_ARG(num_cus > 0);
  SS_ARG(kind >= RT_P1_MASS && kind <= RT_P1_LOAD_P2);
  SS_ARG(nx >= 2 && m >= 1 && n_par >= 1 && n_fun >= 1);
  SS_ARG(rows && h && out);
  SS_ARG((kind == RT_P1_LOAD || kind == RT_P1_LOAD_P2) || cols);
  SS_ARG(par_mode == 0 || par_mode == 2 || par_mode == 3);
  SS_ARG((par_mode == 0) == (par == nullptr));
  if (kind < RT_P1_TRILINEAR) {
    SS_ARG(par == nullptr && fun == nullptr && n_fun == 1);             // these integrate no nodal function
  } else {
    SS_ARG((par != nullptr) != (fun != nullptr));                       // exactly one of the two supplies it
    if (par) {
      SS_ARG(n_fun == 1);
      SS_ARG(par_mode == (kind == RT_P1_LOAD_P2 ? 3 : 2));              // the modes rt_p1_local_assembly takes for the kind
    }
  }
  SS_ARG(n_par <= (SS_MAX_COUNT - 1) / n_fun && n_par * n_fun <= (SS_MAX_COUNT - 1) / m);   // n_par n_fun m < 2^62, no overflow
#undef SS_ARG
  if (nx > SS_MAX_NX) {
    *why = "rt_p1_snapshot_sets: nx > 2^22";
    return RT_ERR_UNSUPPORTED;
  }
  const long total = (long)(n_par * n_fun * m);
  long wgs = (total + SS_THREADS - 1) / SS_THREADS;
  const long cap = (long)num_cus * SS_WG_PER_CU;
  if (wgs > cap) wgs = cap;
  *plan = SsPlan{total, wgs, total < (1L << 32)};
  return RT_OK;
}

}  // namespace

extern "C" int rt_p1_snapshot_sets_plan_info(int num_cus, int kind, int64_t nx, const int64_t* rows, const int64_t* cols,
                                             int64_t m, int64_t n_par, const double* h, const double* coef, int par_mode,
                                             const double* par, int64_t n_fun, const double* fun, int zero_first, double beta,
                                             const double* out, int64_t* info2) {
  (void)coef;
  (void)zero_first;
  (void)beta;
  SsPlan plan;
  const char* why = nullptr;
  RT_TRY(ss_plan(num_cus, kind, nx, rows, cols, m, n_par, h, par_mode, par, n_fun, fun, out, &plan, &why));
  if (info2) {
    info2[0] = plan.workgroups;
    info2[1] = 1;
  }
  return RT_OK;
}

extern "C" int rt_p1_snapshot_sets(rt_ctx* ctx, int kind, int64_t nx, const int64_t* rows, const int64_t* cols, int64_t m,
                                   int64_t n_par, const double* h, const double* coef, int par_mode, const double* par,
                                   int64_t n_fun, const double* fun, int zero_first, double beta, double* out) {
  if (!ctx) return RT_ERR_ARG;
  SsPlan plan;
  const char* why = nullptr;
  const int rc = ss_plan(ctx->num_cus, kind, nx, rows, cols, m, n_par, h, par_mode, par, n_fun, fun, out, &plan, &why);
  if (rc != RT_OK) {
    ctx->err = why;
    return rc;
  }
  SsParams q;
  q.kind = kind;
  q.par_mode = par_mode;
  q.zero_first = zero_first != 0;
  q.read_old = beta != 0.0;   // NaN included: beta = NaN reads
  q.nx = (long)nx;
  q.m = (long)m;
  q.n_fun = (long)n_fun;
  q.fun_width = p1_nodal_width(kind, 1, (long)nx);
  q.total = plan.total;
  q.rows = reinterpret_cast<const long*>(rows);
  q.cols = reinterpret_cast<const long*>(cols);
  q.h = h;
  q.coef = coef;
  q.par = par;
  q.fun = fun;
  q.beta = beta;
  q.out = out;
  if (plan.narrow)
    hipLaunchKernelGGL(p1_snapshot_sets_kernel<unsigned>, dim3((unsigned)plan.workgroups), dim3(SS_THREADS), 0, ctx->stream, q);
  else
    hipLaunchKernelGGL(p1_snapshot_sets_kernel<unsigned long>, dim3((unsigned)plan.workgroups), dim3(SS_THREADS), 0, ctx->stream, q);
  RT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_grid = plan.workgroups;
  ctx->last_splits = 1;
  ctx->last_tile = 1 * 1000 + SS_THREADS;
  return RT_OK;
}
