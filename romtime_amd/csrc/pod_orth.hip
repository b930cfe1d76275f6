// rt_pod_orth: the whole of `orth` (src/romtime/rom/pod.py:7-62) behind ONE C entry point, for hosts that bind the C ABI
// without the Python layer.  Same algorithm as romtime_amd/pod.py (which remains the fast path of the Python drop-in:
// it overlaps the eigenvalue fetch with the back-projection and knows about process groups):
//
//   G = X^T X (rt_gram) -> column norms, D^-1 G D^-1 (rt_gram_scale) -> all eigenvalues (rt_sym_eig_values; host Jacobi for
//   n < 3) -> sigma, energy, truncation rank with the reference's precedence tol > num > drop tolerance (pod.py:46-57) ->
//     shallow spectrum (not rt_deep): k eigenvectors (+ a k x k Rayleigh-Ritz step when the kept eigenvalues are not
//       rt_separated), Q = X D^-1 W S^-1;
//     deep spectrum: deflated levels - accept the modes rt_level_size counts, project them out of a working copy of the
//       snapshots twice, Gram + eigensolve again, until rt_levels_done (DESIGN.md "POD accuracy").
// This file orchestrates the device work.  Every decision taken from a spectrum, with its constants, is plain C++ in
// host_dense.{h,cpp} (the Python side: romtime_amd/pod_rules.py); so are the small dense steps on the host (k x k
// generalised eigenproblem of the Rayleigh-Ritz step): O(k^3) scalar work on kilobytes; everything of size N_h stays on the
// device.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "host_dense.h"

namespace {

// Zs[i][j] = Z[i][j] * rowscale[i] * colscale[j]   (n x k, row-major; either scale may be null)
__global__ void scale_rows_cols_kernel(const double* __restrict__ Z, int n, int k, const double* __restrict__ rowscale_inv,
                                       const double* __restrict__ colscale, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * k) return;
  const int i = (int)(idx / k), j = (int)(idx % k);
  double v = Z[idx];
  if (rowscale_inv) v /= rowscale_inv[i];
  if (colscale) v *= colscale[j];
  out[idx] = v;
}

// Zs[i][j] = Z[i][j] / colnorm[i] / sqrt(lam[j])  (0 where lam[j] <= 0): the n x k matrix D^-1 W S^-1 of the back-projection,
// straight from the device eigenvalues - nothing of it needs the host
__global__ void backproject_weights_kernel(const double* __restrict__ Z, int n, int k, const double* __restrict__ colnorm,
                                           const double* __restrict__ lam, double* __restrict__ out) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)n * k) return;
  const int i = (int)(idx / k), j = (int)(idx % k);
  const double l = lam[j];
  const double inv = l > 0.0 ? 1.0 / sqrt(l) : 0.0;
  double v = Z[idx];
  if (colnorm) v /= colnorm[i];
  out[idx] = v * inv;
}

// dst (N x n row-major) = src (N x n, strides ks / ms) * diag(1 / colnorm)   (colnorm null: plain copy)
__global__ void copy_scaled_kernel(const double* __restrict__ src, long rs, long cs, long N, int n,
                                   const double* __restrict__ colnorm, double* __restrict__ dst) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * n) return;
  const long i = idx / n;
  const int j = (int)(idx % n);
  const double v = src[i * rs + j * cs];
  dst[idx] = colnorm ? v / colnorm[j] : v;
}

struct Eig {                  // eigen-decomposition of one level's Gram matrix
  std::vector<double> lam;    // host, descending
  double* lam_d = nullptr;    // device copy (n), valid when on_device
  bool on_device = false;
  std::vector<double> W_host; // n x n eigenvectors (columns), host route only
  bool blocked = false;       // n > 2048: Ritz pairs of rt_sym_eig_blocked; Z holds the first `resolved` Ritz vectors
  int resolved = 0;
};

// One rt_pod_orth call: its sizes and its small persistent device buffers.  hipMallocAsync keeps them off the ctx arenas,
// which the operators called below carve for themselves; they go back to the pool when the call returns.
struct Pod {
  rt_ctx* ctx;
  hipStream_t st;
  int n;
  long N;
  int64_t q_cols;
  std::vector<void*> ptrs;
  double *G = nullptr, *colnorm = nullptr, *lam_d = nullptr;
  double *Z = nullptr, *Zs = nullptr;   // eigenvectors n x k (k <= n) and their scaled form
  double* scal = nullptr;               // inverse singular values of a level (k)
  double* small = nullptr;              // H and S of the Rayleigh-Ritz step / the deflation coefficients (k x n)
  int* flags = nullptr;                 // zero-norm flag, eigensolver status
  ~Pod() { for (void* p : ptrs) (void)hipFreeAsync(p, st); }
  double* get(size_t count) {
    void* p = nullptr;
    if (hipMallocAsync(&p, sizeof(double) * (count ? count : 1), st) != hipSuccess) return nullptr;
    ptrs.push_back(p);
    return static_cast<double*>(p);
  }
};

// All eigenvalues of Gm to the host (and lam_d); a hand-off timeout is retried once in the general form, then the host takes it
int eigensolve(Pod& p, const double* Gm, Eig& e) {
  rt_ctx* ctx = p.ctx;
  hipStream_t st = p.st;
  const int n = p.n;
  double* lam_d = p.lam_d;
  int* flags = p.flags;
  e.lam.assign(n, 0.0);
  e.on_device = (n >= 3);
  e.blocked = false;
  if (n > 2048) {
    // the block Rayleigh-Ritz route ("pod_blocked"): Ritz values (zeros beyond R) and all R Ritz vectors at once, into Z
    int64_t R = 0, ranks[8];
    int status = 0;
    RT_TRY(rt_sym_eig_blocked(ctx, Gm, n, n * 2.220446049250313e-16, n, lam_d, p.Z, &R, ranks, &status));
    if (status == RT_EIG_BLOCKED_NOT_REDUCIBLE) {
      ctx->err = "rt_pod_orth: the snapshot set is not reducible (more than 2048 block eigenvalues above n eps lam_max: "
                 "rt_sym_eig_blocked); use the pieces with a host eigensolver";
      return RT_ERR_UNSUPPORTED;
    }
    if (status != 0) {
      ctx->err = "rt_pod_orth: an eigensolve of rt_sym_eig_blocked timed out";
      return RT_ERR_HIP;
    }
    RT_HIP_CHECK(ctx, hipMemcpyAsync(e.lam.data(), lam_d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    e.lam_d = lam_d;
    e.blocked = true;
    e.resolved = (int)R;
    return RT_OK;
  }
  if (e.on_device) {
    RT_TRY(rt_sym_eig_values(ctx, Gm, n, lam_d, flags + 1));
    int status = 0;
    RT_HIP_CHECK(ctx, hipMemcpyAsync(e.lam.data(), lam_d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipMemcpyAsync(&status, flags + 1, sizeof(int), hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    e.lam_d = lam_d;
    if (status != 0 && ctx->eig_one_xcd) {  // hand-off timeout in the one-XCD form: once more in the general form
      ctx->eig_one_xcd = false;
      RT_TRY(rt_sym_eig_values(ctx, Gm, n, lam_d, flags + 1));
      RT_HIP_CHECK(ctx, hipMemcpyAsync(e.lam.data(), lam_d, sizeof(double) * n, hipMemcpyDeviceToHost, st));
      RT_HIP_CHECK(ctx, hipMemcpyAsync(&status, flags + 1, sizeof(int), hipMemcpyDeviceToHost, st));
      RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (status == 0) return RT_OK;
    e.on_device = false;  // timed out again: the host takes this eigenproblem
  }
  std::vector<double> A((size_t)n * n);
  RT_HIP_CHECK(ctx, hipMemcpyAsync(A.data(), Gm, sizeof(double) * n * n, hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
  e.W_host.assign((size_t)n * n, 0.0);
  int sweeps = 0;
  // shift to positive definiteness for the relative stopping rule (rounding can leave tiny negative eigenvalues)
  return rt_host_jacobi_eigh(A.data(), n, e.W_host.data(), e.lam.data(), 60, &sweeps);
}

// k leading eigenvectors of level `e` into Z (device, n x k row-major), Rayleigh-Ritz-repaired on G when clustered
int eigenvectors(Pod& p, const double* Gm, Eig& e, int k) {
  rt_ctx* ctx = p.ctx;
  hipStream_t st = p.st;
  const int n = p.n;
  double *Z = p.Z, *small = p.small;
  if (!e.on_device) {
    std::vector<double> Zh((size_t)n * k);
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < k; ++j) Zh[(size_t)i * k + j] = e.W_host[(size_t)i * n + j];
    RT_HIP_CHECK(ctx, hipMemcpyAsync(Z, Zh.data(), sizeof(double) * n * k, hipMemcpyHostToDevice, st));
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return RT_OK;
  }
  int kc = k;   // the columns that hold vectors: all k, but min(k, R) on the blocked route (leading dimension k either way)
  if (e.blocked) {
    // Z holds the R Ritz vectors with leading dimension R: compact the first min(k, R) columns to leading dimension k,
    // zero columns beyond R (their Ritz values are zero, and so are their modes)
    const int R = e.resolved;
    kc = std::min(k, R);
    double* tmp = p.Zs;  // free at this point
    RT_HIP_CHECK(ctx, hipMemsetAsync(tmp, 0, sizeof(double) * (size_t)n * k, st));
    if (kc > 0)
      RT_HIP_CHECK(ctx, hipMemcpy2DAsync(tmp, sizeof(double) * k, Z, sizeof(double) * R, sizeof(double) * kc, n,
                                         hipMemcpyDeviceToDevice, st));
    RT_HIP_CHECK(ctx, hipMemcpyAsync(Z, tmp, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToDevice, st));
    e.blocked = false;   // Z no longer holds the R vectors: a level asks for its vectors once
    if (kc == 0) return RT_OK;
  } else {
    RT_TRY(rt_sym_eig_vectors(ctx, n, k, e.lam_d, Z));
  }
  if (rt_separated(e.lam, kc)) return RT_OK;
  // clustered: H = Z^T G Z, S = Z^T Z, H c = theta S c on the host, Z <- Z C
  double* GZ = p.Zs;  // free at this point (on the blocked route its columns beyond kc are zero, and stay so)
  RT_TRY(rt_gemm_nn(ctx, Gm, n, RT_ROW_MAJOR, Z, k, n, n, kc, GZ, k, RT_ROW_MAJOR));
  RT_TRY(rt_gemm_tn(ctx, Z, k, RT_ROW_MAJOR, GZ, k, RT_ROW_MAJOR, n, kc, kc, small, kc));
  RT_TRY(rt_gemm_tn(ctx, Z, k, RT_ROW_MAJOR, Z, k, RT_ROW_MAJOR, n, kc, kc, small + (size_t)kc * kc, kc));
  std::vector<double> H((size_t)kc * kc), S((size_t)kc * kc), Cm, theta;
  RT_HIP_CHECK(ctx, hipMemcpyAsync(H.data(), small, sizeof(double) * kc * kc, hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(ctx, hipMemcpyAsync(S.data(), small + (size_t)kc * kc, sizeof(double) * kc * kc, hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
  for (int i = 0; i < kc; ++i)
    for (int j = i + 1; j < kc; ++j) {
      H[(size_t)i * kc + j] = H[(size_t)j * kc + i] = 0.5 * (H[(size_t)i * kc + j] + H[(size_t)j * kc + i]);
      S[(size_t)i * kc + j] = S[(size_t)j * kc + i] = 0.5 * (S[(size_t)i * kc + j] + S[(size_t)j * kc + i]);
    }
  if (!rt_small_generalised_eigh(H, S, kc, Cm, theta)) {
    ctx->err = "rt_pod_orth: the Rayleigh-Ritz overlap matrix is not positive definite";
    return RT_ERR_HIP;
  }
  double worst = 0.0;
  for (int i = 0; i < kc; ++i) worst = std::max(worst, std::fabs(theta[i] - e.lam[i]));
  if (worst > 1e-9 * std::max(e.lam[0], 1e-300)) {
    ctx->err = "rt_pod_orth: device eigenvectors failed the Rayleigh-Ritz cross-check";
    return RT_ERR_HIP;
  }
  RT_HIP_CHECK(ctx, hipMemcpyAsync(small, Cm.data(), sizeof(double) * kc * kc, hipMemcpyHostToDevice, st));
  RT_TRY(rt_gemm_nn(ctx, Z, k, RT_ROW_MAJOR, small, kc, n, kc, kc, GZ, k, RT_ROW_MAJOR));
  RT_HIP_CHECK(ctx, hipMemcpyAsync(Z, GZ, sizeof(double) * n * k, hipMemcpyDeviceToDevice, st));
  RT_HIP_CHECK(ctx, hipStreamSynchronize(st));   // Cm is on this stack frame
  return RT_OK;
}

// Qdst (N x k of the caller's Q) = src (N x n, strides src_rs / src_cs) [D^-1] Z diag(1 / sig): the level's modes
int back_project(Pod& p, const double* src, long src_rs, long src_cs, bool scale_rows, const double* sig, int k, double* Qdst) {
  rt_ctx* ctx = p.ctx;
  hipStream_t st = p.st;
  const int n = p.n;
  std::vector<double> inv(k);
  for (int i = 0; i < k; ++i) inv[i] = sig[i] > 0.0 ? 1.0 / sig[i] : 0.0;
  RT_HIP_CHECK(ctx, hipMemcpyAsync(p.scal, inv.data(), sizeof(double) * k, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(scale_rows_cols_kernel, dim3((unsigned)(((long)n * k + 255) / 256)), dim3(256), 0, st, p.Z, n, k,
                     scale_rows ? p.colnorm : nullptr, p.scal, p.Zs);
  RT_HIP_CHECK(ctx, hipGetLastError());
  RT_HIP_CHECK(ctx, hipStreamSynchronize(st));   // inv is on this stack frame
  const int src_layout = (src_cs == 1) ? RT_ROW_MAJOR : RT_COL_MAJOR;
  const long src_ld = (src_cs == 1) ? src_rs : src_cs;
  return rt_gemm_nn(ctx, src, src_ld, src_layout, p.Zs, k, p.N, n, k, Qdst, p.q_cols, RT_ROW_MAJOR);
}

}  // namespace

extern "C" int rt_pod_backproject_weights(rt_ctx* ctx, const double* Z, int64_t n, int64_t k, const double* colnorm,
                                          const double* lam, double* Zs) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, Z && lam && Zs && n >= 1 && k >= 1 && k <= n && n * k < (1LL << 31));
  hipLaunchKernelGGL(backproject_weights_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, ctx->stream, Z, (int)n,
                     (int)k, colnorm, lam, Zs);
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

extern "C" int rt_pod_enqueue(rt_ctx* ctx, const double* X, int64_t n_rows, int64_t n_cols, int64_t ld, int layout, int64_t k,
                              int normalize, double* G, double* colnorm, double* lam, int* status2, double* Z, double* Zs,
                              double* Q) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, X && G && colnorm && lam && status2 && Z && Zs && Q);
  RT_ARG_CHECK(ctx, n_rows >= 1 && n_cols >= 3 && n_cols <= 1024 && k >= 1 && k <= n_cols);
  RT_ARG_CHECK(ctx, layout == RT_ROW_MAJOR || layout == RT_COL_MAJOR);
  RT_TRY(rt_gram(ctx, X, n_rows, n_cols, ld, layout, G));
  RT_TRY(rt_gram_scale(ctx, G, n_cols, colnorm, normalize, status2 + 1));
  RT_TRY(rt_sym_eig_values(ctx, G, n_cols, lam, status2));
  RT_TRY(rt_sym_eig_vectors(ctx, n_cols, k, lam, Z));
  RT_TRY(rt_pod_backproject_weights(ctx, Z, n_cols, k, normalize ? colnorm : nullptr, lam, Zs));
  return rt_gemm_nn(ctx, X, ld, layout, Zs, k, n_rows, n_cols, k, Q, k, RT_ROW_MAJOR);
}

extern "C" int rt_pod_orth(rt_ctx* ctx, const double* X, int64_t n_rows, int64_t n_cols, int64_t ld, int layout, int64_t num,
                           double tol, int normalize, double* Q, int64_t q_cols, int64_t* r_out, double* s_host,
                           double* energy_host, int* levels_out) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, X && Q && r_out && s_host && energy_host && n_rows >= 1 && n_cols >= 1 && q_cols >= 0 && num >= 0);
  RT_ARG_CHECK(ctx, layout == RT_ROW_MAJOR || layout == RT_COL_MAJOR);
  RT_ARG_CHECK(ctx, ld >= (layout == RT_ROW_MAJOR ? n_cols : n_rows));
  if (n_cols > 2048 && !(ctx->pod_blocked && n_cols <= 16384)) {
    ctx->err = "rt_pod_orth: more than 2048 snapshots (the device eigensolver's limit; use the pieces with a host eigensolver)";
    return RT_ERR_UNSUPPORTED;
  }
  const int n = (int)n_cols;
  const long N = n_rows;
  const long rs = (layout == RT_ROW_MAJOR) ? ld : 1, cs = (layout == RT_ROW_MAJOR) ? 1 : ld;
  hipStream_t st = ctx->stream;
  *r_out = 0;
  if (levels_out) *levels_out = 0;

  Pod p{ctx, st, n, N, q_cols};
  p.G = p.get((size_t)n * n);
  p.colnorm = p.get(n);
  p.lam_d = p.get(n);
  p.Z = p.get((size_t)n * n);
  p.Zs = p.get((size_t)n * n);
  p.scal = p.get(n);
  p.small = p.get((size_t)2 * n * n);
  p.flags = reinterpret_cast<int*>(p.get(2));
  if (!p.G || !p.colnorm || !p.lam_d || !p.Z || !p.Zs || !p.scal || !p.small || !p.flags) {
    ctx->err = "rt_pod_orth: hipMallocAsync failed";
    return RT_ERR_HIP;
  }

  auto finish = [&](const std::vector<double>& s, const std::vector<double>& energy, int r) {
    // more snapshots than DoFs: the thin SVD has only min(N, n) singular values (pod.py:38)
    const int len = (int)std::min<long>(N, n);
    for (int i = 0; i < len; ++i) { s_host[i] = s[i]; energy_host[i] = energy[i]; }
    *r_out = std::min(r, len);
  };
  auto no_room = [&](const std::vector<double>& s, const std::vector<double>& energy, int r) {
    finish(s, energy, r);
    ctx->err = "rt_pod_orth: Q has fewer columns than the modes kept (r_out holds the number needed)";
    return RT_ERR_ARG;
  };

  // ---- level 0 ------------------------------------------------------------------------------------------------------
  RT_TRY(rt_gram(ctx, X, n_rows, n_cols, ld, layout, p.G));
  RT_TRY(rt_gram_scale(ctx, p.G, n, p.colnorm, normalize, p.flags));
  Eig eig;
  RT_TRY(eigensolve(p, p.G, eig));
  int zero_norm = 0;
  RT_HIP_CHECK(ctx, hipMemcpyAsync(&zero_norm, p.flags, sizeof(int), hipMemcpyDeviceToHost, st));
  RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
  if (normalize && zero_norm) {
    // the reference divides by a zero norm and scipy.linalg.svd then rejects the NaNs (pod.py:32-38)
    ctx->err = "rt_pod_orth: zero-norm snapshot with normalize (the reference raises: array must not contain infs or NaNs)";
    return RT_WARN_ZERO_NORM;
  }
  const std::vector<double> s = rt_sigma(eig.lam);
  std::vector<double> energy;
  double total = 0.0;   // the energy denominator of every level
  if (eig.blocked) {
    // the Ritz values stop at R: the energy stays over trace(G), which their sum misses by the discarded block energy
    std::vector<double> diag(n);
    RT_HIP_CHECK(ctx, hipMemcpy2DAsync(diag.data(), sizeof(double), p.G, sizeof(double) * (n + 1), sizeof(double), n,
                                       hipMemcpyDeviceToHost, st));
    RT_HIP_CHECK(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) total += diag[i];
  } else {
    for (int i = 0; i < n; ++i) total += s[i] * s[i];
  }
  rt_energy(s, total, energy);
  int r = rt_truncation_rank(s, energy, num, tol);
  if (levels_out) *levels_out = 1;
  if (r == 0) {
    finish(s, energy, 0);
    return RT_OK;
  }
  if (std::min<long>(r, std::min<long>(N, n)) > q_cols) return no_room(s, energy, r);

  // ---- shallow spectrum: one Gram pass -------------------------------------------------------------------------------------
  if (!rt_deep(s, r)) {
    RT_TRY(eigenvectors(p, p.G, eig, r));
    RT_TRY(back_project(p, X, rs, cs, normalize != 0, s.data(), r, Q));
    finish(s, energy, r);
    return RT_OK;
  }

  // ---- deflated levels (romtime_amd/pod.py::_pod_deflated) ---------------------------------------------------------------
  // working copy of the snapshots (row-major).  Not from the ctx's composite arena: the eigensolver keeps its reflectors
  // there between rt_sym_eig_values and rt_sym_eig_vectors.
  double* Xc = p.get((size_t)N * n);
  if (!Xc) { ctx->err = "rt_pod_orth: hipMallocAsync failed (working copy of the snapshots)"; return RT_ERR_HIP; }
  bool have_copy = false;
  std::vector<double> s_acc;
  const int cap = (num != 0 && tol == 0.0) ? (int)std::min<int64_t>(num, n) : n;
  int levels = 0;
  std::vector<double> s_full, e_full;
  const double* Gl = p.G;
  double* G2 = nullptr;
  RT_HIP_CHECK(ctx, hipMemsetAsync(Q, 0, sizeof(double) * (size_t)N * q_cols, st));  // columns beyond the numerical rank stay zero
  for (;;) {
    ++levels;
    const std::vector<double> sig = rt_sigma(eig.lam);
    const int have = (int)s_acc.size();
    const int k = rt_level_size(sig, have, have ? s_acc[0] : 0.0, std::min<int>(cap, (int)q_cols) - have);
    if (k > 0) {
      RT_TRY(eigenvectors(p, Gl, eig, k));
      if (!have_copy) RT_TRY(back_project(p, X, rs, cs, normalize != 0, sig.data(), k, Q + have));
      else RT_TRY(back_project(p, Xc, n, 1, false, sig.data(), k, Q + have));
      s_acc.insert(s_acc.end(), sig.begin(), sig.begin() + k);
    }
    const int got = have + k;
    const int tail_n = rt_merged_spectrum(s_acc, sig, k, total, s_full, e_full);
    r = rt_truncation_rank(s_full, e_full, num, tol);
    if (r > q_cols && std::min<long>(r, std::min<long>(N, n)) > q_cols) return no_room(s_full, e_full, r);
    if (rt_levels_done(r, got, k, n, levels, tail_n, tail_n > 0 ? sig[k] : 0.0)) break;
    // deflate: X <- X - Q_l (Q_l^T X), twice; the first sweep of the first level reads the caller's snapshots and writes
    // the (column-normalised) working copy
    const double* Ql = Q + have;
    for (int sweep = 0; sweep < 2; ++sweep) {
      double* Cm = p.small;   // k x n
      if (!have_copy) {
        hipLaunchKernelGGL(copy_scaled_kernel, dim3((unsigned)((N * n + 255) / 256)), dim3(256), 0, st, X, rs, cs, N, n,
                           normalize ? p.colnorm : nullptr, Xc);
        RT_HIP_CHECK(ctx, hipGetLastError());
        have_copy = true;
      }
      RT_TRY(rt_gemm_tn(ctx, Ql, q_cols, RT_ROW_MAJOR, Xc, n, RT_ROW_MAJOR, N, k, n, Cm, n));
      if (k <= 64) {
        RT_TRY(rt_rank_update(ctx, Xc, n, nullptr, Ql, q_cols, Cm, n, N, k, n, -1.0, Xc, n));
      } else {
        RT_TRY(rt_gemm_nn_axpby(ctx, Ql, q_cols, RT_ROW_MAJOR, Cm, n, N, k, n, -1.0, 1.0, Xc, n, RT_ROW_MAJOR));
      }
    }
    if (!G2) G2 = p.get((size_t)n * n);
    if (!G2) { ctx->err = "rt_pod_orth: hipMallocAsync failed"; return RT_ERR_HIP; }
    RT_TRY(rt_gram(ctx, Xc, N, n, n, RT_ROW_MAJOR, G2));
    Gl = G2;
    RT_TRY(eigensolve(p, G2, eig));
  }
  if (levels_out) *levels_out = levels;
  finish(s_full, e_full, r);
  return RT_OK;
}
