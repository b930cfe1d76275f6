// Interpolation errors of a whole block of snapshots against their (M)DEIM interpolant, without storing a theta array, an
// interpolant or a modified copy of the snapshots:
//   err[q] = (1/g) sum_{i<g} || f_s - I(f_s) ||_2 / sqrt(N),  s = q g + i,   I(f) = Psi f[idx],  Psi = basis_fom PT_U^-1
// with entry pin_row of I(f) replaced by pin_value (MDEIM's Dirichlet entry, deim.py:449-450, nonlinear.py:280-281), and
//   ref[q] = (1/g) sum_{i<g} || f_s ||_2 / sqrt(N)
// (evaluate of the three (M)DEIM classes, deim.py:226-261 and nonlinear.py:470-540: compute_error per sample and for
// N-MDEIM the mean over the states, a running sum in index order and one division, nonlinear.py:518-535).
//
// traj_error.hip's structure with the coefficients taken from the data: a workgroup (4 waves) owns 64 snapshots and walks
// down a slice of rows in stages of 32.  Its 64 x m coefficient block is gathered once, rows idx of its own snapshots
// (te_gather_coefficients), the 32 x m stages of Psi go global -> registers -> LDS with the next stage in flight
// (TeStageLoader, traj_stage.h), each wave multiplies one 16-row block by two 16-snapshot tiles on the f64 matrix cores,
// loads its 8 words of the F tile straight into the accumulator layout, and folds (f - l)^2 into per-lane column sums.
// An FP64 MFMA blocks the VALU of its SIMD (see traj_error.hip), so the pin costs ordinary stages nothing per word: the
// stage that holds pin_row is recognised by one scalar compare and runs its own copy of the epilogue, in which the
// interpolant's word of that row is pin_value.  ref always sums the data as they are.  The interpolation indices travel in
// the kernel's argument block (m <= 128 of them: 1 KB), checked on the host before any launch.
//
// Nothing is accumulated with atomics: a workgroup writes its 64 partial sums to [snapshot][row slice], a finish kernel adds
// the slices in order and applies sqrt and the division, a second one forms the group means.  The slicing depends on N
// and the CU count only - not on S, unlike the siblings' - so the bits of a snapshot's error depend neither on S, its
// place in the block, nor group: callers chunk their snapshot sets.
#include <cmath>
#include <type_traits>

#include "common.h"
#include "traj_stage.h"

// (f - l), the square and the sums are separate IEEE operations, as NumPy's are: exact data then gives NumPy's bits
#pragma clang fp contract(off)

namespace {

constexpr int IE_MAX_M = 128;

struct IeParams {
  const double *Psi, *F;
  double *perr, *pref;                                    // partial sums [snapshot][slice]; pref may be null
  long ldpsi, ldf, N, S, slice_rows;
  long pin_stage;                                         // first row of the stage that holds pin_row, -1 without a pin
  double pin_value;
  int pin_local;                                          // pin_row - pin_stage
  int m, kp, slices, step_blocks;
  long idx[IE_MAX_M];
};

template <bool COLMAJ>
__global__ __launch_bounds__(TE_THREADS, 2) void interp_error_kernel(const IeParams p) {
  extern __shared__ __attribute__((aligned(16))) double ie_smem[];
  const int S = p.kp + 2;                                 // S / 2 odd: the 16 rows of an operand read fall in distinct banks
  const int hp = p.kp >> 1;
  double* sC = ie_smem;                                   // [64 snapshots][S] coefficients
  double* sB = sC + TE_TB * S;                            // [32 rows][S] current stage of Psi
  double* sRed = sB + TE_RS * S;                          // [err | ref][wave][32 snapshots]
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rb = wid & 1, tg = wid >> 1;
  const unsigned bid = blockIdx.x;
  const int sb = (int)(bid % (unsigned)p.step_blocks);
  const int slice = (int)(bid / (unsigned)p.step_blocks);
  const long t0 = (long)sb * TE_TB;
  const long row_lo = (long)slice * p.slice_rows;
  const long row_hi = row_lo + p.slice_rows < p.N ? row_lo + p.slice_rows : p.N;
  const bool want_ref = p.pref != nullptr;

  te_gather_coefficients<COLMAJ>(sC, p.F, p.ldf, p.idx, t0, p.S, p.m, p.kp, S, tid);
  TeStageLoader stage;
  stage.init(p.Psi, p.ldpsi, p.N, p.m, hp, S, sB, tid);

  // this lane's words of the F tile, in the accumulator layout (tile j, register c): row (lane >> 4) + 4 c, column lane & 15
  long foff[TE_TW][4];
  bool fstep[TE_TW][4];
  int frow[4];
#pragma unroll
  for (int j = 0; j < TE_TW; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int step = 16 * (TE_TW * tg + j) + (COLMAJ ? l4 + 4 * c : l15);
      const int row = 16 * rb + (COLMAJ ? l15 : l4 + 4 * c);
      frow[c] = row;
      fstep[j][c] = t0 + step < p.S;
      foff[j][c] = COLMAJ ? (t0 + step) * p.ldf + row : (long)row * p.ldf + t0 + step;
    }

  double se[TE_TW][4], sr[TE_TW][4];
#pragma unroll
  for (int j = 0; j < TE_TW; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) se[j][c] = sr[j][c] = 0.0;

  stage.fetch(row_lo);
  stage.commit();
  __syncthreads();
  const double* fb = sB + (16 * rb + l15) * S + l4;       // operand words: index lane & 15, k = 4 k4 + (lane >> 4)
  const double* fc = sC + (16 * TE_TW * tg + l15) * S + l4;
  for (long r0 = row_lo; r0 < row_hi; r0 += TE_RS) {
    const bool more = r0 + TE_RS < row_hi;
    if (more) stage.fetch(r0 + TE_RS);
    double f[TE_TW][4];
    {
      const double* base = p.F + (COLMAJ ? r0 : r0 * p.ldf);
#pragma unroll
      for (int j = 0; j < TE_TW; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) f[j][c] = (fstep[j][c] && r0 + frow[c] < p.N) ? base[foff[j][c]] : 0.0;
    }
    d4 acc[TE_TW];
#pragma unroll
    for (int j = 0; j < TE_TW; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    auto mma = [&](int k4) {
      const double b = fb[k4];
#pragma unroll
      for (int j = 0; j < TE_TW; ++j) {
        const double a = fc[16 * j * S + k4];
        acc[j] = COLMAJ ? __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0)    // tile[snapshot][row]
                        : __builtin_amdgcn_mfma_f64_16x16x4f64(b, a, acc[j], 0, 0, 0);   // tile[row][snapshot]
      }
    };
    int k4 = 0;
    for (; k4 + 16 <= p.kp; k4 += 16) {                   // four k-steps at a time: their operand reads go out together
#pragma unroll
      for (int i = 0; i < 4; ++i) mma(k4 + 4 * i);
    }
    for (; k4 < p.kp; k4 += 4) mma(k4);
    // rows past N and snapshots past S: the operands and the F words are zero there, so they add nothing (a pinned word of
    // a snapshot past S is not zero, but it sits in a column of its own that is never written)
    auto epilogue = [&](auto pinned) {
#pragma unroll
      for (int j = 0; j < TE_TW; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double l = acc[j][c];
          if (decltype(pinned)::value) l = frow[c] == p.pin_local ? p.pin_value : l;
          const double d = f[j][c] - l;
          if (want_ref) sr[j][c] += f[j][c] * f[j][c];
          se[j][c] += d * d;
        }
    };
    if (r0 == p.pin_stage)                                // uniform: one scalar compare per stage
      epilogue(std::true_type{});
    else
      epilogue(std::false_type{});
    __syncthreads();
    if (more) stage.commit();
    __syncthreads();
  }

  // column sums: over this lane's registers and the lanes that hold other rows of the same snapshot, then over the two row
  // blocks, always in the same order
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    if (e == 1 && !want_ref) break;
    double* red = sRed + e * 4 * 32 + wid * 32;
#pragma unroll
    for (int j = 0; j < TE_TW; ++j) {
      if (COLMAJ) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          double v = e ? sr[j][c] : se[j][c];
          v += __shfl_xor(v, 1);
          v += __shfl_xor(v, 2);
          v += __shfl_xor(v, 4);
          v += __shfl_xor(v, 8);
          if (l15 == 0) red[16 * j + l4 + 4 * c] = v;
        }
      } else {
        double v = e ? (sr[j][0] + sr[j][1]) + (sr[j][2] + sr[j][3]) : (se[j][0] + se[j][1]) + (se[j][2] + se[j][3]);
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        if (l4 == 0) red[16 * j + l15] = v;
      }
    }
  }
  __syncthreads();
  if (tid < TE_TB && t0 + tid < p.S) {
    const int w0 = 2 * (tid >> 5), s = tid & 31;          // the waves of tile group tid / 32: row blocks 0 and 1
    const long out = (t0 + tid) * p.slices + slice;
    p.perr[out] = sRed[w0 * 32 + s] + sRed[(w0 + 1) * 32 + s];
    if (want_ref) p.pref[out] = sRed[4 * 32 + w0 * 32 + s] + sRed[4 * 32 + (w0 + 1) * 32 + s];
  }
}

// per snapshot: the slices in order, the correctly rounded sqrt and division
__global__ __launch_bounds__(256) void interp_error_finish_kernel(const double* perr, const double* pref, double* err, double* ref,
                                                                  int slices, long S, double sqrt_n) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  double a = 0.0;
  for (int i = 0; i < slices; ++i) a += perr[s * slices + i];
  err[s] = __dsqrt_rn(a) / sqrt_n;
  if (ref) {
    double b = 0.0;
    for (int i = 0; i < slices; ++i) b += pref[s * slices + i];
    ref[s] = __dsqrt_rn(b) / sqrt_n;
  }
}

// per group: a running sum in index order, then one division (nonlinear.py:518-535)
__global__ __launch_bounds__(256) void interp_error_group_kernel(const double* es, const double* rs, double* err, double* ref,
                                                                 long group, long groups) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q >= groups) return;
  const double g = (double)group;
  double a = 0.0;
  for (long i = 0; i < group; ++i) a += es[q * group + i];
  err[q] = a / g;
  if (ref) {
    double b = 0.0;
    for (long i = 0; i < group; ++i) b += rs[q * group + i];
    ref[q] = b / g;
  }
}

struct IePlan {
  long step_blocks, slices, slice_rows, grid;
};

// Argument checks and the slicing: host logic only, shared by the entry point and rt_interpolation_errors_plan_info.
// idx is a HOST array and is read here; no other pointer is followed.
int ie_plan(int num_cus, const double* Psi, int64_t ldpsi, const int64_t* idx, int64_t m, const double* F, int64_t ldf,
            int f_layout, int64_t N, int64_t S, int64_t group, int64_t pin_row, const double* err, IePlan* plan,
            const char** why) {
#define IE_ARG(cond)                       \
  do {                                     \
    if (!(cond)) {                         \
      *why = "bad argument: " #cond;       \
      return RT_ERR_ARG;                   \
    }                                      \
  } while (0)
  IE_ARG(num_cus > 0);
  IE_ARG(Psi && idx && F && err);
  IE_ARG(N > 0 && m > 0 && S > 0 && group > 0);
  IE_ARG(S % group == 0);
  IE_ARG(pin_row >= -1 && pin_row < N);
  IE_ARG(f_layout == RT_ROW_MAJOR || f_layout == RT_COL_MAJOR);
  IE_ARG(ldpsi >= m);
  IE_ARG(ldf >= (f_layout == RT_COL_MAJOR ? N : S));
  if (m > IE_MAX_M) {
    *why = "rt_interpolation_errors: m > 128";
    return RT_ERR_UNSUPPORTED;
  }
  for (int64_t e = 0; e < m; ++e) IE_ARG(idx[e] >= 0 && idx[e] < N);
#undef IE_ARG
  const long step_blocks = (S + TE_TB - 1) / TE_TB;
  // row slices: one workgroup per CU for a single block of 64 snapshots where N allows, never fewer than TE_SLICE_ROWS
  // rows each (whole stages); S has no say, so a snapshot's sums are cut the same way in every chunk
  long slices = num_cus;
  const long most = (N + TE_SLICE_ROWS - 1) / TE_SLICE_ROWS;
  if (slices > most) slices = most;
  const long slice_rows = ((N + slices - 1) / slices + TE_RS - 1) / TE_RS * TE_RS;
  slices = (N + slice_rows - 1) / slice_rows;
  const long grid = step_blocks * slices;
  if (grid >= (1L << 31)) {
    *why = "rt_interpolation_errors: more than 2^31 workgroups";
    return RT_ERR_UNSUPPORTED;
  }
  *plan = IePlan{step_blocks, slices, slice_rows, grid};
  return RT_OK;
}

}  // namespace

int rt_interpolation_errors_plan_info(int num_cus, const double* Psi, int64_t ldpsi, const int64_t* idx, int64_t m,
                                      const double* F, int64_t ldf, int f_layout, int64_t N, int64_t S, int64_t group,
                                      int64_t pin_row, double pin_value, const double* err, const double* ref, int64_t* info3) {
  (void)pin_value;
  (void)ref;
  IePlan plan;
  const char* why = nullptr;
  RT_TRY(ie_plan(num_cus, Psi, ldpsi, idx, m, F, ldf, f_layout, N, S, group, pin_row, err, &plan, &why));
  if (info3) {
    info3[0] = plan.grid;
    info3[1] = plan.slices;
    info3[2] = TE_RS * 1000 + TE_TB;
  }
  return RT_OK;
}

int rt_interpolation_errors(rt_ctx* ctx, const double* Psi, int64_t ldpsi, const int64_t* idx, int64_t m, const double* F,
                            int64_t ldf, int f_layout, int64_t N, int64_t S, int64_t group, int64_t pin_row, double pin_value,
                            double* err, double* ref) {
  if (!ctx) return RT_ERR_ARG;
  IePlan plan;
  const char* why = nullptr;
  const int rc = ie_plan(ctx->num_cus, Psi, ldpsi, idx, m, F, ldf, f_layout, N, S, group, pin_row, err, &plan, &why);
  if (rc != RT_OK) {
    ctx->err = why;
    return rc;
  }
  const size_t part = (size_t)S * plan.slices * 8;
  rt_carver carve;
  const size_t o_perr = carve.add(part), o_pref = carve.add(ref ? part : 0);
  const size_t o_es = carve.add(group > 1 ? (size_t)S * 8 : 0), o_rs = carve.add(group > 1 && ref ? (size_t)S * 8 : 0);
  void* scratch = nullptr;
  RT_TRY(rt_scratch(ctx, carve.total(), &scratch));
  const int kp = (int)((m + 3) / 4 * 4);
  IeParams p;
  p.Psi = Psi;
  p.F = F;
  p.perr = rt_carver::at<double>(scratch, o_perr);
  p.pref = ref ? rt_carver::at<double>(scratch, o_pref) : nullptr;
  p.ldpsi = ldpsi;
  p.ldf = ldf;
  p.N = N;
  p.S = S;
  p.slice_rows = plan.slice_rows;
  p.pin_stage = pin_row >= 0 ? pin_row / TE_RS * TE_RS : -1;
  p.pin_value = pin_value;
  p.pin_local = pin_row >= 0 ? (int)(pin_row - p.pin_stage) : -1;
  p.m = (int)m;
  p.kp = kp;
  p.slices = (int)plan.slices;
  p.step_blocks = (int)plan.step_blocks;
  for (int e = 0; e < IE_MAX_M; ++e) p.idx[e] = e < m ? idx[e] : 0;
  const int lds = ((TE_TB + TE_RS) * (kp + 2) + 2 * 4 * 32) * 8;
  const int lds_max = ((TE_TB + TE_RS) * (IE_MAX_M + 2) + 2 * 4 * 32) * 8;
  if (f_layout == RT_COL_MAJOR) {
    RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&interp_error_kernel<true>), lds_max));
    hipLaunchKernelGGL((interp_error_kernel<true>), dim3((unsigned)plan.grid), dim3(TE_THREADS), lds, ctx->stream, p);
  } else {
    RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&interp_error_kernel<false>), lds_max));
    hipLaunchKernelGGL((interp_error_kernel<false>), dim3((unsigned)plan.grid), dim3(TE_THREADS), lds, ctx->stream, p);
  }
  RT_HIP_CHECK(ctx, hipGetLastError());
  double* es = group > 1 ? rt_carver::at<double>(scratch, o_es) : err;
  double* rs = !ref ? nullptr : (group > 1 ? rt_carver::at<double>(scratch, o_rs) : ref);
  hipLaunchKernelGGL(interp_error_finish_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, ctx->stream, p.perr, p.pref, es,
                     rs, (int)plan.slices, (long)S, std::sqrt((double)N));
  RT_HIP_CHECK(ctx, hipGetLastError());
  if (group > 1) {
    const long groups = S / group;
    hipLaunchKernelGGL(interp_error_group_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, ctx->stream, es, rs, err,
                       ref, (long)group, groups);
    RT_HIP_CHECK(ctx, hipGetLastError());
  }
  ctx->last_grid = plan.grid;
  ctx->last_splits = plan.slices;
  ctx->last_tile = TE_RS * 1000 + TE_TB;
  return RT_OK;
}
