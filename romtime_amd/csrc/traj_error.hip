// Error curves of whole reduced trajectories against full-order snapshots, without storing the lifted trajectory:
//   err[j][t] = || U_j[:, t] - B a_j[t] ||_2 / sqrt(N),   ref[j][t] = || U_j[:, t] ||_2 / sqrt(N)
// (compute_error per time step, rom/base.py:52-73, and with U absent the S-ROM estimator compute_rom_difference,
// utils.py:173-212: the three curves of HyperReducedPiston._evaluate, hrom.py:546-582).
//
// The lifted trajectory is a GEMM N x nt x k (k <= 128) whose output is only ever subtracted from U, squared and summed
// down the rows, so it never leaves the accumulators.  A workgroup (4 waves) owns 64 steps and walks down a slice of
// rows in stages of 32: the 64 x k coefficient block stays in LDS, the 32 x k stages of B go global -> registers -> LDS
// with the next stage in flight while the current one is multiplied (tallskinny.hip's scheme; the loader is
// traj_stage.h, shared with traj_output.hip), each wave multiplies one
// 16-row block by two 16-step tiles on the f64 matrix cores, loads its 8 words of the U tile straight into the
// accumulator layout at the top of the stage (they arrive under the MFMAs), and folds (u - l)^2 into per-lane column
// sums that stay in registers until the slice is done.  An FP64 MFMA blocks the VALU of its SIMD: the loader's offsets
// and predicates are computed once per workgroup, a stage costs 2 VALU per load for the address, and the epilogue is 3
// (5 with ref) f64 operations per accumulator word.  The two operands of v_mfma_f64_16x16x4_f64 have the same lane map
// (index = lane & 15, k = lane >> 4), so swapping them transposes the result tile: with U row-major the steps lie along
// lane & 15, with U column-major (each snapshot contiguous) the rows do, and either way a U load touches whole 128-byte
// lines.  LDS (96 (kp + 2) + 256) * 8 bytes, kp = k rounded up to 4: 68 KB at k = 81, two workgroups per CU up to
// kp = 100, one beyond.
//
// Nothing is accumulated with atomics: a workgroup writes its 64 partial sums to [trajectory][row slice][step], a second
// kernel adds the slices in order and applies sqrt and the division.  The slicing depends on N, nt and the CU count only,
// so a trajectory's bits depend neither on n_traj nor on its place in the batch.
#include <cmath>

#include "common.h"
#include "traj_stage.h"

// (u - l)^2 and the sums are separate IEEE operations, as NumPy's are: exact data then gives NumPy's bits
#pragma clang fp contract(off)

namespace {

struct TeParams {
  const double *B, *A, *U;
  double *perr, *pref;                                    // partial sums [trajectory][slice][step]; pref may be null
  long ldb, lda, stride_a, ldu, stride_u, N, nt, slice_rows;
  int k, kp, slices, step_blocks;
};

template <bool COLMAJ>
__global__ __launch_bounds__(TE_THREADS, 2) void traj_error_kernel(const TeParams p) {
  extern __shared__ __attribute__((aligned(16))) double te_smem[];
  const int S = p.kp + 2;                                 // S / 2 odd: the 16 rows of an operand read fall in distinct banks
  const int hp = p.kp >> 1;
  double* sC = te_smem;                                   // [64 steps][S] coefficients
  double* sB = sC + TE_TB * S;                            // [32 rows][S] current stage of B
  double* sRed = sB + TE_RS * S;                          // [err | ref][wave][32 steps]
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
  const long row_hi = row_lo + p.slice_rows < p.N ? row_lo + p.slice_rows : p.N;
  const double* A = p.A + traj * p.stride_a;
  const double* U = p.U ? p.U + traj * p.stride_u : nullptr;
  const bool want_ref = p.pref != nullptr;

  te_load_coefficients(sC, A, p.lda, t0, p.nt, p.k, hp, S, tid);
  TeStageLoader stage;
  stage.init(p.B, p.ldb, p.N, p.k, hp, S, sB, tid);

  // this lane's words of the U tile, in the accumulator layout (tile j, register c): row (lane >> 4) + 4 c, column lane & 15
  long uoff[TE_TW][4];
  bool ustep[TE_TW][4];
  int urow[4];
#pragma unroll
  for (int j = 0; j < TE_TW; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int step = 16 * (TE_TW * tg + j) + (COLMAJ ? l4 + 4 * c : l15);
      const int row = 16 * rb + (COLMAJ ? l15 : l4 + 4 * c);
      urow[c] = row;
      ustep[j][c] = t0 + step < p.nt;
      uoff[j][c] = COLMAJ ? (t0 + step) * p.ldu + row : (long)row * p.ldu + t0 + step;
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
    double u[TE_TW][4];
    if (U) {
      const double* ub = U + (COLMAJ ? r0 : r0 * p.ldu);
#pragma unroll
      for (int j = 0; j < TE_TW; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) u[j][c] = (ustep[j][c] && r0 + urow[c] < p.N) ? ub[uoff[j][c]] : 0.0;
    }
    d4 acc[TE_TW];
#pragma unroll
    for (int j = 0; j < TE_TW; ++j) acc[j] = d4{0.0, 0.0, 0.0, 0.0};
    auto mma = [&](int k4) {
      const double b = fb[k4];
#pragma unroll
      for (int j = 0; j < TE_TW; ++j) {
        const double a = fc[16 * j * S + k4];
        acc[j] = COLMAJ ? __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0)    // tile[step][row]
                        : __builtin_amdgcn_mfma_f64_16x16x4f64(b, a, acc[j], 0, 0, 0);   // tile[row][step]
      }
    };
    int k4 = 0;
    for (; k4 + 16 <= p.kp; k4 += 16) {                   // four k-steps at a time: their operand reads go out together
#pragma unroll
      for (int i = 0; i < 4; ++i) mma(k4 + 4 * i);
    }
    for (; k4 < p.kp; k4 += 4) mma(k4);
    // rows past N and steps past nt: the operands and the U words are zero there, so they add nothing
#pragma unroll
    for (int j = 0; j < TE_TW; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        double d = acc[j][c];
        if (U) {
          d = u[j][c] - d;
          if (want_ref) sr[j][c] += u[j][c] * u[j][c];
        }
        se[j][c] += d * d;
      }
    __syncthreads();
    if (more) stage.commit();
    __syncthreads();
  }

  // column sums: over this lane's registers and the lanes that hold other rows of the same step, then over the two row
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
  if (tid < TE_TB && t0 + tid < p.nt) {
    const int w0 = 2 * (tid >> 5), s = tid & 31;          // the waves of tile group tid / 32: row blocks 0 and 1
    const long out = (traj * p.slices + slice) * p.nt + t0 + tid;
    p.perr[out] = sRed[w0 * 32 + s] + sRed[(w0 + 1) * 32 + s];
    if (want_ref) p.pref[out] = sRed[4 * 32 + w0 * 32 + s] + sRed[4 * 32 + (w0 + 1) * 32 + s];
  }
}

__global__ __launch_bounds__(256) void traj_error_finish_kernel(const double* perr, const double* pref, double* err, double* ref,
                                                                long nt, int slices, long total, double sqrt_n) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long traj = idx / nt, t = idx - traj * nt;
  const long first = traj * slices * nt + t;
  double s = 0.0;
  for (int i = 0; i < slices; ++i) s += perr[first + i * nt];
  err[idx] = __dsqrt_rn(s) / sqrt_n;
  if (ref) {
    double q = 0.0;
    for (int i = 0; i < slices; ++i) q += pref[first + i * nt];
    ref[idx] = __dsqrt_rn(q) / sqrt_n;
  }
}

}  // namespace

int rt_trajectory_errors(rt_ctx* ctx, const double* B, int64_t ldb, const double* A, int64_t lda, int64_t stride_a,
                         const double* U, int64_t ldu, int u_layout, int64_t stride_u, int64_t N, int64_t k, int64_t nt,
                         int64_t n_traj, double* err, double* ref) {
  if (!ctx) return RT_ERR_ARG;
  RT_ARG_CHECK(ctx, B && A && err);
  RT_ARG_CHECK(ctx, N > 0 && k > 0 && nt > 0 && n_traj > 0);
  RT_ARG_CHECK(ctx, ldb >= k && lda >= k);
  RT_ARG_CHECK(ctx, U || !ref);
  if (U) {
    RT_ARG_CHECK(ctx, u_layout == RT_ROW_MAJOR || u_layout == RT_COL_MAJOR);
    RT_ARG_CHECK(ctx, ldu >= (u_layout == RT_COL_MAJOR ? N : nt));
  }
  if (k > 128) {
    ctx->err = "rt_trajectory_errors: k > 128";
    return RT_ERR_UNSUPPORTED;
  }
  const long step_blocks = (nt + TE_TB - 1) / TE_TB;
  // row slices: enough workgroups for four per CU where N allows, never fewer than TE_SLICE_ROWS rows each (whole stages)
  long slices = (4L * ctx->num_cus + step_blocks - 1) / step_blocks;
  const long most = (N + TE_SLICE_ROWS - 1) / TE_SLICE_ROWS;
  if (slices > most) slices = most;
  if (slices < 1) slices = 1;
  const long slice_rows = ((N + slices - 1) / slices + TE_RS - 1) / TE_RS * TE_RS;
  slices = (N + slice_rows - 1) / slice_rows;
  const long grid = step_blocks * slices * n_traj;
  if (grid >= (1L << 31)) {
    ctx->err = "rt_trajectory_errors: more than 2^31 workgroups";
    return RT_ERR_UNSUPPORTED;
  }
  const size_t part = (size_t)n_traj * slices * nt;
  void* scratch = nullptr;
  RT_TRY(rt_scratch(ctx, part * 8 * (ref ? 2 : 1), &scratch));
  const int kp = (int)((k + 3) / 4 * 4);
  TeParams p{B, A, U, static_cast<double*>(scratch), ref ? static_cast<double*>(scratch) + part : nullptr,
             (long)ldb, (long)lda, (long)stride_a, (long)ldu, (long)stride_u, (long)N, (long)nt, slice_rows,
             (int)k, kp, (int)slices, (int)step_blocks};
  const int lds = ((TE_TB + TE_RS) * (kp + 2) + 2 * 4 * 32) * 8;
  const bool colmaj = U && u_layout == RT_COL_MAJOR;
  if (colmaj) {
    RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&traj_error_kernel<true>), ((TE_TB + TE_RS) * 130 + 256) * 8));
    hipLaunchKernelGGL((traj_error_kernel<true>), dim3((unsigned)grid), dim3(TE_THREADS), lds, ctx->stream, p);
  } else {
    RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&traj_error_kernel<false>), ((TE_TB + TE_RS) * 130 + 256) * 8));
    hipLaunchKernelGGL((traj_error_kernel<false>), dim3((unsigned)grid), dim3(TE_THREADS), lds, ctx->stream, p);
  }
  RT_HIP_CHECK(ctx, hipGetLastError());
  const long total = n_traj * nt;
  hipLaunchKernelGGL(traj_error_finish_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, p.perr, p.pref,
                     err, ref, (long)nt, (int)slices, total, std::sqrt((double)N));
  RT_HIP_CHECK(ctx, hipGetLastError());
  ctx->last_grid = grid;
  ctx->last_splits = slices;
  ctx->last_tile = TE_RS * 1000 + TE_TB;
  return RT_OK;
}
