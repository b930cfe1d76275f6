// Tall-skinny product  Y (N x k) = X (N x n, row-major) T (n x k),  k <= 128: the POD back-projection
// U_r = X W (pod.py:38 folded into the Gram route, SURVEY 8d "POD pass 2") and the lift u_h = V u_N.
//
// 8 N (n + k) bytes for 2 N n k flops: at k = 40 the matrix-core time is within 15 % of the HBM time, so the kernel is
// built to overlap the two as well as possible rather than for either alone: a workgroup takes 64 rows and walks the
// contraction in stages of 32 columns (256 contiguous bytes per row), X and T stages go HBM -> registers -> LDS (next
// stage in flight while the current one is multiplied), 4 waves x 16 rows, each wave all output columns; 29 KB of LDS and
// <= 128 VGPRs leave room for four workgroups per CU.
//
// Output columns: k / 16 full tiles through v_mfma_f64_16x16x4_f64, and a remainder of 1 .. 12 columns through
// v_mfma_f64_4x4x4_4b_f64, one instruction per group of four columns: its four blocks are rows 4 b .. 4 b + 3 of the
// 16-row block against the same four columns of T, its A operand is the 16x16x4 A operand lane for lane, its B operand
// one more ds_read_b64 per group and k-step.  On gfx950 the four-block form runs at the flop rate of the 16x16x4 form
// (0.164 of its time per instruction on a chip that issues nothing else, 0.25 in cycles; lane maps and rate:
// profiles/r05_mfma_f64_blocks.txt), so 8 remainder columns cost 32 matrix-core cycles per block and k-step where a
// zero-padded third tile cost 64: at k = 40 the kernel issues 5/6 of the matrix-core cycles it did, which on the POD
// pipeline's 224 CUs is what bounds it (0.84 ms of 16x16x4 cycles against a 0.74 ms HBM floor before, 0.70 ms now).
// A remainder of 13 .. 15 columns stays a zero-padded tile (four groups would cost the same).  T is staged only up to
// the next multiple of four columns; the LDS stride of a T row stays 16 ceil(k / 16).
// Measured at 1e6 x 512 -> 40 on the whole chip: 0.94 ms = 4.7 TB/s (padded third tile: 0.99 ms; generic skinny tile
// 3.8 TB/s; 64-column stages with two workgroups per CU: 3.8); in the pipeline 0.95 ms (1.04):
// profiles/r05_tallskinny_blocks_ab.txt.  A form that fed X to the MFMAs straight from registers, never through LDS,
// measured slower (1.095 vs 1.04 ms) and non-temporal loads of X / stores of Y changed nothing:
// profiles/r03_tallskinny_ab.txt.
#include "common.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_KS = 32;      // contraction columns per stage
constexpr int TS_SA = 34;      // LDS stride of the X stage ([row][k]): 2 SA == 4 (mod 8) -> the 16 rows of an
                               // A-operand read fall in distinct banks

struct TsParams {
  const double* X;
  const double* T;
  double* Y;
  long N, ldx, ldt, ldy;
  int n, k;
};

// RB = 16-row blocks per wave: a workgroup takes 64 RB rows.  With RB = 2 a T stage (re-read from L2 by every workgroup)
// serves twice as many rows: L2 -> CU traffic per row of X drops from 1.75x to 1.37x of the X bytes at k = 40.
// KF = full 16-column tiles (v_mfma_f64_16x16x4_f64), G = groups of four remainder columns (v_mfma_f64_4x4x4_4b_f64, one
// instruction per group and 16-row block: its block b is rows 4 b .. 4 b + 3 against the group's four columns).
template <int KF, int G, int RB>
__global__ __launch_bounds__(TS_THREADS, RB == 2 ? (KF + (G > 0) <= 4 ? 3 : 1) : (KF + (G > 0) <= 4 ? 4 : 2)) void tallskinny_kernel(const TsParams p) {
  constexpr int NT = KF + (G > 0);
  constexpr int TS_BM = 64 * RB;
  constexpr int TS_XL = TS_BM * TS_KS / 2 / TS_THREADS;      // d2 loads of X per thread and stage
  constexpr int KP = 16 * NT;                                 // LDS stride of a T stage row (16 mod 32 for odd NT: the
                                                              // k rows of a B-operand read fall in distinct banks)
  constexpr int KW = 16 * KF + 4 * G;                         // columns staged: k padded with zeros to the next group
  constexpr int TL = (TS_KS * KW / 2 + TS_THREADS - 1) / TS_THREADS;  // d2 loads of T per thread and stage
  constexpr int KF1 = KF > 0 ? KF : 1, G1 = G > 0 ? G : 1;    // array extents (no zero-length arrays)
  __shared__ __attribute__((aligned(16))) double sA[TS_BM * TS_SA];
  __shared__ __attribute__((aligned(16))) double sT[TS_KS * KP];
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long row0 = (long)blockIdx.x * TS_BM;
  const bool xvec = ((p.ldx & 1) == 0) && ((reinterpret_cast<size_t>(p.X) & 15) == 0);
  const bool tvec = ((p.ldt & 1) == 0) && ((reinterpret_cast<size_t>(p.T) & 15) == 0);

  d4 acc[RB][KF1];
  double accg[RB][G1];
#pragma unroll
  for (int b = 0; b < RB; ++b) {
#pragma unroll
    for (int j = 0; j < KF1; ++j) acc[b][j] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int g = 0; g < G1; ++g) accg[b][g] = 0.0;
  }

  d2 xr[TS_XL], tr[TL];
  auto fetch = [&](int c0) {  // stage of contraction columns c0 .. c0 + TS_KS - 1 into registers
#pragma unroll
    for (int i = 0; i < TS_XL; ++i) {
      const int q = tid + TS_THREADS * i, r = q / (TS_KS / 2), c = c0 + 2 * (q % (TS_KS / 2));
      const long row = row0 + r;
      d2 v{0.0, 0.0};
      if (row < p.N) {
        const double* src = p.X + row * p.ldx + c;
        if (xvec && c + 1 < p.n) {
          v = *reinterpret_cast<const d2*>(src);
        } else {
          if (c < p.n) v.x = src[0];
          if (c + 1 < p.n) v.y = src[1];
        }
      }
      xr[i] = v;
    }
#pragma unroll
    for (int i = 0; i < TL; ++i) {
      const int q = tid + TS_THREADS * i, kk = q / (KW / 2), j = 2 * (q % (KW / 2));
      d2 v{0.0, 0.0};
      if (kk < TS_KS && c0 + kk < p.n) {
        const double* src = p.T + (long)(c0 + kk) * p.ldt + j;
        if (tvec && j + 1 < p.k) {
          v = *reinterpret_cast<const d2*>(src);
        } else {
          if (j < p.k) v.x = src[0];
          if (j + 1 < p.k) v.y = src[1];
        }
      }
      tr[i] = v;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < TS_XL; ++i) {
      const int q = tid + TS_THREADS * i, r = q / (TS_KS / 2), c = 2 * (q % (TS_KS / 2));
      *reinterpret_cast<d2*>(&sA[r * TS_SA + c]) = xr[i];
    }
#pragma unroll
    for (int i = 0; i < TL; ++i) {
      const int q = tid + TS_THREADS * i, kk = q / (KW / 2), j = 2 * (q % (KW / 2));
      if (kk < TS_KS) *reinterpret_cast<d2*>(&sT[kk * KP + j]) = tr[i];
    }
  };

  fetch(0);
  commit();
  __syncthreads();
  // Operand addresses, computed once.  The four-block instruction holds A[blk][i][k] in lane i + 4 blk + 16 k, B[blk][k][j]
  // in lane j + 4 blk + 16 k and D[blk][i][j] in lane j + 4 blk + 16 i (measured: profiles/r05_mfma_f64_blocks.txt), so with
  // block blk = rows 4 blk .. 4 blk + 3 its A operand is the 16x16x4 one, register for register, and only B is read anew.
  const double* fa = sA + (16 * wid + l15) * TS_SA + l4;  // A operand: row 16 (w + 4 b) + l15, k = 4 k4 + l4
  const double* fb = sT + l4 * KP + l15;                   // B operand: k = 4 k4 + l4, column 16 j + l15
  const double* fg = sT + l4 * KP + 16 * KF + (lane & 3);  // B operand of a group: k = 4 k4 + l4, column 16 KF + 4 g + (lane & 3)
  auto multiply = [&]() {  // the stage in LDS times the accumulators
#pragma unroll
    for (int k4 = 0; k4 < TS_KS / 4; ++k4) {
      double bq[KF1], bg[G1];
#pragma unroll
      for (int j = 0; j < KF; ++j) bq[j] = fb[4 * k4 * KP + 16 * j];
#pragma unroll
      for (int g = 0; g < G; ++g) bg[g] = fg[4 * k4 * KP + 4 * g];
#pragma unroll
      for (int b = 0; b < RB; ++b) {
        const double a = fa[64 * b * TS_SA + 4 * k4];
#pragma unroll
        for (int j = 0; j < KF; ++j) acc[b][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bq[j], acc[b][j], 0, 0, 0);
#pragma unroll
        for (int g = 0; g < G; ++g) accg[b][g] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, bg[g], accg[b][g], 0, 0, 0);
      }
    }
  };
  int c0 = 0;
  // Fast loop for workgroups whose 64 rows exist and whose stages are whole (n a multiple of 32, 16-byte aligned pairs):
  // the refill addresses are a wave-uniform base, advanced by scalar adds, plus per-thread byte offsets computed once
  // - the general `fetch` spends ~10 VALU instructions per load on 64-bit address arithmetic and predicates, and an FP64
  // MFMA cannot overlap with VALU work of its SIMD (24 MFMAs per wave and stage here: the kernel was VALU-bound).
  const bool fast = xvec && tvec && (row0 + TS_BM <= p.N) && (p.n % TS_KS == 0) && ((p.k & 1) == 0) &&
                    ((long)TS_BM * p.ldx * 8 < (1L << 31)) && ((long)TS_KS * p.ldt * 8 < (1L << 31));
  if (fast) {
    const char* gx = reinterpret_cast<const char*>(p.X + row0 * p.ldx + TS_KS);   // stage 1 of this workgroup's rows
    const char* gt = reinterpret_cast<const char*>(p.T + (long)TS_KS * p.ldt);
    const unsigned xoff = (unsigned)(((long)(tid / (TS_KS / 2)) * p.ldx + 2 * (tid % (TS_KS / 2))) * 8);
    const long xstep = (long)(TS_THREADS / (TS_KS / 2)) * p.ldx * 8;               // load i: 16 i rows further down
    unsigned toff[TL];
    bool tuse[TL];
#pragma unroll
    for (int i = 0; i < TL; ++i) {
      const int q = tid + TS_THREADS * i, kk = q / (KW / 2), j = 2 * (q % (KW / 2));
      toff[i] = (unsigned)(((long)kk * p.ldt + j) * 8);
      tuse[i] = kk < TS_KS && j + 1 < p.k;                                          // padded columns stay zero
      tr[i] = d2{0.0, 0.0};
    }
    const long tstage = (long)TS_KS * p.ldt * 8;
    for (; c0 + TS_KS < p.n; c0 += TS_KS) {
#pragma unroll
      for (int i = 0; i < TS_XL; ++i) xr[i] = *reinterpret_cast<const d2*>(gx + i * xstep + xoff);
#pragma unroll
      for (int i = 0; i < TL; ++i)
        if (tuse[i]) tr[i] = *reinterpret_cast<const d2*>(gt + toff[i]);
      multiply();
      gx += TS_KS * 8;
      gt += tstage;
      __syncthreads();
      commit();
      __syncthreads();
    }
  }
  for (; c0 < p.n; c0 += TS_KS) {
    const bool more = c0 + TS_KS < p.n;
    if (more) fetch(c0 + TS_KS);
    multiply();
    __syncthreads();
    if (more) commit();
    __syncthreads();
  }
#pragma unroll
  for (int b = 0; b < RB; ++b) {
#pragma unroll
    for (int j = 0; j < KF; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const long row = row0 + 64 * b + 16 * wid + l4 + 4 * c;
        const int col = 16 * j + l15;
        if (row < p.N && col < p.k) p.Y[row * p.ldy + col] = acc[b][j][c];
      }
#pragma unroll
    for (int g = 0; g < G; ++g) {  // D[blk][i][j] of the four-block form: blk = (lane >> 2) & 3, i = lane >> 4, j = lane & 3
      const long row = row0 + 64 * b + 16 * wid + (l15 & 12) + l4;
      const int col = 16 * KF + 4 * g + (lane & 3);
      if (row < p.N && col < p.k) p.Y[row * p.ldy + col] = accg[b][g];
    }
  }
}

template <int KF, int G>
void ts_launch(int rb, unsigned grid, hipStream_t stream, const TsParams& p) {
  if constexpr (KF + (G > 0) <= 4) {
    if (rb == 2) {
      hipLaunchKernelGGL((tallskinny_kernel<KF, G, 2>), dim3(grid), dim3(TS_THREADS), 0, stream, p);
      return;
    }
  }
  hipLaunchKernelGGL((tallskinny_kernel<KF, G, 1>), dim3(grid), dim3(TS_THREADS), 0, stream, p);
}

}  // namespace

// RT_ERR_UNSUPPORTED: shape outside this kernel's range (the caller uses the generic GEMM).
int rt_tallskinny(rt_ctx* ctx, const double* X, int64_t ldx, const double* T, int64_t ldt, int64_t N, int64_t n,
                  int64_t k, double* Y, int64_t ldy) {
  if (k > 128 || n < 2 * TS_KS || N < 64L * ctx->num_cus) return RT_ERR_UNSUPPORTED;
  TsParams p{X, T, Y, (long)N, (long)ldx, (long)ldt, (long)ldy, (int)n, (int)k};
  const int nt = (int)((k + 15) / 16);
  // two 16-row blocks per wave when the 128-row workgroups still fill the chip a few times over and the accumulators fit
  const int rb = (nt <= 4 && N >= 128L * 4 * ctx->num_cus) ? 2 : 1;
  const int bm = 64 * rb;
  const unsigned grid = (unsigned)((N + bm - 1) / bm);
  RT_TRY(rt_profile_begin(ctx));
  // 1 <= k % 16 <= 12: the remainder goes through ceil((k % 16) / 4) four-block instructions; otherwise whole tiles only
  const int c = (int)(k % 16);
  const int kf = (c == 0 || c >= 13) ? nt : nt - 1, g = (c == 0 || c >= 13) ? 0 : (c + 3) / 4;
#define TS_CASE(KF_, G_) case 4 * (KF_) + (G_): ts_launch<KF_, G_>(rb, grid, ctx->stream, p); break;
#define TS_ROW(KF_) TS_CASE(KF_, 0) TS_CASE(KF_, 1) TS_CASE(KF_, 2) TS_CASE(KF_, 3)
  switch (4 * kf + g) {
    TS_CASE(0, 1) TS_CASE(0, 2) TS_CASE(0, 3)
    TS_ROW(1) TS_ROW(2) TS_ROW(3) TS_ROW(4) TS_ROW(5) TS_ROW(6) TS_ROW(7)
    default: ts_launch<8, 0>(rb, grid, ctx->stream, p); break;
  }
#undef TS_ROW
#undef TS_CASE
  RT_HIP_CHECK(ctx, hipGetLastError());
  RT_TRY(rt_profile_end(ctx));
  ctx->last_grid = grid; ctx->last_splits = 1; ctx->last_tile = bm * 1000 + 16 * nt;
  return RT_OK;
}
