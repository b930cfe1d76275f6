// What the kernels that walk a tall basis against a block of trajectory steps share (traj_error.hip, traj_output.hip,
// interp_error.hip): the tile sizes, the load (or gather) of the 64 x k coefficient block into LDS, and the loader that
// takes 32 x k stages of the basis global -> registers -> LDS with the next stage in flight while the current one is
// multiplied.
#pragma once
#include "common.h"

namespace {

constexpr int TE_THREADS = 256;
constexpr int TE_RS = 32;                                 // rows of B per stage (two 16-row blocks)
constexpr int TE_TB = 64;                                 // steps per workgroup (four 16-step tiles)
constexpr int TE_TW = 2;                                  // step tiles per wave: wave w = row block w & 1, tiles 2 (w >> 1) ..
constexpr int TE_NL = TE_RS * (128 / 2) / TE_THREADS;     // d2 loads of a B stage per thread at k = 128
constexpr long TE_SLICE_ROWS = 1024;                      // shortest row slice

// the coefficient block, once: rows t0 .. t0 + 63 of A, columns k .. kp - 1 and steps past nt zero
// (S = kp + 2 words per LDS row, hp = kp / 2)
__device__ __forceinline__ void te_load_coefficients(double* sC, const double* A, long lda, long t0, long nt, int k, int hp,
                                                     int S, int tid) {
  const bool avec = ((lda & 1) == 0) && ((reinterpret_cast<size_t>(A) & 15) == 0);
  for (int q = tid; q < TE_TB * hp; q += TE_THREADS) {
    const int r = q / hp, c = 2 * (q - r * hp);
    d2 v{0.0, 0.0};
    if (t0 + r < nt) {
      const double* src = A + (t0 + r) * lda + c;
      if (avec && c + 1 < k) {
        v = *reinterpret_cast<const d2*>(src);
      } else {
        if (c < k) v.x = src[0];
        if (c + 1 < k) v.y = src[1];
      }
    }
    *reinterpret_cast<d2*>(&sC[r * S + c]) = v;
  }
}

// the coefficient block gathered from the data itself (interp_error.hip): word (r, c) is row idx[c] of snapshot t0 + r of
// the N x nt matrix F; columns k .. kp - 1 and snapshots past nt zero.  With every snapshot contiguous (COLMAJ) the
// threads run along c, otherwise along r, where the words of one row of F lie side by side.
template <bool COLMAJ>
__device__ __forceinline__ void te_gather_coefficients(double* sC, const double* F, long ldf, const long* idx, long t0, long nt,
                                                       int k, int kp, int S, int tid) {
  for (int q = tid; q < TE_TB * kp; q += TE_THREADS) {
    const int r = COLMAJ ? q / kp : q % TE_TB, c = COLMAJ ? q - r * kp : q / TE_TB;
    double v = 0.0;
    if (c < k && t0 + r < nt) v = COLMAJ ? F[(t0 + r) * ldf + idx[c]] : F[idx[c] * ldf + t0 + r];
    sC[r * S + c] = v;
  }
}

// B stage loader: what each thread loads, and where it goes, is the same for every stage
struct TeStageLoader {
  const double* B;
  double* sB;
  long ldb, N;
  long goff[TE_NL];
  int loff[TE_NL], code[TE_NL];                           // code: 0 nothing, 1 first word only, 2 two words, 3 one d2, 4 zeros; | row << 3
  d2 breg[TE_NL];

  __device__ __forceinline__ void init(const double* B_, long ldb_, long N_, int k, int hp, int S, double* sB_, int tid) {
    B = B_;
    sB = sB_;
    ldb = ldb_;
    N = N_;
    const bool bvec = ((ldb & 1) == 0) && ((reinterpret_cast<size_t>(B) & 15) == 0);
#pragma unroll
    for (int i = 0; i < TE_NL; ++i) {
      const int q = tid + TE_THREADS * i, r = q / hp, c = 2 * (q - r * hp);
      int m = 0;
      if (q < TE_RS * hp) m = c + 1 < k ? (bvec ? 3 : 2) : (c < k ? 1 : 4);
      code[i] = m | (r << 3);
      goff[i] = (long)r * ldb + c;
      loff[i] = r * S + c;
      breg[i] = d2{0.0, 0.0};
    }
  }
  __device__ __forceinline__ void fetch(long r0) {
    const double* base = B + r0 * ldb;
#pragma unroll
    for (int i = 0; i < TE_NL; ++i) {
      const int m = code[i] & 7;
      d2 v{0.0, 0.0};
      if (m >= 1 && m <= 3 && r0 + (code[i] >> 3) < N) {
        const double* src = base + goff[i];
        if (m == 3) {
          v = *reinterpret_cast<const d2*>(src);
        } else {
          v.x = src[0];
          if (m == 2) v.y = src[1];
        }
      }
      breg[i] = v;
    }
  }
  __device__ __forceinline__ void commit() {
#pragma unroll
    for (int i = 0; i < TE_NL; ++i)
      if (code[i] & 7) *reinterpret_cast<d2*>(&sB[loff[i]]) = breg[i];
  }
};

}  // namespace
