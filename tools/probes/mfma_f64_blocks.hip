// Probe: the two FP64 matrix instructions of gfx950 side by side.
//   (a) issue cost per SIMD of v_mfma_f64_16x16x4_f64 and v_mfma_f64_4x4x4_4b_f64: register operands, 8 independent
//       accumulator chains per wave, 4 waves per SIMD on every CU, launches of >= 5 ms, the two kernels alternated in one
//       process; reported as wall time per instruction and SIMD and as the ratio four-block / 16x16x4.
//   (b) the lane maps of A, B and D of the four-block form, found with indicator inputs: one wave per pair (la, lb) sets
//       A = 1 in lane la and B = 1 in lane lb (zero elsewhere) and records which D lanes become non-zero.  The table is
//       printed per D lane and compared with the map  A[blk][i][k]: lane = i + 4 blk + 16 k,  B[blk][k][j]: lane =
//       j + 4 blk + 16 k,  D[blk][i][j]: lane = j + 4 blk + 16 i  (the 16x16x4 maps restricted to its 4x4 diagonal blocks).
// Build: hipcc -O2 --offload-arch=gfx950 tools/probes/mfma_f64_blocks.hip -o tools/probes/mfma_f64_blocks
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <algorithm>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

typedef double d4 __attribute__((ext_vector_type(4)));
constexpr int CHAINS = 8;

__global__ __launch_bounds__(256) void rate_16x16x4(double* out, int iters, double a0, double b0) {
  d4 acc[CHAINS];
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) acc[c] = d4{0.0, 0.0, 0.0, 0.0};
  const double a = a0 + threadIdx.x, b = b0;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[c], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) s += acc[c][0] + acc[c][1] + acc[c][2] + acc[c][3];
  if (s == 12345.678) out[0] = s;  // keeps the chains alive, never true for the inputs used
}

__global__ __launch_bounds__(256) void rate_4x4x4_4b(double* out, int iters, double a0, double b0) {
  double acc[CHAINS];
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) acc[c] = 0.0;
  const double a = a0 + threadIdx.x, b = b0;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) acc[c] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, acc[c], 0, 0, 0);
  }
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) s += acc[c];
  if (s == 12345.678) out[0] = s;
}

// one wave per (la, lb): out[(la * 64 + lb) * 64 + lane] = D of that lane
__global__ __launch_bounds__(64) void lane_map(double* out) {
  const int la = blockIdx.x >> 6, lb = blockIdx.x & 63, lane = threadIdx.x;
  const double a = lane == la ? 1.0 : 0.0, b = lane == lb ? 1.0 : 0.0;
  out[(size_t)blockIdx.x * 64 + lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, 0, 0, 0);
}

// exact small integers through the map the table gave: D[blk][i][j] = sum_k A[blk][i][k] B[blk][k][j]
__global__ __launch_bounds__(64) void product_check(const double* A, const double* B, double* D) {
  const int lane = threadIdx.x;
  D[lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(A[lane], B[lane], 0.0, 0, 0, 0);
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 5;
  const int it16 = argc > 2 ? atoi(argv[2]) : 8192;     // 8192 x 8 x 4 waves x 64 cycles = 16.8 M cycles per SIMD
  const int it4 = argc > 3 ? atoi(argv[3]) : 32768;     // the same time if the four-block form costs 16 cycles
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  printf("device %s, %d CUs\n", prop.name, cus);
  double* dout;
  CK(hipMalloc(&dout, sizeof(double) * 64 * 64 * 64));

  // ---- (b) lane maps -------------------------------------------------------------------------------------------------
  hipLaunchKernelGGL(lane_map, dim3(64 * 64), dim3(64), 0, 0, dout);
  CK(hipDeviceSynchronize());
  std::vector<double> h(64 * 64 * 64);
  CK(hipMemcpy(h.data(), dout, sizeof(double) * h.size(), hipMemcpyDeviceToHost));
  printf("lane map of v_mfma_f64_4x4x4_4b_f64: D lane <- (A lane, B lane) pairs that reach it\n");
  int wrong = 0, total = 0;
  for (int ld = 0; ld < 64; ++ld) {
    printf("  D %2d <-", ld);
    for (int la = 0; la < 64; ++la)
      for (int lb = 0; lb < 64; ++lb) {
        const double v = h[((size_t)la * 64 + lb) * 64 + ld];
        const bool expect = ((la >> 2) & 3) == ((ld >> 2) & 3) && ((lb >> 2) & 3) == ((ld >> 2) & 3) && (la >> 4) == (lb >> 4) &&
                            (la & 3) == (ld >> 4) && (lb & 3) == (ld & 3);
        if (v != 0.0) { printf(" (%d,%d)%s", la, lb, v == 1.0 ? "" : "!"); ++total; }
        if ((v == 1.0) != expect || (v != 0.0 && v != 1.0)) ++wrong;
      }
    printf("\n");
  }
  printf("non-zero (la, lb, ld) triples: %d (256 expected); disagreements with the block-diagonal 16x16x4 map: %d\n", total, wrong);
  {
    // asymmetric exact integers through that map
    std::vector<double> A(64), B(64), D(64);
    for (int l = 0; l < 64; ++l) {
      const int blk = (l >> 2) & 3, x = l & 3, k = l >> 4;
      A[l] = 1 + 7 * blk + 3 * x + 11 * k;          // A[blk][i = x][k]
      B[l] = 2 + 5 * blk - 13 * x + 17 * k * k;     // B[blk][k][j = x]
    }
    double *dA, *dB, *dD;
    CK(hipMalloc(&dA, 512)); CK(hipMalloc(&dB, 512)); CK(hipMalloc(&dD, 512));
    CK(hipMemcpy(dA, A.data(), 512, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), 512, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(product_check, dim3(1), dim3(64), 0, 0, dA, dB, dD);
    CK(hipMemcpy(D.data(), dD, 512, hipMemcpyDeviceToHost));
    int bad = 0;
    for (int l = 0; l < 64; ++l) {
      const int blk = (l >> 2) & 3, j = l & 3, i = l >> 4;
      double want = 0.0;
      for (int k = 0; k < 4; ++k) want += A[i + 4 * blk + 16 * k] * B[j + 4 * blk + 16 * k];
      bad += D[l] != want;
    }
    printf("integer product through that map: %d of 64 entries differ\n", bad);
  }

  // ---- (a) issue cost ------------------------------------------------------------------------------------------------
  const int grid = cus * 4;  // 4 workgroups of 4 waves per CU: 4 waves per SIMD
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL(rate_16x16x4, dim3(grid), dim3(256), 0, 0, dout, it16, 1.0, 0.5);   // warm-up
  hipLaunchKernelGGL(rate_4x4x4_4b, dim3(grid), dim3(256), 0, 0, dout, it4, 1.0, 0.5);
  CK(hipDeviceSynchronize());
  std::vector<double> r;
  printf("issue cost: %d chains per wave, 4 waves per SIMD, %d workgroups of 256; per round ms and ns per instruction and SIMD\n", CHAINS, grid);
  for (int rd = 0; rd < rounds; ++rd) {
    float t16, t4;
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(rate_16x16x4, dim3(grid), dim3(256), 0, 0, dout, it16, 1.0, 0.5);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&t16, e0, e1));
    CK(hipEventRecord(e0, 0));
    hipLaunchKernelGGL(rate_4x4x4_4b, dim3(grid), dim3(256), 0, 0, dout, it4, 1.0, 0.5);
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&t4, e0, e1));
    const double n16 = t16 * 1e6 / ((double)it16 * CHAINS * 4), n4 = t4 * 1e6 / ((double)it4 * CHAINS * 4);
    printf("  round %d: 16x16x4 %.3f ms = %.2f ns   4x4x4_4b %.3f ms = %.2f ns   ratio %.4f\n", rd, t16, n16, t4, n4, n4 / n16);
    r.push_back(n4 / n16);
  }
  std::sort(r.begin(), r.end());
  printf("ratio four-block / 16x16x4: median %.4f, min %.4f, max %.4f (0.25 = equal flop rate, 0.5 = the CDNA3 ratio)\n",
         r[r.size() / 2], r.front(), r.back());
  return 0;
}
