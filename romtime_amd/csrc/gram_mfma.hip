// Snapshot Gram matrix G = X^T X for n >= 97 columns and long X: the dominant kernel of the POD.
//
// Differences from the generic strided GEMM (gemm_mfma.hip), all aimed at the two losses its
// profile showed (profiles/r01_v1_*: 20 % of the MFMAs spent below the diagonal, L2 hit rate 26 %):
//
//  * XCD-local K ranges.  XCD x (workgroups with blockIdx % 8 == x) owns rows [x K/8, (x+1) K/8).
//    Every workgroup of that XCD sweeps the SAME range, taking 16-row stages q, q+S, q+2S, ... of
//    it, so at any moment the 64 workgroups of an XCD read a window of a few hundred consecutive
//    rows: each 128-column panel is fetched from HBM once and re-read from that XCD's L2 by the
//    other tiles.  A workgroup that runs ahead misses in L2 and slows down, one that lags hits and
//    catches up, so the window stays together without any inter-workgroup protocol.
//  * Diagonal tiles do only the 36 MFMA tiles on/above the diagonal (of 64), 9 per wave:
//    executed/algorithmic flops 0.80 -> 0.97 at n = 512.  They run as a second launch of a
//    DIAG instantiation (72 accumulator VGPRs instead of 128, A panel only), each launch with
//    its own number of sub-splits so that it fills the chip evenly.
//  * Spare slots take the tiles' tails.  n_t tiles with s slots each rarely fill an XCD's slots (the pipeline's 56: 6
//    off-diagonal tiles x 9 = 54; 64 at n = 640: 10 x 6 = 60).  The R slots left over get workgroups of their own: every
//    regular slot stops at stage n_main of the XCD's range, and the stages behind it - the tile's tail - go whole to a
//    spare slot, which sweeps its at most ceil(n_t / R) tails one after the other into one more slab per tile
//    (gram_spare_plan()).  n_main makes a regular and a full spare slot equally long.  Short sets, where the 48-stage
//    floor and not the slot count limits s, keep the plain launch bit for bit.  Measured on the pipeline's off-diagonal
//    launch: 3.50 -> 3.39 ms (profiles/gram_spare_slots_ab.txt).
//
//  * ONE launch for long snapshot sets where the slot model says it pays (gram_choose()).  The two launches each sweep
//    all of X (8.2 GB of HBM reads at best, 13 GB measured in the pipeline).  In the one-launch form every off-diagonal
//    tile gets a workgroup slots of an XCD and every diagonal tile b, (a, b) chosen so that all slots move through the
//    XCD's K range at about one rate (gram_plan()): every panel is read from HBM once per XCD and shared through the L2
//    by all tiles that need it, at the price of slots that idle part of the time.  (A plan that balanced the slots
//    perfectly, by dealing the tail of each diagonal tile's range to off-diagonal slots as a second segment, was
//    measured and bought nothing: profiles/r03_gram_merged_ab.txt.)
//
// Output: per-(XCD, slot) 128x128 slabs, summed in a fixed order by gram_reduce_kernel
// (bitwise reproducible; exactly symmetric G).
#include <algorithm>
#include <type_traits>

#include "gemm_panel.h"

using namespace rtk;

namespace {

constexpr int BT = 128;
constexpr int GT = 512;         // threads per workgroup: 8 waves as 2 (M) x 4 (N), 64 x 32 per wave
constexpr int MAX_SLOTS = 64;   // workgroups per XCD
constexpr int MAX_TILES = 36;   // upper-triangular 128-tiles: n <= 1024
typedef unsigned u2 __attribute__((ext_vector_type(2)));
constexpr unsigned long long PACE_ONE = 1ull << 40;   // one member of an XCD's pack (high 24 bits of its word)
constexpr int PACE_DROP = 6;    // own stages behind the pack's mean beyond which a workgroup leaves the pack

struct GramParams {
  const double* X;
  long ks, ms;        // X(k, i) at X[k*ks + i*ms]
  long K, n, kx;      // rows, columns, rows per XCD range (multiple of KB)
  long last0;         // first column of the last tile row / column: (tiles1 - 1) * 128, or n - 128 (see rt_gram128)
  double* slab;       // [8][nslots][128*128]
  int nslots, tiles1, vec;
  long* counters;      // rt_ctx::dev_counters
  unsigned long long* pace;  // this launch's progress counters ([8 XCDs][16]: {stages done, workgroups started}), or nullptr
  int pace_every, pace_slack, pace_naps;   // check every so many stages; lead allowed (stages of its own); naps per check
  // Two launches: slots below n_regular take stages q, q + S, ... below n_main[x] of XCD x's range and write slab
  // slot_slab; the spare slots behind them take the tails [n_main[x], end) of slot_tn tiles from tile slot_tm on, one after
  // the other (gram_spare_plan()).  Without spare slots n_regular is the grid's slot count and n_main[x] the whole range.
  int n_regular;
  int n_main[8];
  unsigned char slot_tm[MAX_SLOTS], slot_tn[MAX_SLOTS], slot_q[MAX_SLOTS], slot_S[MAX_SLOTS], slot_slab[MAX_SLOTS];
};

// One launch (gram128_merged_kernel): the tile, stage offset and stride of every slot and the slab it writes.
// S == 0: the plan leaves the slot idle.
struct GramSegs {
  unsigned char tm[MAX_SLOTS], tn[MAX_SLOTS], q[MAX_SLOTS], S[MAX_SLOTS];
  unsigned short slab[MAX_SLOTS];
};

// MFMA-tile sets of a diagonal 128x128 tile (8x8 grid of 16x16 tiles, only i <= j: 36 tiles): waves 0-3 take five
// consecutive tiles of the row-wise list each, waves 4-7 four.  Waves w and w + 4 of a workgroup share a SIMD, so
// every SIMD issues 9 MFMAs per k-step (5,5,5,5,5,5,4,2 put 10 on two of them: 10 % of the kernel).
// The operands of each MFMA are read from LDS at run-time offsets (no register-array indexing),
// so all waves run the same instruction stream.
__device__ const unsigned char kDiagTi[8][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 1, 1}, {1, 1, 1, 1, 1}, {2, 2, 2, 2, 2}, {2, 3, 3, 3, 255}, {3, 3, 4, 4, 255}, {4, 4, 5, 5, 255}, {5, 6, 6, 7, 255}};
__device__ const unsigned char kDiagTj[8][5] = {{0, 1, 2, 3, 4}, {5, 6, 7, 1, 2}, {3, 4, 5, 6, 7}, {2, 3, 4, 5, 6}, {7, 3, 4, 5, 0}, {6, 7, 4, 5, 0}, {6, 7, 5, 6, 0}, {7, 6, 7, 7, 0}};

// Stages (16 rows each) of XCD x's K range; the last one may be partial, the last XCD's range is the shortest.
__device__ __forceinline__ int gram_range_stages(const GramParams& p, int x) {
  const long kbeg = (long)x * p.kx, kend = (kbeg + p.kx < p.K) ? kbeg + p.kx : p.K;
  return (kend > kbeg) ? (int)((kend - kbeg + KB - 1) / KB) : 0;
}

// One segment of a slot's work: the 128 x 128 tile (tm, tn) of X^T X over the stage window q0, q0 + S, ... (nstages of
// them, all inside XCD x's K range), written to `out` (a 128 x 128 slab; zeros for an empty window).  `paced`: the
// workgroup joins the XCD's pack for this segment.  All arguments are wave-uniform (SGPRs).
template <bool KC, bool DIAG>
__device__ __forceinline__ void gram_segment(const GramParams& p, double* smem, int x, int tm, int tn, int q0, int S,
                                             int nstages, bool paced, int tid, double* out) {
  using P = Panel<BT, KC, GT>;
  double* sA0 = smem;
  double* sA1 = smem + P::LDS;
  double* sB0 = smem + 2 * P::LDS;
  double* sB1 = smem + 3 * P::LDS;

  // opaque to the optimiser: nothing derived from the thread index is computed ahead of this point and kept alive (the
  // off-diagonal loop has no VGPR to spare: without the fence the column-major kernels spill 8 and 4 more bytes per lane)
  asm volatile("" : "+v"(tid));
  const long m0 = (tm == p.tiles1 - 1) ? p.last0 : (long)tm * BT, n0 = (tn == p.tiles1 - 1) ? p.last0 : (long)tn * BT;
  const long kbeg = (long)x * p.kx;
  const long kend = (kbeg + p.kx < p.K) ? kbeg + p.kx : p.K;

  const int lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 2, wn = wid & 3;
  const int l15 = lane & 15, l4 = lane >> 4;

  // Pacing (a hint for L2 reuse, never a condition for progress).  The tiles of an XCD share a panel stage through the
  // L2 only while they read it within the few microseconds it stays there, and nothing keeps workgroups together by
  // itself: unpaced, the off-diagonal launch of 1e6 x 512 fetched 10.4 GB where perfect sharing needs 4.1; paced, 4.15 GB
  // and 2 % less time (profiles/r03_gram_pace_ab.txt).  One 64-bit word per XCD holds the PACK: the sum of its members'
  // positions (stage index in the XCD's K range, low 40 bits) and their number (high 24 bits).  Every pace_every stages
  // lane 0 of wave 0 adds the workgroup's advance with one returning atomic, issued behind the stage's panel loads:
  //   - more than pace_slack of its own stages AHEAD of the pack's mean: nap ~0.45 us and look again, pace_naps times at most;
  //   - more than PACE_DROP of its own stages BEHIND (started late: its CU was busy, or it is a second batch): it leaves
  //     the pack - takes its position and itself out of the word - and runs unpaced, so the pack never waits for it.
  // Workgroups that have not started are not in the word; finished ones stay in it and look like leaders.
  unsigned long long* pace = (p.pace && paced) ? p.pace + 16 * x : nullptr;
  int pacer = (pace && __builtin_amdgcn_readfirstlane(wid) == 0 && nstages > 0) ? 1 : 0;
  int pace_pos = 0, pace_cnt = 0;
  if (pacer && lane == 0) __hip_atomic_fetch_add(pace, PACE_ONE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  constexpr int NACC = DIAG ? 5 : 8;
  d4 acc[NACC];
#pragma unroll
  for (int i = 0; i < NACC; ++i) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
  int dti[5], dtj[5];  // panel-local column offsets (x16) of this wave's diagonal MFMA tiles
  bool dval[5];
  {
    const int w = __builtin_amdgcn_readfirstlane(wid);
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      dval[q] = kDiagTi[w][q] != 255;
      dti[q] = dval[q] ? 16 * kDiagTi[w][q] : 0;
      dtj[q] = 16 * kDiagTj[w][q];
    }
  }

  d2 ra[P::NL], rb[DIAG ? 1 : P::NL];
  // interior tiles take the predicate-free loader for every stage that lies fully inside the K range
  const bool interior = p.vec && (m0 + BT <= p.n) && (n0 + BT <= p.n);
  if (nstages > 0) {
    const long k0 = kbeg + (long)q0 * KB;
    P::load(ra, p.X, p.ks, p.ms, k0, kend, m0, p.n, p.vec, tid);
    if constexpr (!DIAG) P::load(rb, p.X, p.ks, p.ms, k0, kend, n0, p.n, p.vec, tid);
    P::store(ra, sA0, tid);
    if constexpr (!DIAG) P::store(rb, sB0, tid);
  }
  __syncthreads();

  // scalar-base addressing of the refills (interior tiles): uniform pointers to the panel rows of
  // the NEXT stage, advanced by scalar adds; one per-thread byte offset for every load of the kernel
  const long k1 = kbeg + (long)(q0 + S) * KB;   // first row of stage 1
  const char* gA = reinterpret_cast<const char*>(p.X + k1 * p.ks + m0 * p.ms);
  const char* gB = reinterpret_cast<const char*>(p.X + k1 * p.ks + n0 * p.ms);
  const unsigned voff = P::lane_offset(p.ks, p.ms, tid);
  const long rows_step = P::load_step(p.ks, p.ms), stage_step = (long)S * KB * p.ks * 8;

  // stages whose 16 rows lie fully inside the K range: all of them, or all but the last (32-bit scalar compares in the loop)
  int n_full = nstages;
  if (nstages > 0 && kbeg + (long)(q0 + (nstages - 1) * S) * KB + KB > kend) n_full = nstages - 1;
  if (!interior) n_full = 0;

  auto compute = [&](const double* cA, const double* cB) {
    if constexpr (DIAG) {
#pragma unroll
      for (int k4 = 0; k4 < KB / 4; ++k4) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
          if (!dval[q]) continue;  // wave-uniform
          const double a = P::frag(cA, dti[q], k4, l15, l4);
          const double b = P::frag(cA, dtj[q], k4, l15, l4);
          acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int k4 = 0; k4 < KB / 4; ++k4) {
        double a[4], b[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = P::frag(cA, wm * 64 + i * 16, k4, l15, l4);
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = P::frag(cB, wn * 32 + j * 16, k4, l15, l4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i * 2 + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i * 2 + j], 0, 0, 0);
      }
    }
  };

  int st = 0;
  {
    // Fast loop (interior tile, either memory order): every stage here refills the other buffer from a stage that lies
    // fully inside the K range, through the scalar-base loader; unrolled by two so that the buffer parity is a
    // compile-time constant and buffer selection folds into the immediate offsets of the ds instructions.  Nothing of
    // the general (predicated) loader is live in it.
    auto fast_stage = [&](auto parity) {
      constexpr int PAR = decltype(parity)::value;
      P::load_full_u(ra, gA, voff, rows_step);
      if constexpr (!DIAG) P::load_full_u(rb, gB, voff, rows_step);
      // pacing: the advance goes in behind the panel loads and its answer (the word before the add) is back, like
      // them, by the time the stage's vmcnt wait is over - nothing waits for the L2 round trip
      const bool check = pacer && ++pace_cnt == p.pace_every;
      unsigned long long before = 0;
      if (check) {
        pace_cnt = 0;
        const int adv = S * p.pace_every;
        if (lane == 0) before = __hip_atomic_fetch_add(pace, (unsigned long long)adv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        pace_pos += adv;
      }
      __builtin_amdgcn_s_setprio(1);
      compute(PAR ? sA1 : sA0, PAR ? sB1 : sB0);
      __builtin_amdgcn_s_setprio(0);
      gA += stage_step;
      gB += stage_step;
      P::store(ra, PAR ? sA0 : sA1, tid);
      if constexpr (!DIAG) P::store(rb, PAR ? sB0 : sB1, tid);
      if (check) {
        unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)before), hi = __builtin_amdgcn_readfirstlane((unsigned)(before >> 32));
        unsigned long long word = (((unsigned long long)hi << 32) | lo) + (unsigned long long)(S * p.pace_every);
#pragma unroll 1
        for (int nap = 0;; ++nap) {
          const long long total = (long long)(word & (PACE_ONE - 1)), members = (long long)(word >> 40);
          const long long lead = (long long)pace_pos * members - total;          // (mine - mean) x members
          if (lead < -(long long)PACE_DROP * S * members) {                     // a straggler: leave the pack
            if (lane == 0)
              __hip_atomic_fetch_add(pace, 0ull - (PACE_ONE + (unsigned long long)pace_pos), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
            pacer = 0;
            break;
          }
          if (lead <= (long long)p.pace_slack * S * members || nap >= p.pace_naps) break;
          // The window is tight (a panel stage lives in the L2 for about two rounds), so the control is firm: nap
          // ~0.45 us and look again, up to pace_naps times.  Gentler rules were measured and lose the sharing:
          // two short naps per stage of excess lead without polling fetched 9 GB, a slack of 4 stages 8 GB.
          __builtin_amdgcn_s_sleep(16);
          u2 v;  // the word straight from the L2 (scalar load past the scalar cache)
          asm volatile("s_load_dwordx2 %0, %1, 0x0 glc\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(pace) : "memory");
          word = ((unsigned long long)v.y << 32) | v.x;
        }
      }
      __syncthreads();
    };
    for (; st + 2 < n_full; st += 2) {
      fast_stage(std::integral_constant<int, 0>{});
      fast_stage(std::integral_constant<int, 1>{});
    }
  }
  for (; st < nstages; ++st) {  // the remaining stages (all of them for column-major snapshots and edge tiles)
    const double* cA = (st & 1) ? sA1 : sA0;
    const double* cB = (st & 1) ? sB1 : sB0;
    const bool more = st + 1 < nstages;
    if (more) {
      const long k0 = kbeg + (long)(q0 + (st + 1) * S) * KB;
      if (st + 1 < n_full) {
        P::load_full(ra, p.X, p.ks, p.ms, k0, m0, tid);
        if constexpr (!DIAG) P::load_full(rb, p.X, p.ks, p.ms, k0, n0, tid);
      } else {
        P::load(ra, p.X, p.ks, p.ms, k0, kend, m0, p.n, p.vec, tid);
        if constexpr (!DIAG) P::load(rb, p.X, p.ks, p.ms, k0, kend, n0, p.n, p.vec, tid);
      }
    }
    __builtin_amdgcn_s_setprio(1);
    compute(cA, cB);
    __builtin_amdgcn_s_setprio(0);
    if (more) {
      P::store(ra, (st & 1) ? sA0 : sA1, tid);
      if constexpr (!DIAG) P::store(rb, (st & 1) ? sB0 : sB1, tid);
    }
    __syncthreads();
  }

  if constexpr (DIAG) {
#pragma unroll
    for (int q = 0; q < 5; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (dval[q]) out[(dti[q] + l4 + 4 * r) * BT + dtj[q] + l15] = acc[q][r];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          out[(wm * 64 + i * 16 + l4 + 4 * r) * BT + wn * 32 + j * 16 + l15] = acc[i * 2 + j][r];
  }
}

// the XCD-local K ranges rest on workgroup i running on XCD i % 8: count the ones that do not (rt_ctx_get_counter
// "gram_off_xcd"; a CU-masked stream or a driver change could break the rule, the L2 reuse would go with it)
__device__ __forceinline__ void gram_check_xcd(const GramParams& p, int x) {
  if (threadIdx.x == 0 && (int)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 15u) != x)
    atomicAdd(reinterpret_cast<unsigned long long*>(&p.counters[RT_CNT_GRAM_OFF_XCD]), 1ull);
}

// Two launches (short snapshot sets, where the plan of the merged kernel does not apply): one tile kind per launch.
// A regular slot runs one segment, a spare slot the tails of its tiles one after the other, each into that tile's tail
// slab (the slab behind its regular ones).  Spare slots are elsewhere in K and never join the pack.
// (The row-major diagonal kernel is held to the 80 VGPRs it always took: given 128, the scheduler spreads the LDS reads of
// its stage loop over 92 and the launch measured 2.4 % slower, profiles/gram_spare_slots_ab.txt.)
template <bool KC, bool DIAG>
__global__ __launch_bounds__(GT, (DIAG && !KC) ? 6 : 4) void gram128_kernel(const GramParams p) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int x = blockIdx.x & 7, slot = blockIdx.x >> 3;
  gram_check_xcd(p, x);
  // (a byte table in the kernel arguments indexed by a run-time slot is fetched with VECTOR loads: without the
  // readfirstlane every quantity derived from these - tile origin, K range, panel pointers - lives in VGPRs and
  // all the "uniform" arithmetic of the loop is VALU work, which FP64 MFMAs cannot overlap with)
  const int S = __builtin_amdgcn_readfirstlane((int)p.slot_S[slot]);
  const int n_main = p.n_main[x];
  // Both paths rebuild the thread index from the wave's number (an SGPR) and the lane's: the spare slots' loop must not
  // carry threadIdx.x, a VGPR, through a segment, and the register allocation of the regular path then is the plain
  // launch's (the workgroup is one-dimensional: wave w holds threads 64 w ... 64 w + 63 in lane order).
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (slot < p.n_regular) {
    const int lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int tm = __builtin_amdgcn_readfirstlane((int)p.slot_tm[slot]), tn = __builtin_amdgcn_readfirstlane((int)p.slot_tn[slot]),
              q0 = __builtin_amdgcn_readfirstlane((int)p.slot_q[slot]), slab = __builtin_amdgcn_readfirstlane((int)p.slot_slab[slot]);
    const int nstages = (n_main > q0) ? (n_main - q0 + S - 1) / S : 0;    // stages q0, q0+S, ... below n_main
    gram_segment<KC, DIAG>(p, smem, x, tm, tn, q0, S, nstages, true, wave * 64 + lane, p.slab + ((long)x * p.nslots + slab) * (BT * BT));
    return;
  }
  // A spare slot, in a loop of its own: the stage loops of the regular slots above stay the plain launch's.  Every
  // iteration derives its state anew from the workgroup index behind a fence, so that nothing but the counter is carried
  // through a segment (the off-diagonal stage loop has no register to spare for values hoisted out of this loop: one
  // loop around a single call for both kinds of slot spilled 16 bytes per lane in the row-major kernel).
#pragma unroll 1
  for (int i = 0;; ++i) {
    int wg = blockIdx.x, zero = 0;
    asm volatile("" : "+s"(wg), "+s"(zero));
    const int tid = wave * 64 + __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, zero));
    const int xs = wg & 7, ss = wg >> 3;
    const int Ss = __builtin_amdgcn_readfirstlane((int)p.slot_S[ss]);
    if (i >= __builtin_amdgcn_readfirstlane((int)p.slot_tn[ss])) break;
    const int r = (__builtin_amdgcn_readfirstlane((int)p.slot_tm[ss]) + i) * Ss;   // the first regular slot of the tile whose tail this is
    const int tm = __builtin_amdgcn_readfirstlane((int)p.slot_tm[r]), tn = __builtin_amdgcn_readfirstlane((int)p.slot_tn[r]),
              slab = __builtin_amdgcn_readfirstlane((int)p.slot_slab[r + Ss - 1]) + 1;
    const int first = p.n_main[xs];
    gram_segment<KC, DIAG>(p, smem, xs, tm, tn, first, 1, gram_range_stages(p, xs) - first, false, tid,
                           p.slab + ((long)xs * p.nslots + slab) * (BT * BT));
  }
}

// One launch: every slot runs the tile the plan gave it, off-diagonal or diagonal (gram_plan()).
template <bool KC>
__global__ __launch_bounds__(GT, 4) void gram128_merged_kernel(const GramParams p, const GramSegs g) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int x = blockIdx.x & 7, slot = blockIdx.x >> 3;
  gram_check_xcd(p, x);
  const int S = __builtin_amdgcn_readfirstlane((int)g.S[slot]);
  if (S == 0) return;
  const int tm = __builtin_amdgcn_readfirstlane((int)g.tm[slot]), tn = __builtin_amdgcn_readfirstlane((int)g.tn[slot]),
            q0 = __builtin_amdgcn_readfirstlane((int)g.q[slot]), slab = __builtin_amdgcn_readfirstlane((int)g.slab[slot]);
  double* out = p.slab + ((long)x * p.nslots + slab) * (BT * BT);
  const int nst_x = gram_range_stages(p, x);
  const int nstages = (nst_x > q0) ? (nst_x - q0 + S - 1) / S : 0;    // stages q0, q0+S, ...
  if (tm == tn)
    gram_segment<KC, true>(p, smem, x, tm, tn, q0, S, nstages, true, threadIdx.x, out);
  else
    gram_segment<KC, false>(p, smem, x, tm, tn, q0, S, nstages, true, threadIdx.x, out);
}

struct GramReduceParams {
  const double* slab_off;   // [8][nslots_off][128*128]
  const double* slab_diag;  // [8][nslots_diag][128*128]
  double* G;
  long n, last0;
  int nslots_off, nslots_diag, tiles1;
  unsigned char first[MAX_TILES], count[MAX_TILES];  // per upper-triangular tile, in its own launch's slots
  unsigned long long* pace;  // rt_ctx::gram_pace (256 words), zeroed here for the next Gram; or nullptr
};

// Each thread on or above the diagonal sums its element over the 8 XCD slabs x sub-splits in a fixed order (rows
// of a slab are contiguous, so the reads coalesce) and writes it to both (i, j) and (j, i): G is exactly symmetric
// and the slabs are read once (the mirrored half used to re-read them column-wise).
__global__ void gram_reduce_kernel(const GramReduceParams p) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p.pace && idx < 256) p.pace[idx] = 0ull;
  if (idx >= p.n * p.n) return;
  const long i = idx / p.n, j = idx % p.n;
  if (i > j) return;
  const int tm = (int)(i / BT), tn = (int)(j / BT);
  const int t = tm * p.tiles1 - tm * (tm - 1) / 2 + (tn - tm);
  const long off = (i - (tm == p.tiles1 - 1 ? p.last0 : (long)tm * BT)) * BT + (j - (tn == p.tiles1 - 1 ? p.last0 : (long)tn * BT));
  const double* slab = (tm == tn) ? p.slab_diag : p.slab_off;
  const int nslots = (tm == tn) ? p.nslots_diag : p.nslots_off;
  const int cnt = p.count[t];
  const double* base = slab + (long)p.first[t] * (BT * BT) + off;
  double sum = 0.0;
  for (int x = 0; x < 8; ++x) {
    const double* src = base + (long)x * nslots * (BT * BT);
#pragma unroll 4
    for (int q = 0; q < cnt; ++q) sum += src[(long)q * (BT * BT)];
  }
  p.G[idx] = sum;
  if (i != j) p.G[j * p.n + i] = sum;
}

template <bool KC, bool DIAG>
int launch_gram(rt_ctx* ctx, const GramParams& p, int grid) {
  const size_t lds = sizeof(double) * (DIAG ? 2 : 4) * Panel<BT, KC, GT>::LDS;
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&gram128_kernel<KC, DIAG>), (int)lds));
  hipLaunchKernelGGL((gram128_kernel<KC, DIAG>), dim3(grid), dim3(GT), lds, ctx->stream, p);
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

// Cost of a diagonal-tile stage relative to an off-diagonal one (36 of 64 MFMA tiles, one panel instead of two):
// measured from the two-launch kernels' rates.
constexpr double GRAM_RHO = 0.60;

// Pacing parameters (GramParams::pace_every / pace_slack / pace_naps).  Two launches (equal workgroups, only jitter to
// correct): 2 stages of slack; one launch (diagonal slots are ~1/6 faster and must be held back all the time): 1 stage.
struct GramPace {
  int every, slack, naps;
};
constexpr GramPace PACE_TWO_LAUNCHES{2, 2, 8}, PACE_ONE_LAUNCH{2, 1, 8};

// Slots per off-diagonal (a) and per diagonal tile (b) of the one-launch plan: (a, b) minimising the slowest slot's time
// per stage of the range, max(1/a, rho/b), within P slots (fewest slots among equals).  Returns that time, or 0 when
// there is no such plan.  `cap`: most slots a tile may get (short sets: at least 48 stages per workgroup).
double gram_uniform_ab(int P, int n_off, int n_d, double rho, int cap, int* a_out, int* b_out) {
  double best = 1e30;
  int best_slots = 0;
  *a_out = *b_out = 0;
  for (int a = 1; a <= cap && n_off * a + n_d <= P; ++a)
    for (int b = 1; b <= cap && n_off * a + n_d * b <= P; ++b) {
      const double T = (1.0 / a > rho / b) ? 1.0 / a : rho / b;
      const int used = n_off * a + n_d * b;
      if (T < best - 1e-12 || (T < best + 1e-12 && used < best_slots)) { best = T; *a_out = a; *b_out = b; best_slots = used; }
    }
  return *a_out ? best : 0.0;
}

// The plan of the one-launch kernel on a tiles1 x tiles1 tile grid (upper triangle): every off-diagonal tile gets s_off
// slots and every diagonal tile s_diag (gram_choose()'s a and b; at most MAX_SLOTS in all).  All slots then move through
// the K range at about one rate (s_off vs s_diag / rho stages per unit of time; pacing trims the rest), so ALL tiles of an
// XCD read a panel stage while it is in the L2: one read of X per Gram, at the price of slots that idle part of the time.
// Fills the slots (slab = slot, tile-major: off-diagonal tiles first) and the per-tile slab lists of the reduction;
// returns the number of slots in use.
int gram_plan(int tiles1, int s_off, int s_diag, GramSegs& g, unsigned char* first, unsigned char* count) {
  g = GramSegs{};
  int slot = 0;
  for (int diag = 0; diag < 2; ++diag) {
    const int S = diag ? s_diag : s_off;
    int t = 0;
    for (int a = 0; a < tiles1; ++a)
      for (int b = a; b < tiles1; ++b, ++t) {
        if ((a == b) != (diag == 1)) continue;
        first[t] = (unsigned char)slot;
        count[t] = (unsigned char)S;
        for (int q = 0; q < S; ++q, ++slot) {
          g.tm[slot] = (unsigned char)a; g.tn[slot] = (unsigned char)b;
          g.q[slot] = (unsigned char)q; g.S[slot] = (unsigned char)S;
          g.slab[slot] = (unsigned short)slot;
        }
      }
  }
  return slot;
}

// Which form the snapshot Gram takes for a K x n set on `num_cus` CUs - pure host logic, no GPU (rt_gram_plan_info lets
// the CPU-side tests check it).  form 0: not this kernel (the generic symmetric GEMM), 1: two launches (S_off / S_diag
// sub-splits per off-diagonal / diagonal tile and XCD), 2: one launch with uniform slots (a / b per tile) on a grid of
// `slots` workgroups per XCD.
struct GramChoice {
  int form, a, b, s_off, s_diag, slots;
};
GramChoice gram_choose(int num_cus, long K, long n) {
  const int slots_max = 2 * num_cus / 8;   // 2 workgroups per CU, per XCD
  GramChoice c{0, 0, 0, 0, 0, slots_max};
  const int tiles1 = (int)((n + BT - 1) / BT), ntiles = tiles1 * (tiles1 + 1) / 2, n_off = ntiles - tiles1;
  if (n < 97 || ntiles > MAX_TILES || n_off > slots_max || slots_max > MAX_SLOTS || K < 8L * 64 * KB) return c;
  const long kx = ((K + 7) / 8 + KB - 1) / KB * KB;
  // Shorter snapshot sets get fewer sub-splits, at least 48 stages each (below that the slab traffic and the two launches
  // dominate), as long as an XCD still has 16 workgroups of the bigger launch to run: 1e5 x 256 then takes 197 us instead
  // of the generic symmetric GEMM's 255, 2e5 x 128 93 instead of 286, 5e4 x 512 296 instead of 374; 3e4 x 384 (12
  // workgroups per XCD) is left to the generic kernel, which is faster there (188 vs 212 us).
  const int cap = (int)(kx / KB / 48);
  if (cap < 1) return c;
  c.s_off = n_off ? std::min(slots_max / n_off, cap) : 0;
  c.s_diag = std::min(slots_max / tiles1, cap);
  if (n_off >= 1) {
    // One launch with uniform slots reads X once (4.15 GB on 1e6 x 512 against 8.2 for two paced launches and 14.5
    // unpaced) but leaves slots idle part of the time; taken when the slot model says it costs at most 5 % more than two
    // launches (measured 1-17 % faster there: n = 256, 384, 512, 1024, profiles/r03_gram_pace_ab.txt), with at least 16
    // workgroups per XCD, and not for two-tile-column sets while the cap binds (1e5 x 256: 0.219 vs 0.209 ms).
    // n = 640 / 768 (model 1.15 / 1.07, measured 1.12 / 1.05) and the pipeline's 56 slots (1.08, measured 1.08) stay with
    // two launches.
    const double t_uni = gram_uniform_ab(slots_max, n_off, tiles1, GRAM_RHO, cap, &c.a, &c.b);
    const double t_two = (c.s_off >= 1 && c.s_diag >= 1) ? 1.0 / c.s_off + GRAM_RHO / c.s_diag : 0.0;
    if (t_uni > 0.0 && t_two > 0.0 && t_uni <= 1.05 * t_two && n_off * c.a + tiles1 * c.b >= 16 && !(tiles1 == 2 && c.a >= cap)) {
      c.form = 2;
      return c;
    }
  }
  const int busiest = n_off ? n_off * c.s_off : tiles1 * c.s_diag;
  c.form = (busiest >= 16) ? 1 : 0;
  return c;
}

// Spare slots of one launch of the two-launch form: n_t tiles of one kind with s slots each leave R = slots_max - n_t s
// slots of every XCD without a workgroup (the pipeline's 56 slots, 6 off-diagonal tiles: 9 each, 2 left over).  They take
// the TAIL of every tile's range: regular slot (t, q) keeps its stages q, q + s, ... but only below n_main, and the stages
// [n_main, end) of the tiles are dealt whole to the spare slots, at most m = ceil(n_t / R) tails each, which a spare slot
// sweeps one after the other with stride 1.  A regular slot then does n_main / s stages and a spare one m (end - n_main):
// equal at n_main = end m s / (1 + m s), taken per XCD (the last range is shorter).  Every tile gets one more slab per
// XCD for its tail, behind its s regular ones.
// Taken only when s is what the slots allow, not what `cap` allows (short sets keep the plain plan), and when the
// spare workgroup with the fewest tails still sweeps the 48 stages that `cap` asks of a workgroup; spare slots beyond one
// per tile stay unused.  Otherwise spare == 0 and the launch is the plain one: n_main is the whole range.
int gram_n_main(int nst, int m, int s) {   // round(nst m s / (1 + m s))
  const long ms = (long)m * s;
  return (int)((2 * nst * ms + 1 + ms) / (2 * (1 + ms)));
}
struct GramSpare {
  int spare, m;   // spare slots in use (0: the plain launch), most tails per spare slot
};
GramSpare gram_spare_plan(int slots_max, int n_t, int s, int cap, long kx) {
  GramSpare sp{0, 0};
  if (n_t < 1 || s < 1 || slots_max / n_t > cap) return sp;
  const int R = std::min(slots_max - n_t * s, n_t);
  if (R < 1) return sp;
  const int m = (n_t + R - 1) / R;
  const int nst = (int)(kx / KB);
  if ((long)(n_t / R) * (nst - gram_n_main(nst, m, s)) < 48) return sp;
  sp.spare = R; sp.m = m;
  return sp;
}

// Fills one launch of the two-launch form for the tiles of one kind (`diag`), in upper-triangle order: the slot tables and
// n_main of `p`, and the per-tile slab lists of the reduction (tile-major: s regular slabs, then the tail slab if the
// launch has spare slots).  Returns the workgroups per XCD; *nslabs: the slabs per XCD.
int gram_fill_launch(GramParams& p, int tiles1, bool diag, int s, const GramSpare& sp, unsigned char* first,
                     unsigned char* count, int* nslabs) {
  const int per_tile = s + (sp.spare ? 1 : 0);
  int slot = 0, n_t = 0, t = 0;
  for (int a = 0; a < tiles1; ++a)
    for (int b = a; b < tiles1; ++b, ++t) {
      if ((a == b) != diag) continue;
      first[t] = (unsigned char)(n_t * per_tile); count[t] = (unsigned char)per_tile;
      for (int q = 0; q < s; ++q, ++slot) {
        p.slot_tm[slot] = (unsigned char)a; p.slot_tn[slot] = (unsigned char)b;
        p.slot_q[slot] = (unsigned char)q; p.slot_S[slot] = (unsigned char)s;
        p.slot_slab[slot] = (unsigned char)(n_t * per_tile + q);
      }
      ++n_t;
    }
  p.n_regular = slot;
  for (int x = 0; x < 8; ++x) {
    const long kbeg = (long)x * p.kx, kend = std::min(kbeg + p.kx, p.K);
    const int nst_x = (kend > kbeg) ? (int)((kend - kbeg + KB - 1) / KB) : 0;
    p.n_main[x] = sp.spare ? gram_n_main(nst_x, sp.m, s) : nst_x;
  }
  // spare slot j: the tails of tiles [t0, t0 + cnt), the first n_t % spare slots one tail more than the others
  for (int j = 0, t0 = 0; j < sp.spare; ++j, ++slot) {
    const int cnt = n_t / sp.spare + (j < n_t % sp.spare ? 1 : 0);
    p.slot_tm[slot] = (unsigned char)t0; p.slot_tn[slot] = (unsigned char)cnt;
    p.slot_q[slot] = 0; p.slot_S[slot] = (unsigned char)s; p.slot_slab[slot] = 0;
    t0 += cnt;
  }
  *nslabs = n_t * per_tile;
  return slot;
}

template <bool KC>
int launch_gram_merged(rt_ctx* ctx, const GramParams& p, const GramSegs& g, int grid) {
  constexpr size_t lds = sizeof(double) * 4 * Panel<BT, KC, GT>::LDS;
  RT_TRY(rt_func_lds(ctx, reinterpret_cast<const void*>(&gram128_merged_kernel<KC>), (int)lds));
  hipLaunchKernelGGL((gram128_merged_kernel<KC>), dim3(grid), dim3(GT), lds, ctx->stream, p, g);
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

}  // namespace

// Returns RT_ERR_UNSUPPORTED when the shape is outside this kernel's regime (caller falls back to
// the generic symmetric GEMM).
int rt_gram128(rt_ctx* ctx, const double* X, int64_t ks, int64_t ms, int64_t K, int64_t n, double* G) {
  if (!(ks == 1 || ms == 1)) return RT_ERR_UNSUPPORTED;
  // the form depends on the shape and the CU count alone: the "gram_pace" option must not change a bit of G
  const GramChoice c = gram_choose(ctx->num_cus, (long)K, (long)n);
  if (c.form == 0) return RT_ERR_UNSUPPORTED;
  const bool one_launch = c.form == 2;
  const bool kc = (ks == 1) && (ms != 1);
  const int tiles1 = (int)((n + BT - 1) / BT), n_off = tiles1 * (tiles1 - 1) / 2;

  GramParams p;
  p.X = X; p.ks = ks; p.ms = ms; p.K = K; p.n = n;
  p.kx = ((K + 7) / 8 + KB - 1) / KB * KB;
  p.tiles1 = tiles1;
  const long other = kc ? ms : ks;
  p.vec = ((((uintptr_t)X) & 15) == 0 && (other % 2 == 0)) ? 1 : 0;
  // A last tile row / column that is not full (n no multiple of 128) would take the predicated loader for every stage:
  // 7.0 ms at n = 500 against 4.4 at n = 512.  Instead the last panel is SHIFTED to end at column n (it overlaps its
  // left neighbour; 16-byte alignment of its rows asks for an even n in row-major order): all panels are full, every tile
  // takes the fast loader, the entries computed twice are taken from the tile that owns them by the reduction.
  p.last0 = (long)(tiles1 - 1) * BT;
  if (n % BT != 0 && n >= BT && p.vec && (kc || n % 2 == 0)) p.last0 = n - BT;
  // the scalar-base loader keeps a 32-bit per-thread byte offset of up to 8 rows: beyond that, the predicated loader
  if ((!kc && (long)ks * 8 * 8 >= (1L << 31)) || (kc && (long)ms * 64 * 8 >= (1L << 31))) p.vec = 0;
  p.counters = ctx->dev_counters;
  p.pace = nullptr;
  const GramPace pace = one_launch ? PACE_ONE_LAUNCH : PACE_TWO_LAUNCHES;
  p.pace_every = pace.every; p.pace_slack = pace.slack; p.pace_naps = pace.naps;
  if (ctx->gram_pace_on) {
    if (!ctx->gram_pace) {
      RT_HIP_CHECK(ctx, hipMalloc(reinterpret_cast<void**>(&ctx->gram_pace), sizeof(unsigned long long) * 256));
      RT_HIP_CHECK(ctx, hipMemsetAsync(ctx->gram_pace, 0, sizeof(unsigned long long) * 256, ctx->stream));
    }
    p.pace = ctx->gram_pace;
  }

  GramSegs g;
  GramReduceParams rp;
  int nslots_off, nslots_diag;   // slabs per XCD of the off-diagonal / diagonal tiles; one launch: one list for both
  int wgs_off = 0, wgs_diag = 0; // two launches: workgroups per XCD of each (regular and spare slots)
  GramParams p_diag = p;
  if (one_launch) {
    nslots_off = nslots_diag = gram_plan(tiles1, c.a, c.b, g, rp.first, rp.count);
  } else {
    const int cap = (int)(p.kx / KB / 48);
    nslots_off = 0;
    if (n_off) wgs_off = gram_fill_launch(p, tiles1, false, c.s_off, gram_spare_plan(c.slots, n_off, c.s_off, cap, p.kx), rp.first, rp.count, &nslots_off);
    wgs_diag = gram_fill_launch(p_diag, tiles1, true, c.s_diag, gram_spare_plan(c.slots, tiles1, c.s_diag, cap, p.kx), rp.first, rp.count, &nslots_diag);
  }
  void* slab = nullptr;
  int rc = rt_scratch(ctx, sizeof(double) * BT * BT * 8 * (size_t)(one_launch ? nslots_off : nslots_off + nslots_diag), &slab);
  if (rc != RT_OK) return rc;
  double* slab_off = static_cast<double*>(slab);
  double* slab_diag = one_launch ? slab_off : slab_off + (size_t)8 * nslots_off * BT * BT;
  rp.slab_off = slab_off; rp.slab_diag = slab_diag; rp.G = G; rp.n = n; rp.last0 = p.last0;
  rp.nslots_off = nslots_off; rp.nslots_diag = nslots_diag; rp.tiles1 = tiles1; rp.pace = ctx->gram_pace;

  RT_TRY(rt_profile_begin(ctx, true));
  if (one_launch) {
    p.slab = slab_off; p.nslots = nslots_off;
    rc = kc ? launch_gram_merged<true>(ctx, p, g, 8 * c.slots) : launch_gram_merged<false>(ctx, p, g, 8 * c.slots);
    if (rc != RT_OK) return rc;
  } else {
    // launch 1: off-diagonal tiles
    if (n_off) {
      p.slab = slab_off; p.nslots = nslots_off;
      rc = kc ? launch_gram<true, false>(ctx, p, 8 * wgs_off) : launch_gram<false, false>(ctx, p, 8 * wgs_off);
      if (rc != RT_OK) return rc;
    }
    // launch 2: diagonal tiles (upper MFMA tiles only)
    p_diag.slab = slab_diag; p_diag.nslots = nslots_diag;
    p_diag.pace = nullptr;   // every panel has one reader here
    rc = kc ? launch_gram<true, true>(ctx, p_diag, 8 * wgs_diag) : launch_gram<false, true>(ctx, p_diag, 8 * wgs_diag);
    if (rc != RT_OK) return rc;
  }
  RT_TRY(rt_profile_end(ctx, true));
  ctx->last_grid = one_launch ? 8 * c.slots : 8 * (wgs_off + wgs_diag);
  ctx->last_splits = 8 * (one_launch ? c.a : c.s_off);
  ctx->last_tile = 128 * 1000 + 128;
  const long total = n * n;
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, rp);
  RT_HIP_CHECK(ctx, hipGetLastError());
  return RT_OK;
}

// Diagnostic / test hook: the form rt_gram would take (gram_choose) - out = {form, a, b, S_off, S_diag}.  No GPU needed.
extern "C" int rt_gram_plan_info(int num_cus, int64_t n_rows, int64_t n_cols, int* out) {
  if (!out || num_cus < 8 || n_rows < 1 || n_cols < 1) return RT_ERR_ARG;
  const GramChoice c = gram_choose(num_cus, (long)n_rows, (long)n_cols);
  out[0] = c.form; out[1] = c.a; out[2] = c.b; out[3] = c.s_off; out[4] = c.s_diag;
  return RT_OK;
}

// Diagnostic / test hook: the slot plan of one launch of the two-launch form for XCD xcd's row range (gram_spare_plan) -
// out = {tiles, regular slots per tile, spare slots in use, most tails per spare slot, n_main, stages}.  No GPU needed.
extern "C" int rt_gram_spare_plan_info(int num_cus, int64_t n_rows, int64_t n_cols, int launch, int xcd, int* out) {
  if (!out || num_cus < 8 || n_rows < 1 || n_cols < 1 || launch < 0 || launch > 1 || xcd < 0 || xcd > 7) return RT_ERR_ARG;
  const GramChoice c = gram_choose(num_cus, (long)n_rows, (long)n_cols);
  const int tiles1 = (int)((n_cols + BT - 1) / BT), n_t = launch ? tiles1 : tiles1 * (tiles1 - 1) / 2;
  if (c.form != 1 || n_t < 1) return RT_ERR_UNSUPPORTED;
  GramParams p;
  p.K = (long)n_rows;
  p.kx = ((p.K + 7) / 8 + KB - 1) / KB * KB;
  const int s = launch ? c.s_diag : c.s_off;
  const GramSpare sp = gram_spare_plan(c.slots, n_t, s, (int)(p.kx / KB / 48), p.kx);
  unsigned char first[MAX_TILES], count[MAX_TILES];
  int nslabs;
  gram_fill_launch(p, tiles1, launch == 1, s, sp, first, count, &nslabs);
  const long kbeg = (long)xcd * p.kx, kend = std::min(kbeg + p.kx, p.K);
  out[0] = n_t; out[1] = s; out[2] = sp.spare; out[3] = sp.m; out[4] = p.n_main[xcd];
  out[5] = (kend > kbeg) ? (int)((kend - kbeg + KB - 1) / KB) : 0;
  return RT_OK;
}
