// CDNA4 (gfx950) fp64 tile kernels for the dense linear-algebra taskpools.
//
//  * Grouped DGEMM / DSYRK (lower) on v_mfma_f64_16x16x4f64: ONE launch runs every
//    ready GEMM-shaped tile task of a scheduling round, so 512^2 tiles still fill
//    the 256 CUs. Two tilings: 128x128 (8 waves x 64x32, 8 accumulators per wave)
//    for big batches and 64x64 for small ones. Workgroups are remapped so a task's
//    tiles stay on one XCD (its operands stay in that XCD's 4 MiB L2).
//    Two k loops for the full, register-staged, double-buffered launches
//    (PARSEC_GEMM_MAINLOOP / gemm_mainloop()): 0 = load, multiply, store, barrier
//    per k-tile; 1 = rotated by one kk-group with the fragments double-buffered
//    in registers, so MFMAs span the k-tile barrier (default). Same results bit
//    for bit. The rotated loop has two bodies (PARSEC_GEMM_PIPELINE /
//    gemm_pipeline()): 0 = the compiler's order inside a k-tile, 1 = every
//    fragment read pinned a whole kk-group of MFMAs ahead of its use (default).
//  * MFMA operand roles are swapped (A-operand <- B tile, B-operand <- A tile) so
//    the f64 accumulator layout (col = lane&15, row = (lane>>4)+4*r, measured on
//    MI355X: profiles/probe_mfma_f64_and_vendor_baselines.log) maps lanes to
//    consecutive ROWS of the column-major C tile: 128-byte coalesced epilogues.
//  * TRSM (B := B L^-T, right/lower/trans) = blocked MFMA solve with precomputed
//    inverses of the 64x64 diagonal blocks: R_j = B_j - X_<j L_j,<j^T ; X_j = R_j invD_j^T.
//    Each workgroup owns 16 rows and keeps its row panel in LDS with a stride of 16
//    doubles, which makes every MFMA operand read bank-conflict free.
//  * POTRF of a tile: per 64-column block, ONE wave factors the diagonal block
//    (row per lane in registers, column broadcast through LDS, no block barriers)
//    and inverts it, then the panel TRSM and the lower-only GEMM update run
//    stream-ordered.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "../device/device.hpp"

namespace parsec {
namespace kern {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

constexpr int kMaxGemmBatch = 40;

struct GemmBatchArgs {
  int count;
  int prio;  // critical-path launch: raise the waves' issue priority (s_setprio)
  int claim; // critical-path launch: claim the CUs (bulk waves there pause)
  int yield; // bulk launch: pause while the CU hosts claimed critical work
  int total_tiles;
  // split-K tail: workgroups [main_tiles, grid) each take 1/ksplit of the K range
  // of one of the last (total_tiles - main_tiles) tiles and add alpha * partial
  // into C with f64 atomics (beta == 1 for every descriptor of such a launch)
  int main_tiles;
  int ksplit;
  double gate_limit;  // gated descriptors (GemmDesc::gate) skip above this estimate
  int tile_start[kMaxGemmBatch + 1];
  GemmDesc d[kMaxGemmBatch];
};
static_assert(sizeof(GemmBatchArgs) <= 4096, "GemmBatchArgs exceeds the kernel argument limit");

// Issue priority of the waves of the kernels launched by this thread right now:
// launch_kernel_batch sets it for the critical stream's batch. A critical kernel
// sharing a CU with bulk GEMM waves otherwise gets a third of the SIMD's MFMA
// pipe and waits behind their instructions (s_setprio: the SIMD arbitrates by
// priority, then age).
static thread_local int t_launch_prio = 0;
// extra dynamic LDS of the 128x128 GEMM launched by this thread right now:
// 8 KB pads a workgroup to 82 KB, so a CU holds ONE bulk GEMM workgroup and
// keeps room for a critical-path tile-POTRF step workgroup (78 KB)
static thread_local int t_launch_pad = 0;
constexpr int kBulkPadBytes = 8192;
#define PARSEC_WAVE_PRIO(p) do { if (p) __builtin_amdgcn_s_setprio(2); } while (0)
// critical-path launch of this thread: its workgroups claim their CUs
static thread_local int t_launch_claim = 0;
// bulk launch of this thread: its GEMM waves yield claimed CUs
static thread_local int t_launch_yield = 0;

// ---- Cooperative CU yield. A critical-path workgroup (tile POTRF step, the
// critical TRSM / SYRK GEMMs) counts itself into g_crit_cu[its CU] while it
// runs; a bulk GEMM workgroup on the same CU polls that count once per k-tile
// and sleeps while it is non-zero, so the critical workgroup gets the CU's MFMA
// / LDS / issue bandwidth to itself (beside bulk waves it ran 2-4x slower:
// profiles/r4_chain16_breakdown.txt). Only the CUs that host critical work
// pause; a pause is bounded (kYieldMaxPolls) so a stale count can never stall
// bulk work. One counter per CU: XCC id x (CU, SH, SE) bits of HW_ID.
__device__ int g_crit_cu[8 * 256];
__device__ __forceinline__ int cu_key() {
  // HW_REG_HW_ID (4) bits [15:8] = CU_ID, SH_ID, SE_ID; HW_REG_XCC_ID (20) bits [3:0]
  const unsigned hw = __builtin_amdgcn_s_getreg((7 << 11) | (8 << 6) | 4);
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);
  return (int)(((xcc & 7u) << 8) | (hw & 0xffu));
}
__device__ __forceinline__ void crit_claim(int on) {
  if (on && threadIdx.x == 0) __hip_atomic_fetch_add(&g_crit_cu[cu_key()], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void crit_release(int on) {
  if (!on) return;
  __syncthreads();  // every wave of the workgroup is done
  if (threadIdx.x == 0) __hip_atomic_fetch_add(&g_crit_cu[cu_key()], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// host side: the table's device address (for kernels of other translation
// units) and the engine's cu_yield mode (HipDevice init)
static std::atomic<int> g_cu_yield_mode{0};
void set_cu_yield_mode(int m) { g_cu_yield_mode.store(m); }
int cu_yield_mode() { return g_cu_yield_mode.load(std::memory_order_relaxed); }
int* crit_cu_table() {
  static int* p = [] {
    void* q = nullptr;
    if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_crit_cu)) != hipSuccess) { (void)hipGetLastError(); q = nullptr; }
    return static_cast<int*>(q);
  }();
  return p;
}
constexpr int kYieldMaxPolls = 2000;  // x ~0.1 us sleep: at most ~0.2 ms of pause per k-tile
__device__ __forceinline__ int crit_count(int key) { return __hip_atomic_load(&g_crit_cu[key], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <class Args>
__device__ __forceinline__ int find_desc(const Args& a, const int* starts, int t) {
  int lo = 0, hi = a.count - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (starts[mid] <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// XCD-aware bijective remap: blocks b, b+8, b+16... share an XCD; give each XCD a
// contiguous range of logical tiles.
__device__ __forceinline__ int xcd_remap(int b, int nwg) {
  const int nx = 8;
  int q = nwg / nx, r = nwg % nx;
  int x = b % nx, i = b / nx;
  int base = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + i;
}

// ==================================================================== GEMM
// FULL: every descriptor of the launch is a whole number of BM x BN x BK tiles
// with 16-byte aligned operands (the host checks), so the k loop carries no
// bounds checks and no divergent control flow around its loads.
// The LDS k-tiles are double-buffered (one barrier per k-tile) and staged
// through registers.
// EPI = 1: the epilogue adds alpha * acc into C with no-return f64 atomics
// performed at the memory side (beta == 1 for every descriptor of the launch):
// the accumulators start from zero (no C preload), nothing of C is read by the
// waves, and the wave does not wait for the update -- C traffic leaves the MFMA
// timeline of the workgroup. Each element gets one add per tile (or per K chunk
// of a split tile), so the result does not depend on timing.
// ML = 1 (FULL only): the rotated k loop. The k loop
// is shifted by one kk-group (4 of k) and the MFMA fragments live in two
// register sets: the fragments of group g + 1 are read while group g is
// multiplied, the last group of a k-tile is multiplied behind the k-tile
// barrier while the first group of the next k-tile is read and the global loads
// of the one after are issued. The global addresses are a uniform base advanced
// by a k-tile plus per-thread offsets fixed before the loop (no 64-bit vector
// multiply per k-tile). Split-K chunks and the a_lower / b_upper K ranges are BK
// multiples and take the same loop. ML = 0 is the loop every other launch runs.
// ML = 2: the rotated loop with a pinned schedule. The k-tile loop is unrolled
// by two, so the LDS buffer is a constant and every LDS address is one register
// per fragment plus an immediate; the k-tiles come through buffer loads with
// the tile's corner in the uniform base, so a thread keeps one 32-bit offset
// per operand (the host checks that they fit: gemm_pipeline_fits). The
// registers this frees hold a second fragment set for real: the reads of
// group g + 1 are issued in front of the MFMAs of group g
// (sched_group_barrier), the reads of the last group a whole group in front
// of the k-tile barrier, and group 0 of the next k-tile right behind it, in
// front of the held-back MFMAs. No yield poll: such launches keep ML = 1.
template <int BM, int BN, int BK, int WM, int WN, bool TRANSA, bool TRANSB, bool FULL, int EPI, int ML>
__device__ __forceinline__ void gemm_tile(const GemmBatchArgs& args, int tile, int ks, int nsplit, double (&As)[2][BK][BM + (((BM % 32) == 16) ? 0 : 16)],
                                          double (&Bs)[2][BK][BN + (((BN % 32) == 16) ? 0 : 16)]) {
  static_assert(EPI == 0 || EPI == 1, "plain or atomic epilogue");
  static_assert(ML == 0 || FULL, "rotated k loop: full tiles only");
  constexpr bool ROT = ML == 1;
  constexpr bool PIPE = ML == 2;
  constexpr int NT = WM * WN * 64;
  constexpr int WTM = BM / WM;
  constexpr int WTN = BN / WN;
  constexpr int FM = WTM / 16;
  constexpr int FN = WTN / 16;
  const int di = find_desc(args, args.tile_start, tile);
  const GemmDesc& d = args.d[di];
  const int local = tile - args.tile_start[di];
  const int mt = (d.m + BM - 1) / BM;
  const int tm = local % mt, tn = local / mt;
  const int m0 = tm * BM, n0 = tn * BN;
  if (d.lower_only && n0 > m0 + BM - 1) return;
  if (d.gate) {
    // panel solve through W = L^-1 whose condition estimate is too large: the
    // gated substitution kernel launched behind this one solves instead (the
    // estimate slots: Cin, which a gated descriptor (beta 0) never reads as C)
    const double* __restrict__ slot = d.Cin;
    if (slot[0] * slot[1] > args.gate_limit) return;
  }

  const int tid = threadIdx.x;
  const int ykey = args.yield ? cu_key() : 0;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int M = d.m, N = d.n;
  const int lda = d.lda, ldb = d.ldb;
  // K range of this workgroup (whole K unless split); chunks are BK multiples
  // op(A) lower triangular: row block m0 needs k < m0 + BM only (never split)
  int kfull = d.a_lower ? min(d.k, m0 + BM) : d.k;
  if (d.b_upper) kfull = min(kfull, n0 + BN);  // op(B) upper triangular: column block n0 reads k < n0 + BN
  const int kchunk = nsplit > 1 ? (((kfull + nsplit - 1) / nsplit + BK - 1) / BK) * BK : kfull;
  const int kbeg = ks * kchunk;
  // an empty K chunk of a split tile adds nothing. K = 0 itself (ks == 0: the
  // host keeps it out of the FULL launches, whose prologue loads k-tile 0
  // unconditionally) runs the epilogue with zero accumulators: C := beta C
  if (kbeg >= kfull && (FULL || ks > 0)) return;
  const int K = min(kfull, kbeg + kchunk) - kbeg;
  crit_claim(args.claim);
  const double* __restrict__ A = d.A + (TRANSA ? (size_t)kbeg : (size_t)kbeg * lda);
  const double* __restrict__ B = d.B + (TRANSB ? (size_t)kbeg * ldb : (size_t)kbeg);
  // 16-byte loads when every row pair is aligned and fully inside the tile
  const bool vec = FULL || ((lda | ldb) % 2 == 0) && ((((uintptr_t)A) | ((uintptr_t)B)) % 16 == 0) && (TRANSA ? (K % 2 == 0) : (M % 2 == 0)) &&
                   (TRANSB ? (N % 2 == 0) : (K % 2 == 0));

  double4_t acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};

  constexpr int A_PAIRS = BM * BK / 2 / NT;  // double2 per thread
  constexpr int B_PAIRS = BN * BK / 2 / NT;
  static_assert(A_PAIRS >= 1 && B_PAIRS >= 1, "tile too small");
  double2_t ra[A_PAIRS], rb[B_PAIRS];

  auto load_tile = [&](int k0) {
#pragma unroll
    for (int e = 0; e < A_PAIRS; ++e) {
      int idx = tid + NT * e;
      if (TRANSA) {  // A is K x M (k contiguous): op(A)(m, k) = A[k + m*lda]
        int kk = (idx % (BK / 2)) * 2, mm = idx / (BK / 2);
        int gm = m0 + mm, gk = k0 + kk;
        const double* p = A + (size_t)gm * lda + gk;
        if (FULL) ra[e] = *reinterpret_cast<const double2_t*>(p);
        else if (vec && gm < M && gk + 1 < K) ra[e] = *reinterpret_cast<const double2_t*>(p);
        else {
          ra[e].x = (gm < M && gk < K) ? p[0] : 0.0;
          ra[e].y = (gm < M && gk + 1 < K) ? p[1] : 0.0;
        }
      } else {
        int mm = (idx % (BM / 2)) * 2, kk = idx / (BM / 2);
        int gm = m0 + mm, gk = k0 + kk;
        const double* p = A + (size_t)gk * lda + gm;
        if (FULL) ra[e] = *reinterpret_cast<const double2_t*>(p);
        else if (vec && gk < K && gm + 1 < M) ra[e] = *reinterpret_cast<const double2_t*>(p);
        else {
          ra[e].x = (gm < M && gk < K) ? p[0] : 0.0;
          ra[e].y = (gm + 1 < M && gk < K) ? p[1] : 0.0;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < B_PAIRS; ++e) {
      int idx = tid + NT * e;
      if (TRANSB) {  // B is N x K (n contiguous)
        int nn = (idx % (BN / 2)) * 2, kk = idx / (BN / 2);
        int gn = n0 + nn, gk = k0 + kk;
        const double* p = B + (size_t)gk * ldb + gn;
        if (FULL) rb[e] = *reinterpret_cast<const double2_t*>(p);
        else if (vec && gk < K && gn + 1 < N) rb[e] = *reinterpret_cast<const double2_t*>(p);
        else {
          rb[e].x = (gn < N && gk < K) ? p[0] : 0.0;
          rb[e].y = (gn + 1 < N && gk < K) ? p[1] : 0.0;
        }
      } else {  // B is K x N (k contiguous)
        int kk = (idx % (BK / 2)) * 2, nn = idx / (BK / 2);
        int gn = n0 + nn, gk = k0 + kk;
        const double* p = B + (size_t)gn * ldb + gk;
        if (FULL) rb[e] = *reinterpret_cast<const double2_t*>(p);
        else if (vec && gn < N && gk + 1 < K) rb[e] = *reinterpret_cast<const double2_t*>(p);
        else {
          rb[e].x = (gn < N && gk < K) ? p[0] : 0.0;
          rb[e].y = (gn < N && gk + 1 < K) ? p[1] : 0.0;
        }
      }
    }
  };
  // Operands loaded as k-pairs (op(A) = A^T, op(B) = B): LDS holds them
  // m- / n-major with k contiguous, rows of BK + 1 doubles inside the same
  // buffer. The fragment reads (ds_read2_b64: 16-lane groups, banks mod 32)
  // of 16 consecutive rows then start 34 r mod 32 = 2 r banks apart, and the
  // two 8-byte stores of a pair (ds_write_b64, 16-lane groups) hit 2 kk + 34 m
  // mod 32: both conflict-free. The k-major layout made the stores 8-way
  // conflicts; even rows (BK + 2, one 16-byte store) still left the reads
  // 2-way (SQ_LDS_BANK_CONFLICT 40 % of the TN kernels' LDS cycles).
  constexpr int KS = BK + 1;
  // (tile shapes whose k-contiguous rows would not fit the buffer keep the k-major layout)
  constexpr bool KA = TRANSA && BM * KS <= BK * (BM + (((BM % 32) == 16) ? 0 : 16));
  constexpr bool KB = !TRANSB && BN * KS <= BK * (BN + (((BN % 32) == 16) ? 0 : 16));
  auto a_km = [&](int buf) { return &As[buf][0][0]; };
  auto b_km = [&](int buf) { return &Bs[buf][0][0]; };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int e = 0; e < A_PAIRS; ++e) {
      int idx = tid + NT * e;
      if (KA) {
        int kk = (idx % (BK / 2)) * 2, mm = idx / (BK / 2);
        a_km(buf)[mm * KS + kk] = ra[e].x;
        a_km(buf)[mm * KS + kk + 1] = ra[e].y;
      } else if (TRANSA) {
        int kk = (idx % (BK / 2)) * 2, mm = idx / (BK / 2);
        As[buf][kk][mm] = ra[e].x;
        As[buf][kk + 1][mm] = ra[e].y;
      } else {
        int mm = (idx % (BM / 2)) * 2, kk = idx / (BM / 2);
        *reinterpret_cast<double2_t*>(&As[buf][kk][mm]) = ra[e];
      }
    }
#pragma unroll
    for (int e = 0; e < B_PAIRS; ++e) {
      int idx = tid + NT * e;
      if (TRANSB) {
        int nn = (idx % (BN / 2)) * 2, kk = idx / (BN / 2);
        *reinterpret_cast<double2_t*>(&Bs[buf][kk][nn]) = rb[e];
      } else if (KB) {
        int kk = (idx % (BK / 2)) * 2, nn = idx / (BK / 2);
        b_km(buf)[nn * KS + kk] = rb[e].x;
        b_km(buf)[nn * KS + kk + 1] = rb[e].y;
      } else {
        int kk = (idx % (BK / 2)) * 2, nn = idx / (BK / 2);
        Bs[buf][kk][nn] = rb[e].x;
        Bs[buf][kk + 1][nn] = rb[e].y;
      }
    }
  };
  const int fr = lane & 15, fk = lane >> 4;
  auto mma_tile = [&](int cur) {
    if (args.yield && tid < 64) {
      // wave 0 sleeps while this CU hosts critical work; the other waves wait
      // for it at the k-tile barrier
      int polls = 0;
      while (crit_count(ykey) > 0 && polls++ < kYieldMaxPolls) __builtin_amdgcn_s_sleep(4);
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      double bfr[FM], afr[FN];
#pragma unroll
      for (int j = 0; j < FM; ++j) bfr[j] = KA ? a_km(cur)[(wm * WTM + j * 16 + fr) * KS + kk + fk] : As[cur][kk + fk][wm * WTM + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < FN; ++i) afr[i] = KB ? b_km(cur)[(wn * WTN + i * 16 + fr) * KS + kk + fk] : Bs[cur][kk + fk][wn * WTN + i * 16 + fr];
#pragma unroll
      for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  };

  const int nkt = (K + BK - 1) / BK;
  // Full tiles with |alpha| = 1: the accumulators start from (beta/alpha) C (exact),
  // loaded behind the first A/B tile so the C read latency overlaps the prologue
  // and the epilogue is a pure store (no read-modify-write tail when a batch's
  // workgroups all finish together).
  const bool split = nsplit > 1;
  const bool preload = EPI == 0 && FULL && !split && (d.alpha == 1.0 || d.alpha == -1.0);
  double* __restrict__ C = d.C;
  const int ldc = d.ldc;
  // beta's operand: C itself or a separate input (Cin)
  const double* __restrict__ Cr = d.Cin ? d.Cin : C;
  const int ldcr = d.Cin ? d.ldcin : ldc;
  // ROT: global addresses of the k loop = one uniform base per operand, advanced
  // by a k-tile per load, plus per-thread element offsets fixed here (the
  // plain loop recomputes (size_t)gk * lda per load and k-tile)
  const double* __restrict__ Ak = A;
  const double* __restrict__ Bk = B;
  size_t oa[ROT ? A_PAIRS : 1], ob[ROT ? B_PAIRS : 1];
  if constexpr (ROT) {
#pragma unroll
    for (int e = 0; e < A_PAIRS; ++e) {
      const int idx = tid + NT * e;
      if (TRANSA) oa[e] = (size_t)(m0 + idx / (BK / 2)) * lda + (idx % (BK / 2)) * 2;
      else oa[e] = (size_t)(idx / (BM / 2)) * lda + m0 + (idx % (BM / 2)) * 2;
    }
#pragma unroll
    for (int e = 0; e < B_PAIRS; ++e) {
      const int idx = tid + NT * e;
      if (TRANSB) ob[e] = (size_t)(idx / (BN / 2)) * ldb + n0 + (idx % (BN / 2)) * 2;
      else ob[e] = (size_t)(n0 + idx / (BK / 2)) * ldb + (idx % (BK / 2)) * 2;
    }
  }
  const size_t step_a = TRANSA ? (size_t)BK : (size_t)BK * lda, step_b = TRANSB ? (size_t)BK * ldb : (size_t)BK;
  // loads the next k-tile in line (tiles are taken strictly in order)
  auto load_next = [&]() {
#pragma unroll
    for (int e = 0; e < A_PAIRS; ++e) ra[e] = *reinterpret_cast<const double2_t*>(Ak + oa[ROT ? e : 0]);
#pragma unroll
    for (int e = 0; e < B_PAIRS; ++e) rb[e] = *reinterpret_cast<const double2_t*>(Bk + ob[ROT ? e : 0]);
    Ak += step_a;
    Bk += step_b;
  };
  // PIPE: k-tiles come through buffer loads. The resource's base is uniform (the
  // operand at the tile's corner, advanced by a k-tile per load); a thread adds
  // one 32-bit byte offset per operand, and its e-th pair a uniform one. Both
  // span at most BK or BM / BN columns of the operand: the host checks that this
  // stays below the 2^32 - 1 bytes the resource covers (gemm_pipeline_fits).
  const double* __restrict__ Ag = A + (TRANSA ? (size_t)m0 * lda : (size_t)m0);
  const double* __restrict__ Bg = B + (TRANSB ? (size_t)n0 : (size_t)n0 * ldb);
  static_assert(!PIPE || (NT % (BK / 2) == 0 && NT % (BM / 2) == 0 && NT % (BN / 2) == 0), "pair e of a thread lies a whole number of columns behind pair 0");
  const unsigned oa32 = ((tid / ((TRANSA ? BK : BM) / 2)) * (unsigned)lda + (tid % ((TRANSA ? BK : BM) / 2)) * 2) * 8u;
  const unsigned ob32 = ((tid / ((TRANSB ? BN : BK) / 2)) * (unsigned)ldb + (tid % ((TRANSB ? BN : BK) / 2)) * 2) * 8u;
  const unsigned ea32 = (NT / ((TRANSA ? BK : BM) / 2)) * (unsigned)lda * 8u, eb32 = (NT / ((TRANSB ? BN : BK) / 2)) * (unsigned)ldb * 8u;
  auto load_next32 = [&]() {
    // raw buffer (stride 0), 2^32 - 1 bytes, 32-bit untyped data
    const __amdgpu_buffer_rsrc_t ares = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(Ag), 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t bres = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(Bg), 0, -1, 0x00020000);
#pragma unroll
    for (int e = 0; e < A_PAIRS; ++e) ra[e] = __builtin_bit_cast(double2_t, __builtin_amdgcn_raw_buffer_load_b128(ares, oa32, e * ea32, 0));
#pragma unroll
    for (int e = 0; e < B_PAIRS; ++e) rb[e] = __builtin_bit_cast(double2_t, __builtin_amdgcn_raw_buffer_load_b128(bres, ob32, e * eb32, 0));
    Ag += step_a;
    Bg += step_b;
  };
  if constexpr (PIPE) load_next32();
  else if constexpr (ROT) load_next();
  else load_tile(0);
  if (preload && d.beta != 0.0) {
    const double cs = d.beta / d.alpha;
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        const double* p = Cr + (size_t)(n0 + wn * WTN + i * 16 + fk) * ldcr + (m0 + wm * WTM + j * 16 + fr);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = cs * p[(size_t)4 * r * ldcr];
      }
  }
  store_tile(PIPE ? (nkt & 1) : 0);  // PIPE: the last k-tile goes to buffer 1
  if constexpr (PIPE) {
    // The rotated loop below with its instruction order pinned. Per kk-group:
    // the fragment reads of the next group (into the other register set), then
    // this group's MFMAs, so every read has a whole group of the wave's own
    // MFMAs between its issue and the wait for it. The LDS store of k-tile
    // kt + 1 goes behind the reads of the last group; those reads are waited
    // for in front of the barrier, a group of MFMAs later. Behind the barrier:
    // the reads of group 0 of k-tile kt + 1, the global loads of kt + 2, then
    // the held-back MFMAs. The buffer argument of the two-buffer reasoning
    // below holds unchanged; cur, more and load are compile-time constants (the
    // k-tile loop is unrolled by two), so the steady-state body has no branch
    // but the back edge.
    constexpr int NKK = BK / 4;
    static_assert(NKK % 2 == 0, "group 0 of every k-tile lives in register set 0");
    // instructions per kk-group / k-tile: a ds_read_b64 per fragment (below); a
    // staged pair is one ds_write (b128 or write2_b64) and one buffer load
    constexpr int NRD = FM + FN;
    constexpr int NWR = A_PAIRS + B_PAIRS;
    constexpr int NLD = A_PAIRS + B_PAIRS;
    constexpr int SG_MFMA = 0x8, SG_VMEM_READ = 0x20, SG_DS_READ = 0x100, SG_DS_WRITE = 0x200;
    double bfr[2][FM], afr[2][FN];
    // One LDS address register per fragment, everything else (buffer, kk-group)
    // in the 16-bit immediate of a ds_read_b64. Left to itself the compiler
    // pairs fragments 16 rows apart into ds_read2_b64, whose 8-bit offsets do
    // not reach the next kk-group, and keeps a base register per buffer and
    // group (16 in all) live across the loop; an index it cannot see through
    // keeps the reads single.
    constexpr int LDA_S = BM + (((BM % 32) == 16) ? 0 : 16), LDB_S = BN + (((BN % 32) == 16) ? 0 : 16);
    int ia[FM], ib[FN];
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      ia[j] = KA ? (wm * WTM + j * 16 + fr) * KS + fk : fk * LDA_S + wm * WTM + j * 16 + fr;
      asm("" : "+v"(ia[j]));
    }
#pragma unroll
    for (int i = 0; i < FN; ++i) {
      ib[i] = KB ? (wn * WTN + i * 16 + fr) * KS + fk : fk * LDB_S + wn * WTN + i * 16 + fr;
      asm("" : "+v"(ib[i]));
    }
    auto read_frag = [&](int buf, int kk, double* bf, double* af) {
      // af first: the group's first MFMAs take af[0] with every bf
#pragma unroll
      for (int i = 0; i < FN; ++i) af[i] = b_km(0)[ib[i] + buf * BK * LDB_S + (KB ? kk : kk * LDB_S)];
#pragma unroll
      for (int j = 0; j < FM; ++j) bf[j] = a_km(0)[ia[j] + buf * BK * LDA_S + (KA ? kk : kk * LDA_S)];
    };
    __syncthreads();
    read_frag(nkt & 1, 0, bfr[0], afr[0]);
    if (1 < nkt) load_next32();
    auto k_tile = [&](auto cur_c, auto more_c, auto load_c) {
      constexpr int cur = decltype(cur_c)::value;
      constexpr bool more = decltype(more_c)::value, load = decltype(load_c)::value;
#pragma unroll
      for (int g = 0; g < NKK; ++g) {
        if (g + 1 < NKK) {
          read_frag(cur, (g + 1) * 4, bfr[(g + 1) & 1], afr[(g + 1) & 1]);
          if (g == NKK - 2 && more) store_tile(cur ^ 1);  // k-tile kt + 1, loaded a k-tile ago
        } else if (more) {
          // the one fence of a k-tile: nothing moves across the barrier
          __builtin_amdgcn_sched_barrier(0);
          __syncthreads();
          read_frag(cur ^ 1, 0, bfr[0], afr[0]);
          if (load) load_next32();
        }
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[g & 1][i], bfr[g & 1][j], acc[i][j], 0, 0, 0);
        if (g + 1 < NKK) {
          __builtin_amdgcn_sched_group_barrier(SG_DS_READ, NRD, 0);
          if (g == NKK - 2 && more) __builtin_amdgcn_sched_group_barrier(SG_DS_WRITE, NWR, 0);
          __builtin_amdgcn_sched_group_barrier(SG_MFMA, FN * FM, 0);
        } else if (more) {
          __builtin_amdgcn_sched_group_barrier(SG_DS_READ, NRD, 0);
          if (load) __builtin_amdgcn_sched_group_barrier(SG_VMEM_READ, NLD, 0);
          __builtin_amdgcn_sched_group_barrier(SG_MFMA, FN * FM, 0);
        }
      }
    };
    constexpr std::integral_constant<int, 0> c0{};
    constexpr std::integral_constant<int, 1> c1{};
    constexpr std::true_type yes{};
    constexpr std::false_type no{};
    // k-tiles to go; the last one lies in buffer 1 (the prologue chose the
    // first buffer by the parity of nkt), so one tail serves both parities: an
    // odd count peels its first k-tile instead. nkt >= 1, as in the loop
    // below (the last k_tile runs unconditionally): FULL launches have k > 0,
    // an empty split-K chunk returned above, and the a_lower / b_upper ranges
    // hold at least one tile
    int left = nkt;
    if ((left & 1) && left > 1) {
      k_tile(c1, yes, yes);
      --left;
    }
    for (; left > 2; left -= 2) {
      k_tile(c0, yes, yes);
      k_tile(c1, yes, yes);
    }
    if (left == 2) k_tile(c0, yes, no);
    k_tile(c1, no, no);
  } else if constexpr (ROT) {
    // Rotated k loop. The fragments of kk-group g + 1 are read into the other
    // register set while group g is multiplied, and the rotation crosses the
    // k-tile boundary: the last group of k-tile kt is multiplied BEHIND the
    // barrier, from registers, while the wave reads group 0 of k-tile kt + 1 and
    // issues the global loads of k-tile kt + 2 -- the MFMA pipe keeps work over
    // the store / barrier / load-issue / first-read sequence that every wave of
    // the workgroup runs at the same moment. Each accumulator still takes its
    // MFMAs in ascending k order, so the results are those of the loop below bit
    // for bit.
    // Two LDS buffers suffice: (1) every read of buffer cur in k-tile kt (groups
    // 1 .. NKK - 1; group 0 was read behind the previous barrier) is issued and
    // waited for before the barrier of kt (__syncthreads drains lgkmcnt), and
    // the next writes to cur (k-tile kt + 2) come behind that barrier; (2) the
    // writes of k-tile kt + 1 to cur ^ 1 come behind the barrier of kt - 1, after
    // which nobody reads cur ^ 1 (its last reads were k-tile kt - 1's, before that
    // barrier), and complete before the barrier of kt; its first reads (kt + 1,
    // group 0) come behind it. ra / rb are free for the loads of kt + 2 because
    // the store of kt + 1 precedes the barrier.
    constexpr int NKK = BK / 4;
    static_assert(NKK % 2 == 0, "group 0 of every k-tile lives in register set 0");
    double bfr[2][FM], afr[2][FN];
    auto read_frag = [&](int buf, int kk, double* bf, double* af) {
#pragma unroll
      for (int j = 0; j < FM; ++j) bf[j] = KA ? a_km(buf)[(wm * WTM + j * 16 + fr) * KS + kk + fk] : As[buf][kk + fk][wm * WTM + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < FN; ++i) af[i] = KB ? b_km(buf)[(wn * WTN + i * 16 + fr) * KS + kk + fk] : Bs[buf][kk + fk][wn * WTN + i * 16 + fr];
    };
    __syncthreads();
    read_frag(0, 0, bfr[0], afr[0]);
    if (1 < nkt) load_next();
    // one k-tile; more: k-tile kt + 1 exists (store it, barrier, read its group
    // 0), load: k-tile kt + 2 exists (issue its global loads). Both are constants
    // at the three call sites, so the steady-state body is straight-line code and
    // the compiler's wait counts are exact (a branch that skips the store or the
    // read makes it wait for every LDS operation at the join, i.e. for the fresh
    // reads in front of the held-back MFMAs).
    auto k_tile = [&](int cur, bool more, bool load) {
      if (args.yield && tid < 64) {
        // wave 0 sleeps while this CU hosts critical work; the other waves wait
        // for it at the k-tile barrier
        int polls = 0;
        while (crit_count(ykey) > 0 && polls++ < kYieldMaxPolls) __builtin_amdgcn_s_sleep(4);
      }
#pragma unroll
      for (int g = 0; g < NKK; ++g) {
        if (g + 1 < NKK) {
          if (g == NKK - 2 && more) store_tile(cur ^ 1);  // k-tile kt + 1, loaded a k-tile ago
          read_frag(cur, (g + 1) * 4, bfr[(g + 1) & 1], afr[(g + 1) & 1]);
        } else if (more) {
          // only the last group is held back: without this fence the compiler also
          // moves group NKK - 2 behind the barrier (a third fragment set: 128 VGPRs
          // and spills in sibling instantiations) and leaves the store and the reads
          // in front of it with no MFMA of this wave to cover their latency. Inside
          // the two regions the compiler's own order stays: a fence around every
          // group (reads strictly in front of the MFMAs that cover them) measured
          // +3.0 .. 3.9 % over the plain loop where this form gives +5.1 .. 5.6 %
          // (profiles/gemm_rotated_mainloop.txt)
          __builtin_amdgcn_sched_barrier(0);
          __syncthreads();
          read_frag(cur ^ 1, 0, bfr[0], afr[0]);
          if (load) load_next();
        }
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FM; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[g & 1][i], bfr[g & 1][j], acc[i][j], 0, 0, 0);
      }
    };
    int kt = 0;
    for (; kt + 2 < nkt; ++kt) k_tile(kt & 1, true, true);
    if (kt + 1 < nkt) {
      k_tile(kt & 1, true, false);
      ++kt;
    }
    k_tile(kt & 1, false, false);
  } else {
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int cur = kt & 1;
      if (kt + 1 < nkt) load_tile((kt + 1) * BK);
      mma_tile(cur);
      if (kt + 1 < nkt) store_tile(cur ^ 1);
      __syncthreads();
    }
  }

  const double alpha = d.alpha, beta = preload ? 0.0 : d.beta;
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int gm = m0 + wm * WTM + j * 16 + fr;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gn = n0 + wn * WTN + i * 16 + fk + 4 * r;
        if ((FULL || (gm < M && gn < N)) && (!d.lower_only || gm >= gn)) {
          double* p = C + (size_t)gn * ldc + gm;
          double v = alpha * acc[i][j][r];
          if (split || EPI == 1) {
            unsafeAtomicAdd(p, v);  // no-return global f64 add, performed at the memory side
            continue;
          }
          if (beta != 0.0) v += beta * Cr[(size_t)gn * ldcr + gm];
          *p = v;
          if (d.C2) d.C2[(size_t)gn * d.ldc2 + gm] -= v;
        }
      }
    }
  crit_release(args.claim);
}

template <int BM, int BN, int BK, int WM, int WN, bool TRANSA, bool TRANSB, bool FULL, int EPI = 0, int ML = 0>
__global__ __launch_bounds__(WM * WN * 64) __attribute__((amdgpu_waves_per_eu(WM * WN / 2))) void dgemm_batch_kernel(const GemmBatchArgs args) {
  constexpr int PADM = ((BM % 32) == 16) ? 0 : 16;
  constexpr int PADN = ((BN % 32) == 16) ? 0 : 16;
  __shared__ __attribute__((aligned(16))) double As[2][BK][BM + PADM];
  __shared__ __attribute__((aligned(16))) double Bs[2][BK][BN + PADN];
  PARSEC_WAVE_PRIO(args.prio);
  // Workgroups [0, main_tiles) own whole tiles (XCD-aware order); the ones
  // dispatched last split the K range of the tail tiles (wave quantisation:
  // a 606-tile launch on 512 slots would otherwise run a 94-tile second round)
  int tile, ks = 0, nsplit = 1;
  if ((int)blockIdx.x < args.main_tiles) {
    tile = xcd_remap(blockIdx.x, args.main_tiles);
  } else {
    const int u = blockIdx.x - args.main_tiles;
    nsplit = args.ksplit;
    tile = args.main_tiles + u / nsplit;
    ks = u % nsplit;
  }
  if (tile >= args.total_tiles) return;
  gemm_tile<BM, BN, BK, WM, WN, TRANSA, TRANSB, FULL, EPI, ML>(args, tile, ks, nsplit, As, Bs);
}

// ========================================================= diag blocks (4 waves)
// Factor the w x w (w <= 64) lower block at T (ldt) in place and/or write its
// inverse (64 x 64 col-major, identity padded) to invD. 256 threads; lane r of
// wave v owns row r of columns 16v..16v+15 in registers. Blocked by 16-column
// panels so the serial chain never leaves a wave:
//   * panel p is factored entirely inside wave p: pivots and column entries are
//     broadcast with v_readlane (no LDS round trip, no barrier), 1/sqrt is a
//     hardware rsq refined by two Newton steps (no IEEE divide on the chain);
//   * the panel goes to LDS (double-buffered, one barrier per panel) and waves
//     v > p apply the rank-16 update to their columns.
// The inverse is blocked the same way: each wave inverts its 16x16 diagonal
// block, then wave j walks down its block column X_ij = -X_ii sum_k L_ik X_kj.
__device__ __forceinline__ double readlane_d(double x, int lane) {
  const long long b = __builtin_bit_cast(long long, x);
  const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), lane);
  const int hi = __builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
}

__device__ __forceinline__ double rsqrt_nr(double d) {
  double y = __builtin_amdgcn_rsq(d);
  const double h = 0.5 * d;
  y = y * __builtin_fma(-h * y, y, 1.5);
  y = y * __builtin_fma(-h * y, y, 1.5);
  return y;
}

// kUpper (inverse only, factor == false): T is upper triangular; its transpose
// is inverted with the same code and the result is written back transposed, so
// invD holds T^-1 (upper). T's strict lower triangle is never read.
// kUnit (inverse only): T's diagonal is taken as 1 and never read.
template <bool kUpper = false, bool kUnit = false>
__device__ __forceinline__ void block_potrf64(double* T, int ldt, int w, double* invD, int* info, int info_base, bool factor) {
  __shared__ double Ls[64][65];      // Ls[c][r] = L(r, c)
  __shared__ double Xs[64][65];      // Xs[c][r] = X(r, c), X = L^-1
  // The panel broadcast buffers (factor phase) and the per-wave scratch of the
  // inverse phase share one LDS array: the kernel then fits (83 KB) next to a
  // resident 128x128 GEMM workgroup (74 KB), so the critical-path factorization
  // is not held back until a CU drains completely.
  __shared__ double PnTs[2 * 16 * 65];
  double(*Pn)[16][65] = reinterpret_cast<double(*)[16][65]>(PnTs);  // panel broadcast buffers
  double(*Ts)[16][17] = reinterpret_cast<double(*)[16][17]>(PnTs);  // per-wave scratch for the inverse
  __shared__ double dinv[64];
  __shared__ int bad_s;
  const int r = threadIdx.x & 63;
  const int v = threadIdx.x >> 6;
  double a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = 16 * v + i;
    if (kUpper)
      a[i] = (r < w && c < w && !(kUnit && r == c)) ? (r >= c ? T[(size_t)r * ldt + c] : 0.0) : (r == c ? 1.0 : 0.0);
    else
      a[i] = (r < w && c < w && !(kUnit && r == c)) ? T[(size_t)c * ldt + r] : (r == c ? 1.0 : 0.0);
  }
  if (threadIdx.x == 0) bad_s = 0x7fffffff;
  __syncthreads();
  if (factor) {
#pragma unroll 1
    for (int p = 0; p < 4; ++p) {
      double* pn = &Pn[p & 1][0][0];
      if (v == p) {
        int bad = 0x7fffffff;
#pragma unroll
        for (int jj = 0; jj < 16; ++jj) {
          const int j = 16 * p + jj;
          double d = readlane_d(a[jj], j);
          if (d <= 0.0 && j < w && bad == 0x7fffffff) bad = j + 1;
          d = d <= 0.0 ? 1.0 : d;
          const double rs = rsqrt_nr(d);
          const double lv = (r == j) ? d * rs : (r > j ? a[jj] * rs : 0.0);
          a[jj] = lv;
          if (r == j) dinv[j] = rs;
#pragma unroll
          for (int i = jj + 1; i < 16; ++i) a[i] -= lv * readlane_d(lv, 16 * p + i);
        }
        if (r == 0 && bad != 0x7fffffff) atomicMin(&bad_s, bad);
#pragma unroll
        for (int i = 0; i < 16; ++i) pn[i * 65 + r] = a[i];
      }
      __syncthreads();
      if (v > p) {
        double lr[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) lr[t] = pn[t * 65 + r];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          double s = 0.0;
#pragma unroll
          for (int t = 0; t < 16; ++t) s = __builtin_fma(lr[t], pn[t * 65 + 16 * v + i], s);
          a[i] -= s;
        }
      }
    }
    __syncthreads();
    if (threadIdx.x == 0 && bad_s != 0x7fffffff && info) atomicCAS(info, 0, info_base + bad_s);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int c = 16 * v + i;
      if (r < w && c < w && r >= c) T[(size_t)c * ldt + r] = a[i];
    }
  }
  if (!invD) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = 16 * v + i;
    Ls[c][r] = (r >= c) ? a[i] : 0.0;
    Xs[c][r] = 0.0;
    if (!factor && r == c) dinv[c] = 1.0 / a[i];
  }
  __syncthreads();
  // (1) wave v inverts its 16x16 diagonal block; lane c < 16 owns column c
  const int b0 = 16 * v;
  if (r < 16) {
    double x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      double s = (i == r) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) s = __builtin_fma(-Ls[b0 + k][b0 + i], x[k], s);
      x[i] = s * dinv[b0 + i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) Xs[b0 + r][b0 + i] = x[i];
  }
  __syncthreads();
  // (2) wave j computes block column j below the diagonal, top to bottom
  {
    const int j = v;
    const int c = r & 15, rg = r >> 4;  // lane -> column c, rows rg + 4q
#pragma unroll 1
    for (int i = j + 1; i < 4; ++i) {
      double tq[4] = {0.0, 0.0, 0.0, 0.0};
      for (int k = j; k < i; ++k) {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const double xv = Xs[16 * j + c][16 * k + t];
#pragma unroll
          for (int q = 0; q < 4; ++q) tq[q] = __builtin_fma(Ls[16 * k + t][16 * i + rg + 4 * q], xv, tq[q]);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) Ts[j][rg + 4 * q][c] = tq[q];
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): scratch visible to the wave
      double oq[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const double tv = Ts[j][t][c];
#pragma unroll
        for (int q = 0; q < 4; ++q) oq[q] = __builtin_fma(-Xs[16 * i + t][16 * i + rg + 4 * q], tv, oq[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) Xs[16 * j + c][16 * i + rg + 4 * q] = oq[q];
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_s_waitcnt(0xc07f);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = 16 * v + k;
    if (kUpper)
      invD[(size_t)r * 64 + c] = Xs[c][r];
    else
      invD[(size_t)c * 64 + r] = Xs[c][r];
  }
}

constexpr int kDiagThreads = 256;

__global__ __launch_bounds__(kDiagThreads) void dpotrf_diag_inv_kernel(double* A, int lda, int j, int jb, double* invD, int* info) {
  block_potrf64(A + (size_t)j * lda + j, lda, jb, invD, info, j, true);
}

// Inverses of the 64x64 diagonal blocks of L (n x n): block b -> invD + b*4096.
__global__ __launch_bounds__(kDiagThreads) void dtrtri_diag_kernel(const double* L, int ldl, int n, double* invD) {
  const int b = blockIdx.x;
  const int c0 = b * 64;
  block_potrf64(const_cast<double*>(L) + (size_t)c0 * ldl + c0, ldl, min(64, n - c0), invD + (size_t)b * 4096, nullptr, 0, false);
}

// The same for U (n x n upper): block b of invD is the (upper) inverse of U's block b.
__global__ __launch_bounds__(kDiagThreads) void dtrtri_diag_upper_kernel(const double* U, int ldu, int n, double* invD) {
  const int b = blockIdx.x;
  const int c0 = b * 64;
  block_potrf64<true>(const_cast<double*>(U) + (size_t)c0 * ldu + c0, ldu, min(64, n - c0), invD + (size_t)b * 4096, nullptr, 0, false);
}

// The unit-diagonal variants: the diagonal of L / U is taken as 1 and never read
// (the L of an LU factor shares its tile with U, whose diagonal sits there).
__global__ __launch_bounds__(kDiagThreads) void dtrtri_diag_unit_kernel(const double* L, int ldl, int n, double* invD) {
  const int b = blockIdx.x;
  const int c0 = b * 64;
  block_potrf64<false, true>(const_cast<double*>(L) + (size_t)c0 * ldl + c0, ldl, min(64, n - c0), invD + (size_t)b * 4096, nullptr, 0, false);
}
__global__ __launch_bounds__(kDiagThreads) void dtrtri_diag_upper_unit_kernel(const double* U, int ldu, int n, double* invD) {
  const int b = blockIdx.x;
  const int c0 = b * 64;
  block_potrf64<true, true>(const_cast<double*>(U) + (size_t)c0 * ldu + c0, ldu, min(64, n - c0), invD + (size_t)b * 4096, nullptr, 0, false);
}

// ==================================================================== TRSM
constexpr int kMaxTrsmBatch = 48;
struct TrsmInvArgs {
  int count;
  int prio;
  double gate_limit;  // gated descriptors (TrsmDesc::gate) run only above this estimate
  int block_start[kMaxTrsmBatch + 1];
  TrsmDesc d[kMaxTrsmBatch];
  const double* invD[kMaxTrsmBatch];
};
static_assert(sizeof(TrsmInvArgs) <= 4096, "TrsmInvArgs exceeds the kernel argument limit");

// B := B L^-T by 64-column blocks: R_j = B_j - X_<j L_j,<j^T, X_j = R_j invD_j^T.
// A workgroup owns BR = 16 rows of B (its row panel lives in LDS, stride 16:
// conflict-free MFMA operand reads). 8 waves: wave (g, h) computes columns
// 16g..16g+15 of the block over half h of the reduction, with four independent
// MFMA accumulator chains; the two halves are summed through LDS.
// kGlobal: the row panel stays in B itself (solved in place, 8 KB of LDS for the
// reduction only), so the launch fits on a CU beside a resident bulk GEMM
// workgroup: the gated fallback of the auto panel solve, whose workgroups nearly
// always return at once (the 139 KB LDS version waited for whole CUs at
// nb = 1024: 6.3 ms per launch on the critical stream, profiles/r4_kernel_stats_final.txt).
// Needs n % 64 == 0. Waves of a workgroup share the CU's L1, so the in-place
// writes of one block are visible to the next block's reads after the barrier.
constexpr int kTrsmThreads = 512;
template <int BR, bool kGlobal>
__global__ __launch_bounds__(kTrsmThreads) void dtrsm_inv_kernel(const TrsmInvArgs args) {
  static_assert(BR == 16, "MFMA operand layout assumes 16-row panels");
  extern __shared__ double P[];  // [ncols_padded][BR], then red[16][64] (kGlobal: red only)
  PARSEC_WAVE_PRIO(args.prio);
  const int b = blockIdx.x;
  const int di = find_desc(args, args.block_start, b);
  const TrsmDesc& d = args.d[di];
  const double* __restrict__ invD = args.invD[di];
  // invD: contiguous 64x64 blocks, or the diagonal 64-blocks of W = L^-1 (ld invD_ld)
  const size_t ldD = d.invD_ld ? (size_t)d.invD_ld : 64;
  const size_t bstride = d.invD_ld ? (size_t)64 * d.invD_ld + 64 : 4096;
  if (d.gate) {
    const double* __restrict__ slot = d.gate_slot;
    if (!(slot[0] * slot[1] > args.gate_limit)) return;  // the W-GEMM solved this panel
  }
  const bool packed = d.packed != 0;  // L(i, k) = d.L(k, i) for i > k (packed panel tile)
  const int r0 = (b - args.block_start[di]) * BR;
  const int n = d.n, m = d.m;
  const int nblk = (n + 63) / 64;
  double* red = kGlobal ? P : P + nblk * 64 * BR;
  double* Bp = d.B;
  const size_t ldb = d.ldb;
  // element (row rr of the panel, column c)
  auto pget = [&](int c, int rr) -> double {
    if (kGlobal) return r0 + rr < m ? Bp[(size_t)c * ldb + r0 + rr] : 0.0;
    return P[c * BR + rr];
  };
  auto pset = [&](int c, int rr, double v) {
    if (kGlobal) {
      if (r0 + rr < m) Bp[(size_t)c * ldb + r0 + rr] = v;
    } else {
      P[c * BR + rr] = v;
    }
  };
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = wv & 3, h = wv >> 2;
  const int fr = lane & 15, fk = lane >> 4;
  const double* __restrict__ L = d.L;
  const size_t ldl = d.ldl;
  if (!kGlobal) {
    for (int idx = tid; idx < nblk * 64 * BR; idx += kTrsmThreads) {
      int c = idx / BR, rr = idx % BR;
      P[idx] = (c < n && r0 + rr < m) ? Bp[(size_t)c * ldb + r0 + rr] : 0.0;
    }
    __syncthreads();
  }
  for (int jb = 0; jb < nblk; ++jb) {
    const int c0 = jb * 64;
    const int cw = c0 + 16 * g + fr;  // L row this lane feeds as the MFMA A-operand
    const bool valid = cw < n;
    const double* __restrict__ Lp = packed ? L + (size_t)(valid ? cw : 0) * ldl : L + (valid ? cw : 0);
    const size_t lstride = packed ? 1 : ldl;
    double4_t acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = (double4_t){0.0, 0.0, 0.0, 0.0};
    const int kh = c0 / 2;  // multiple of 32
    const int kbeg = h * kh, kend = kbeg + kh;
    for (int k = kbeg; k < kend; k += 16) {
      double av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        av[u] = valid ? Lp[(size_t)(k + 4 * u + fk) * lstride] : 0.0;
        bv[u] = pget(k + 4 * u + fk, fr);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc[u], 0, 0, 0);
    }
    double4_t s = acc[0] + acc[1] + acc[2] + acc[3];
    if (h == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[(g * 4 + q) * 64 + lane] = s[q];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * g + fk + 4 * q;
        pset(c, fr, pget(c, fr) - (s[q] + red[(g * 4 + q) * 64 + lane]));
      }
    }
    __syncthreads();
    // X_j = R_j invD_j^T, reduction over kk split between the two halves
    double4_t t0 = (double4_t){0.0, 0.0, 0.0, 0.0}, t1 = t0;
    const double* __restrict__ Dj = invD + (size_t)jb * bstride + 16 * g + fr;
#pragma unroll
    for (int kk = 32 * h; kk < 32 * h + 32; kk += 8) {
      const double a0 = Dj[(kk + fk) * ldD], a1 = Dj[(kk + 4 + fk) * ldD];
      const double b0 = pget(c0 + kk + fk, fr), b1 = pget(c0 + kk + 4 + fk, fr);
      t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, t1, 0, 0, 0);
    }
    double4_t t = t0 + t1;
    if (h == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[(g * 4 + q) * 64 + lane] = t[q];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * g + fk + 4 * q;
        pset(c, fr, t[q] + red[(g * 4 + q) * 64 + lane]);
      }
    }
    __syncthreads();
  }
  if (!kGlobal) {
    for (int idx = tid; idx < n * BR; idx += kTrsmThreads) {
      int c = idx / BR, rr = idx % BR;
      if (r0 + rr < m) Bp[(size_t)c * ldb + r0 + rr] = P[idx];
    }
  }
}

// ======================================================== TRSM (left side)
constexpr int kMaxTrsmLeftBatch = 64;
struct TrsmLeftArgs {
  int count;
  int prio;
  int block_start[kMaxTrsmLeftBatch + 1];
  TrsmLeftDesc d[kMaxTrsmLeftBatch];  // invD always set (the launcher fills it in)
};
static_assert(sizeof(TrsmLeftArgs) <= 4096, "TrsmLeftArgs exceeds the kernel argument limit");

// B := alpha op(L)^-1 B by 64-row blocks, the scheme of dtrsm_inv_kernel turned
// on its side. Forward (trans 0): R_j = B_j - L_j,<j X_<j, X_j = invD_j R_j;
// backward (trans 1, j descending): R_j = B_j - L_>j,j^T X_>j, X_j = invD_j^T R_j.
// A workgroup owns 16 columns of B for the whole sweep: the strip lives in LDS
// as [row][16] (stride 16: conflict-free MFMA B-operand reads), its rows padded
// with zeros to a multiple of 64, so the MFMA loops carry no masks: a lane whose
// L row / column lies past n reads the last valid one instead (finite data times
// the zero padding, or a result row that is written back as zero). 8 waves: wave
// (g, h) computes rows 16g..16g+15 of the block over half h of the reduction.
// kUpper: L is upper triangular (U). op(U) = U couples block j with the blocks
// below it, so trans 0 is the backward sweep and trans 1 (U^T, lower) the forward
// one; the element op(U)(i, k) sits where op(L)(i, k) does, so only the
// direction and the side that needs the clamp differ. Either way every element
// read lies in the named triangle.
// TrsmLeftDesc::right: B is nrhs x n and X op(L) = alpha B, i.e. op(L)^T X^T =
// alpha B^T: the same sweep with the transpose flipped on the strip of B^T. A
// workgroup then owns 16 ROWS of B, LDS element [i][jj] is B[i * ldb + j0 + jj]
// (128 contiguous bytes per column of B); only the two strip loops differ.
// TrsmLeftDesc::unit is the launcher's business alone: the kernel reads diagonal
// blocks only through invD.
template <bool kUpper>
__global__ __launch_bounds__(kTrsmThreads) void dtrsm_left_kernel(const TrsmLeftArgs args) {
  extern __shared__ double P[];  // [rows padded][16], then red[16][64]
  PARSEC_WAVE_PRIO(args.prio);
  const int b = blockIdx.x;
  const int di = find_desc(args, args.block_start, b);
  const TrsmLeftDesc& d = args.d[di];
  const int j0 = (b - args.block_start[di]) * 16;
  const int n = d.n, nrhs = d.nrhs;
  const int nblk = (n + 63) / 64;
  const int np = nblk * 64;
  double* red = P + np * 16;
  const bool right = d.right != 0;
  const bool tr = (d.trans != 0) != right;
  const double alpha = d.alpha;
  double* Bp = d.B;
  const size_t ldb = d.ldb;
  const double* __restrict__ L = d.L;
  const size_t ldl = d.ldl;
  const double* __restrict__ invD = d.invD;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int g = wv & 3, h = wv >> 2;
  const int fr = lane & 15, fk = lane >> 4;
  if (!right) {
    for (int idx = tid; idx < np * 16; idx += kTrsmThreads) {
      const int i = idx >> 4, jj = idx & 15;
      P[idx] = (i < n && j0 + jj < nrhs && alpha != 0.0) ? alpha * Bp[(size_t)(j0 + jj) * ldb + i] : 0.0;
    }
  } else {
    for (int idx = tid; idx < np * 16; idx += kTrsmThreads) {
      const int i = idx >> 4, jj = idx & 15;
      P[idx] = (i < n && j0 + jj < nrhs && alpha != 0.0) ? alpha * Bp[(size_t)i * ldb + j0 + jj] : 0.0;
    }
  }
  __syncthreads();
  const bool down = kUpper ? !tr : tr;  // backward sweep: blocks bottom up
  for (int s = 0; s < nblk; ++s) {
    const int jb = down ? nblk - 1 - s : s;
    const int c0 = jb * 64;
    const int cw = min(c0 + 16 * g + fr, n - 1);  // row (op N) / column (op T) of L this lane feeds as the MFMA A-operand
    double4_t acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = (double4_t){0.0, 0.0, 0.0, 0.0};
    // the reduction runs over the solved blocks: above (forward) or below (backward)
    const int kh = (down ? np - c0 - 64 : c0) / 2;  // multiple of 32
    const int kbeg = (down ? c0 + 64 : 0) + h * kh, kend = kbeg + kh;
    if (!tr) {
      const double* __restrict__ Lp = L + cw;
      for (int k = kbeg; k < kend; k += 16) {
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kk = k + 4 * u + fk;
          av[u] = Lp[(size_t)(kUpper ? min(kk, n - 1) : kk) * ldl];  // upper: columns >= n meet the strip's zero padding
          bv[u] = P[kk * 16 + fr];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc[u], 0, 0, 0);
      }
    } else {
      const double* __restrict__ Lp = L + (size_t)cw * ldl;
      for (int k = kbeg; k < kend; k += 16) {
        double av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int kk = k + 4 * u + fk;
          av[u] = Lp[kUpper ? kk : min(kk, n - 1)];  // lower: rows >= n meet the strip's zero padding
          bv[u] = P[kk * 16 + fr];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc[u], 0, 0, 0);
      }
    }
    double4_t sum = acc[0] + acc[1] + acc[2] + acc[3];
    if (h == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[(g * 4 + q) * 64 + lane] = sum[q];
    }
    __syncthreads();
    if (h == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * g + fk + 4 * q;
        P[c * 16 + fr] = c < n ? P[c * 16 + fr] - (sum[q] + red[(g * 4 + q) * 64 + lane]) : 0.0;
      }
    }
    __syncthreads();
    // X_j = op(invD_j) R_j, reduction over kk split between the two halves
    double4_t t0 = (double4_t){0.0, 0.0, 0.0, 0.0}, t1 = t0;
    const double* __restrict__ Dj = invD + (size_t)jb * 4096 + (tr ? (16 * g + fr) * 64 : 16 * g + fr);
    const int dk = tr ? 1 : 64;
#pragma unroll
    for (int kk = 32 * h; kk < 32 * h + 32; kk += 8) {
      const double a0 = Dj[(kk + fk) * dk], a1 = Dj[(kk + 4 + fk) * dk];
      const double b0 = P[(c0 + kk + fk) * 16 + fr], b1 = P[(c0 + kk + 4 + fk) * 16 + fr];
      t0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, t0, 0, 0, 0);
      t1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, t1, 0, 0, 0);
    }
    double4_t t = t0 + t1;
    if (h == 1) {
#pragma unroll
      for (int q = 0; q < 4; ++q) red[(g * 4 + q) * 64 + lane] = t[q];
    }
    __syncthreads();  // every wave has read R_j
    if (h == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * g + fk + 4 * q;
        P[c * 16 + fr] = c < n ? t[q] + red[(g * 4 + q) * 64 + lane] : 0.0;
      }
    }
    __syncthreads();
  }
  if (!right) {
    for (int idx = tid; idx < n * 16; idx += kTrsmThreads) {
      const int i = idx >> 4, jj = idx & 15;
      if (j0 + jj < nrhs) Bp[(size_t)(j0 + jj) * ldb + i] = P[idx];
    }
  } else {
    for (int idx = tid; idx < n * 16; idx += kTrsmThreads) {
      const int i = idx >> 4, jj = idx & 15;
      if (j0 + jj < nrhs) Bp[(size_t)i * ldb + j0 + jj] = P[idx];
    }
  }
}

// ================================================================ launchers
// Every knob of the grouped-GEMM dispatch: read from the environment once
// (gemm_policy_init, no device needed), changed afterwards by the setters below.
struct GemmPolicy {
  int tile = 0;          // PARSEC_GEMM_TILE: 0 auto, 64, 128
  int full = 1;          // PARSEC_GEMM_FULL=0 disables the unchecked fast path
  int big_tiles = 384;   // PARSEC_GEMM_BIG_TILES: 128x128 tiles in a launch to pick the big kernel
  int splitk = 1;        // PARSEC_GEMM_SPLITK=0 disables the split-K tail of the 128x128 kernel (tests/test_headline_gpu.py, profiles/r2_bench_ab_fill_splitk.log)
  int mainloop = 1;      // PARSEC_GEMM_MAINLOOP: k loop of the full launches, 0 plain, 1 rotated (profiles/gemm_rotated_mainloop.txt, tests/test_gemm_mainloop_gpu.py)
  int pipeline = 1;      // PARSEC_GEMM_PIPELINE: body of the rotated k loop, 0 compiler-scheduled, 1 pinned (gemm_tile ML = 2; profiles/gemm_pipelined_mainloop.txt, tests/test_gemm_pipeline_gpu.py)
  int chunk_fill = 1;    // PARSEC_GEMM_CHUNK_FILL=0: fixed 40-descriptor launches
  int slots = 0;         // PARSEC_GEMM_SLOTS: resident 128x128 workgroups, one round of the big kernel; 0 = two per CU of the device
  // PARSEC_GEMM_EPI: the atomic epilogue 1 always, 0 never, -1 when every
  // descriptor has K >= 1024: 40 x 1024^3 61.6 -> 63.9 TF, 16 x 1024^3 57.9 ->
  // 58.9 TF, but 32 x 512^3 51.3 -> 47.5 TF (half the flops per memory-side
  // add) -- profiles/r5_gemm_epilogue.txt
  int epi = -1;
  bool pad_test = false;   // PARSEC_GEMM_PAD_TEST=1: parsec_amd_dgemm_batch launches like a DPOTRF bulk stream
  bool pad_debug = false;  // PARSEC_GEMM_PAD_DEBUG: say so once when a padded launch goes out
};
static GemmPolicy gemm_policy_init() {
  GemmPolicy p;
  auto num = [](const char* name, int& v) {
    if (const char* e = getenv(name)) v = atoi(e);
  };
  num("PARSEC_GEMM_TILE", p.tile);
  num("PARSEC_GEMM_FULL", p.full);
  num("PARSEC_GEMM_BIG_TILES", p.big_tiles);
  num("PARSEC_GEMM_SPLITK", p.splitk);
  num("PARSEC_GEMM_MAINLOOP", p.mainloop);
  num("PARSEC_GEMM_PIPELINE", p.pipeline);
  num("PARSEC_GEMM_CHUNK_FILL", p.chunk_fill);
  num("PARSEC_GEMM_SLOTS", p.slots);
  num("PARSEC_GEMM_EPI", p.epi);
  p.mainloop = p.mainloop != 0;
  p.pipeline = p.pipeline != 0;
  if (getenv("PARSEC_GEMM_SLOTS")) p.slots = std::max(1, p.slots);
  if (p.epi != 0 && p.epi != 1) p.epi = -1;
  int pad_test = 0;
  num("PARSEC_GEMM_PAD_TEST", pad_test);
  p.pad_test = pad_test != 0;
  p.pad_debug = getenv("PARSEC_GEMM_PAD_DEBUG") != nullptr;
  return p;
}
static GemmPolicy& gemm_policy() {
  static GemmPolicy p = gemm_policy_init();
  return p;
}
// resident 128x128 workgroups of the launch being issued: half when bulk
// launches are padded to one workgroup per CU (t_launch_pad)
static int gemm_slots() {
  static const int device_slots = [] {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) return 2 * ncu;
    return 512;
  }();
  const int slots = gemm_policy().slots > 0 ? gemm_policy().slots : device_slots;
  return t_launch_pad ? std::max(1, slots / 2) : slots;
}

// The pinned body addresses an operand as a uniform base plus a 32-bit
// per-thread byte offset that spans the columns of the stored operand a k-tile
// touches: BK of A (BM when A is transposed), BN of B (BK when B is transposed).
int gemm_pipeline_fits(int bm, int bn, int bk, int transA, int transB, long long lda, long long ldb) {
  const unsigned long long span_a = (unsigned long long)(transA ? bm : bk) * (unsigned long long)lda * sizeof(double);
  const unsigned long long span_b = (unsigned long long)(transB ? bk : bn) * (unsigned long long)ldb * sizeof(double);
  // strictly below 2^32: the buffer resource of the loads covers 2^32 - 1 bytes
  return span_a < (1ull << 32) && span_b < (1ull << 32);
}

// launch record of this thread (gemm_launch_log): a ring of the last launches
static thread_local bool t_gemm_log_on = false;
static thread_local GemmLaunchRecord t_gemm_log[kGemmLaunchLogSize];
static thread_local unsigned t_gemm_log_count = 0;  // records written since the last reset

// ---- Decide. What launch_gemm_batch issues for a descriptor list is computed
// here on the host alone, from the descriptors and an explicit environment; no
// pointer is dereferenced and no device is asked.
struct GemmPlanEnv {
  GemmPolicy policy;
  int slots;      // resident 128x128 workgroups of one round (already halved for a padded launch)
  int pad_bytes;  // extra dynamic LDS of a 128x128 launch (one bulk workgroup per CU)
  bool yield;     // bulk launch: the waves poll their CU's claim count
  bool claim;     // critical launch: the workgroups claim their CUs
};
// one launch: its record and its descriptors, [first, first + rec.descs) of the regrouped list
struct GemmLaunch {
  GemmLaunchRecord rec;
  int first;
};

// Descriptors per launch (<= kMaxGemmBatch, the kernel-argument limit): the cut
// that fills whole rounds of resident 128x128 workgroups best. 40 tiles of
// 512^2 are 640 128-tiles = 1.25 rounds of 512 slots (62 % of the second round
// idle); 32 of them are exactly one round.
template <class Tiles128>  // tiles128(i): 128 x 128 tiles of descriptor i
static int gemm_chunk_cut(Tiles128 tiles128, int n, int slots, bool fill_rounds) {
  const int cap = std::min(n, kMaxGemmBatch);
  if (!fill_rounds) return cap;
  int best = cap, tiles = 0;
  double best_fill = -1.0;
  for (int c = 1; c <= cap; ++c) {
    tiles += tiles128(c - 1);
    if (tiles < slots) continue;
    const int rounds = (tiles + slots - 1) / slots;
    const double fill = (double)tiles / ((double)rounds * slots);
    if (fill >= best_fill - 1e-9) { best_fill = fill; best = c; }  // ties: the larger cut
  }
  return best_fill >= 0.0 ? best : cap;
}
int gemm_chunk_plan(const int* m, const int* n, int count, int slots, int* out) {
  int cuts = 0;
  for (int s = 0; s < count;) {
    const int c = gemm_chunk_cut([&](int i) { return ((m[s + i] + 127) / 128) * ((n[s + i] + 127) / 128); }, count - s, std::max(1, slots),
                                 gemm_policy().chunk_fill != 0);
    out[cuts++] = c;
    s += c;
  }
  return cuts;
}

// One launch of n descriptors of one operand mode: tile shape, kernel, grid.
static GemmLaunchRecord gemm_plan_launch(const GemmDesc* descs, int n, const GemmPlanEnv& env) {
  const GemmPolicy& p = env.policy;
  GemmLaunchRecord r{};
  int t128 = 0;
  bool big = true;
  for (int i = 0; i < n; ++i) {
    t128 += ((descs[i].m + 127) / 128) * ((descs[i].n + 127) / 128);
    if (descs[i].m < 128 || descs[i].n < 128) big = false;
  }
  // 128x128: 8 waves (2 x 4) of 64x32, 126 VGPRs -> 4 waves per SIMD with two
  // workgroups per CU (profiles/r1_gemm_variants_v8.log); 64x64: 4 waves of 32x32
  const bool use_big = p.tile == 128 || (p.tile == 0 && big && t128 >= p.big_tiles);
  const int BM = use_big ? 128 : 64, BN = BM, BK = 16;
  r.bm = BM; r.bn = BN;
  r.descs = n;
  r.transA = descs[0].transA != 0; r.transB = descs[0].transB != 0;
  r.pad_bytes = use_big ? env.pad_bytes : 0;
  int total = 0;
  bool full = p.full != 0;
  for (int i = 0; i < n; ++i) {
    const GemmDesc& g = descs[i];
    full = full && g.m % BM == 0 && g.n % BN == 0 && g.k > 0 && g.k % BK == 0 && (g.lda | g.ldb) % 2 == 0 &&
           ((uintptr_t)g.A | (uintptr_t)g.B) % 16 == 0;
    total += ((g.m + BM - 1) / BM) * ((g.n + BN - 1) / BN);
  }
  r.total_tiles = r.main_tiles = r.grid = total;
  r.ksplit = 1;
  const int slots = env.slots;
  if (use_big && p.splitk != 0 && total > slots) {
    // the last partial round of workgroups: split its tiles' K range so it
    // finishes in 1/s of a tile time; needs beta == 1 (partials are added into C)
    // and >= 256 of K per chunk (fewer flops per added byte would be bound by
    // the chip's f64 atomic rate)
    const int tail = total % slots;
    int kmin = 1 << 30;
    bool ok = tail > 0 && 2 * tail <= slots;
    for (int i = 0; ok && i < n; ++i) {
      ok = descs[i].beta == 1.0 && !descs[i].a_lower && !descs[i].b_upper && !descs[i].Cin && !descs[i].C2;
      kmin = std::min(kmin, descs[i].k);
    }
    const int s = ok ? std::min({slots / std::max(tail, 1), kmin / 256, 8}) : 1;
    if (s >= 2) {
      r.main_tiles = total - tail;
      r.ksplit = s;
      r.grid = r.main_tiles + tail * s;
    }
  }
  // atomic epilogue: every descriptor accumulates into C (beta 1, no separate Cin / C2)
  bool epi = p.epi != 0 && full;
  for (int i = 0; epi && i < n; ++i) epi = descs[i].beta == 1.0 && !descs[i].Cin && !descs[i].C2 && (p.epi > 0 || descs[i].k >= 1024);
  // rotated k loop (gemm_tile ML = 1) for the full launches
  const bool rot = full && p.mainloop == 1;
  // its pinned body (ML = 2): no yield poll or CU claim, 32-bit per-thread operand offsets
  bool pipe = rot && p.pipeline == 1 && !env.yield && !env.claim;
  for (int i = 0; pipe && i < n; ++i) pipe = gemm_pipeline_fits(BM, BN, BK, descs[i].transA, descs[i].transB, descs[i].lda, descs[i].ldb) != 0;
  r.full = full; r.epilogue = epi ? 1 : 0;
  r.rotated = rot; r.pipelined = pipe;
  return r;
}

// Group descriptors by (transA, transB): one grouped launch per combination
// (the vendor library is an A/B reference only: scripts/kbench_gemm_vs_vendor.py).
// A descriptor with alpha == 0 or k <= 0 references neither A nor B (BLAS): it
// goes out as K = 0 in a launch of its own kind, C := beta C from the
// bounds-checked kernel's epilogue, so NaN / Inf in the operands stay out of C
// and the k loops carry no test for it. (Gated descriptors are a protocol of
// the panel solve and stay where they are.) `sorted` receives the descriptors
// in launch order; a chunk without tiles launches nothing and has no record.
static std::vector<GemmLaunch> gemm_plan(const GemmDesc* descs, int n, const GemmPlanEnv& env, std::vector<GemmDesc>& sorted) {
  std::vector<GemmDesc> g[5];
  for (int i = 0; i < n; ++i) {
    const GemmDesc& d = descs[i];
    if ((d.alpha == 0.0 || d.k <= 0) && !d.gate) {
      GemmDesc z = d;
      z.k = 0;
      z.transA = z.transB = 0;
      z.a_lower = z.b_upper = 0;
      g[4].push_back(z);
    } else {
      g[(d.transA ? 2 : 0) | (d.transB ? 1 : 0)].push_back(d);
    }
  }
  std::vector<GemmLaunch> plan;
  sorted.clear();
  for (const auto& v : g) {
    for (size_t s = 0; s < v.size();) {
      const GemmDesc* d = v.data() + s;
      const int c = gemm_chunk_cut([d](int i) { return ((d[i].m + 127) / 128) * ((d[i].n + 127) / 128); }, (int)(v.size() - s), env.slots,
                                   env.policy.chunk_fill != 0);
      const GemmLaunchRecord r = gemm_plan_launch(d, c, env);
      if (r.total_tiles > 0) plan.push_back({r, (int)sorted.size()});
      sorted.insert(sorted.end(), d, d + c);
      s += (size_t)c;
    }
  }
  return plan;
}
int gemm_launch_plan(const GemmDesc* descs, int n, int slots, bool one_per_cu, bool bulk_yield, int claim, GemmLaunchRecord* out) {
  std::vector<GemmDesc> sorted;
  const GemmPlanEnv env{gemm_policy(), std::max(1, one_per_cu ? slots / 2 : slots), one_per_cu ? kBulkPadBytes : 0, bulk_yield, claim >= 2};
  const std::vector<GemmLaunch> plan = gemm_plan(descs, n, env, sorted);
  for (size_t i = 0; i < plan.size(); ++i) out[i] = plan[i].rec;
  return (int)plan.size();
}

// ---- Launch.
// the seven kernels of one tile shape and operand mode: the checked one, and
// the full one with each loop body (ML 0 plain, 1 rotated, 2 pinned) and epilogue
template <int BM, int BN, int BK, int WM, int WN, bool TA, bool TB>
static void launch_gemm_kernel(const GemmLaunchRecord& r, const GemmBatchArgs& a, hipStream_t stream) {
  const dim3 grid(r.grid), block(WM * WN * 64);
  const size_t pad = (size_t)r.pad_bytes;
  const int ml = r.pipelined ? 2 : r.rotated ? 1 : 0;
  switch (r.full ? 1 + 2 * ml + r.epilogue : 0) {
    case 0: hipLaunchKernelGGL((dgemm_batch_kernel<BM, BN, BK, WM, WN, TA, TB, false, 0, 0>), grid, block, pad, stream, a); break;
    case 1: hipLaunchKernelGGL((dgemm_batch_kernel<BM, BN, BK, WM, WN, TA, TB, true, 0, 0>), grid, block, pad, stream, a); break;
    case 2: hipLaunchKernelGGL((dgemm_batch_kernel<BM, BN, BK, WM, WN, TA, TB, true, 1, 0>), grid, block, pad, stream, a); break;
    case 3: hipLaunchKernelGGL((dgemm_batch_kernel<BM, BN, BK, WM, WN, TA, TB, true, 0, 1>), grid, block, pad, stream, a); break;
    case 4: hipLaunchKernelGGL((dgemm_batch_kernel<BM, BN, BK, WM, WN, TA, TB, true, 1, 1>), grid, block, pad, stream, a); break;
    case 5: hipLaunchKernelGGL((dgemm_batch_kernel<BM, BN, BK, WM, WN, TA, TB, true, 0, 2>), grid, block, pad, stream, a); break;
    default: hipLaunchKernelGGL((dgemm_batch_kernel<BM, BN, BK, WM, WN, TA, TB, true, 1, 2>), grid, block, pad, stream, a); break;
  }
}
template <int BM, int BN, int BK, int WM, int WN>
static void launch_gemm_shape(const GemmLaunchRecord& r, const GemmBatchArgs& a, hipStream_t stream) {
  switch ((r.transA ? 2 : 0) | (r.transB ? 1 : 0)) {
    case 0: launch_gemm_kernel<BM, BN, BK, WM, WN, false, false>(r, a, stream); break;
    case 1: launch_gemm_kernel<BM, BN, BK, WM, WN, false, true>(r, a, stream); break;
    case 2: launch_gemm_kernel<BM, BN, BK, WM, WN, true, false>(r, a, stream); break;
    default: launch_gemm_kernel<BM, BN, BK, WM, WN, true, true>(r, a, stream); break;
  }
}

// Issues the plan: every launch is driven by its record, and the record is
// what the launch log keeps.
void launch_gemm_batch(const GemmDesc* descs, int n, hipStream_t stream) {
  const GemmPlanEnv env{gemm_policy(), gemm_slots(), t_launch_pad, t_launch_yield != 0, t_launch_claim >= 2};
  std::vector<GemmDesc> sorted;
  for (const GemmLaunch& l : gemm_plan(descs, n, env, sorted)) {
    const GemmLaunchRecord& r = l.rec;
    GemmBatchArgs a;
    a.count = r.descs;
    a.prio = t_launch_prio;
    a.claim = env.claim;
    a.yield = env.yield;
    a.total_tiles = r.total_tiles;
    a.main_tiles = r.main_tiles;
    a.ksplit = r.ksplit;
    a.gate_limit = parsec::trsm_inverse_limit();
    int total = 0;
    for (int i = 0; i < r.descs; ++i) {
      const GemmDesc& g = sorted[l.first + i];
      a.d[i] = g;
      a.tile_start[i] = total;
      total += ((g.m + r.bm - 1) / r.bm) * ((g.n + r.bn - 1) / r.bn);
    }
    a.tile_start[r.descs] = total;
    if (r.pad_bytes && env.policy.pad_debug) {
      static bool said = false;
      if (!said) {
        said = true;
        std::fprintf(stderr, "[gemm] bulk 128x128 launch with %d extra LDS bytes (one workgroup per CU)\n", r.pad_bytes);
      }
    }
    if (t_gemm_log_on) t_gemm_log[t_gemm_log_count++ % kGemmLaunchLogSize] = r;
    if (r.bm == 128) launch_gemm_shape<128, 128, 16, 2, 4>(r, a, stream);
    else launch_gemm_shape<64, 64, 16, 2, 2>(r, a, stream);
  }
}

// Split-K tail of the 128x128 kernel on (1) / off (0), < 0 queries; returns the previous setting.
int gemm_splitk(int on) {
  const int prev = gemm_policy().splitk;
  if (on >= 0) gemm_policy().splitk = on;
  return prev;
}

// k loop of the full register-staged GEMM launches: 0 plain, 1 rotated, < 0 queries; returns the previous setting.
int gemm_mainloop(int mode) {
  const int prev = gemm_policy().mainloop;
  if (mode >= 0) gemm_policy().mainloop = mode == 0 ? 0 : 1;
  return prev;
}

// Body of the rotated k loop (consulted only when gemm_mainloop is 1): 0 compiler-scheduled, 1 pinned, < 0 queries; returns the previous setting.
int gemm_pipeline(int mode) {
  const int prev = gemm_policy().pipeline;
  if (mode >= 0) gemm_policy().pipeline = mode == 0 ? 0 : 1;
  return prev;
}

// Round-filling launch chunks on (1) / off (0), < 0 queries; returns the previous setting.
int gemm_chunk_fill(int on) {
  const int prev = gemm_policy().chunk_fill;
  if (on >= 0) gemm_policy().chunk_fill = on != 0;
  return prev;
}

int gemm_launch_log(int on) {
  const int prev = t_gemm_log_on;
  if (on >= 0) t_gemm_log_on = on != 0;
  return prev;
}

int gemm_launch_log_read(GemmLaunchRecord* out, bool reset) {
  const unsigned have = std::min<unsigned>(t_gemm_log_count, kGemmLaunchLogSize);
  for (unsigned i = 0; i < have; ++i) out[i] = t_gemm_log[(t_gemm_log_count - have + i) % kGemmLaunchLogSize];
  if (reset) t_gemm_log_count = 0;
  return (int)have;
}

// Tile-size policy of the grouped GEMM (0 = auto, 64, 128); returns the previous one.
int gemm_tile_policy(int p) {
  const int prev = gemm_policy().tile;
  if (p >= 0) gemm_policy().tile = p;
  return prev;
}

static constexpr int kTrsmRows = 16;
static constexpr int kTrsmMaxCols = 18 * 64;  // LDS bound: (18*64*16 + 1024) doubles < 160 KiB

// invD[i] must already hold the inverted diagonal blocks of descs[i].L.
// in_place: the small-LDS variant (every n a multiple of 64; see dtrsm_inv_kernel)
void launch_trsm_inv(const TrsmDesc* descs, const double* const* invD, int n, hipStream_t stream, bool in_place = false) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)dtrsm_inv_kernel<kTrsmRows, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  for (int s0 = 0; s0 < n; s0 += kMaxTrsmBatch) {
    int cnt = std::min(kMaxTrsmBatch, n - s0);
    TrsmInvArgs a;
    a.count = cnt;
    a.prio = t_launch_prio;
    a.gate_limit = parsec::trsm_inverse_limit();
    int total = 0, maxn = 0;
    for (int i = 0; i < cnt; ++i) {
      a.d[i] = descs[s0 + i];
      a.invD[i] = invD[s0 + i];
      a.block_start[i] = total;
      total += (a.d[i].m + kTrsmRows - 1) / kTrsmRows;
      maxn = std::max(maxn, a.d[i].n);
      if (in_place && a.d[i].n % 64 != 0) fatal("dtrsm in-place kernel: n=%d is not a multiple of 64", a.d[i].n);
    }
    a.block_start[cnt] = total;
    if (total == 0) continue;
    if (in_place) {
      hipLaunchKernelGGL((dtrsm_inv_kernel<kTrsmRows, true>), dim3(total), dim3(kTrsmThreads), 1024 * sizeof(double), stream, a);
      continue;
    }
    if (maxn > kTrsmMaxCols) fatal("dtrsm tile kernel: n=%d exceeds the LDS-resident panel limit %d", maxn, kTrsmMaxCols);
    size_t lds = ((size_t)((maxn + 63) / 64) * 64 * kTrsmRows + 1024) * sizeof(double);
    hipLaunchKernelGGL((dtrsm_inv_kernel<kTrsmRows, false>), dim3(total), dim3(kTrsmThreads), lds, stream, a);
  }
}

size_t trsm_workspace_bytes(const TrsmDesc* descs, int n) {
  size_t bytes = 0;
  std::vector<const double*> seen;
  for (int i = 0; i < n; ++i) {
    if (descs[i].invD) continue;
    if (std::find(seen.begin(), seen.end(), descs[i].L) != seen.end()) continue;
    seen.push_back(descs[i].L);
    bytes += (size_t)((descs[i].n + 63) / 64) * 4096 * sizeof(double);
  }
  return bytes;
}

// Diagonal-block inverses come from the descriptor (kept by POTRF) or are
// computed once per distinct L into the workspace.
void launch_trsm_batch(const TrsmDesc* descs, int n, hipStream_t stream, double* ws) {
  if (n <= 0) return;
  std::vector<std::pair<const double*, const double*>> seen;  // L -> inverse blocks
  std::vector<const double*> inv(n);
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    if (descs[i].invD) { inv[i] = descs[i].invD; continue; }
    auto it = std::find_if(seen.begin(), seen.end(), [&](const auto& e) { return e.first == descs[i].L; });
    if (it != seen.end()) { inv[i] = it->second; continue; }
    int nblk = (descs[i].n + 63) / 64;
    double* blk = ws + off;
    off += (size_t)nblk * 4096;
    hipLaunchKernelGGL(dtrtri_diag_kernel, dim3(nblk), dim3(kDiagThreads), 0, stream, descs[i].L, descs[i].ldl, descs[i].n, blk);
    seen.emplace_back(descs[i].L, blk);
    inv[i] = blk;
  }
  launch_trsm_inv(descs, inv.data(), n, stream);
}

void launch_trtri_diag(const double* L, int ldl, int n, double* invD, hipStream_t stream, bool unit) {
  if (n <= 0) return;
  if (unit)
    hipLaunchKernelGGL(dtrtri_diag_unit_kernel, dim3((n + 63) / 64), dim3(kDiagThreads), 0, stream, L, ldl, n, invD);
  else
    hipLaunchKernelGGL(dtrtri_diag_kernel, dim3((n + 63) / 64), dim3(kDiagThreads), 0, stream, L, ldl, n, invD);
}

void launch_trtri_diag_upper(const double* U, int ldu, int n, double* invD, hipStream_t stream, bool unit) {
  if (n <= 0) return;
  if (unit)
    hipLaunchKernelGGL(dtrtri_diag_upper_unit_kernel, dim3((n + 63) / 64), dim3(kDiagThreads), 0, stream, U, ldu, n, invD);
  else
    hipLaunchKernelGGL(dtrtri_diag_upper_kernel, dim3((n + 63) / 64), dim3(kDiagThreads), 0, stream, U, ldu, n, invD);
}

// a matrix and the triangle of it that is solved with: the lower and the upper
// triangle of one pointer are different matrices, and so are the unit and the
// non-unit reading of one triangle (bit 0: upper, bit 1: unit). The side is not
// part of it: a right-side solve uses the same inverses.
using TrsmLeftKey = std::pair<const double*, int>;
static inline TrsmLeftKey trsm_left_key(const TrsmLeftDesc& d) { return {d.L, (d.upper ? 1 : 0) | (d.unit ? 2 : 0)}; }

size_t trsm_left_workspace_bytes(const TrsmLeftDesc* descs, int n) {
  size_t bytes = 0;
  std::vector<TrsmLeftKey> seen;
  for (int i = 0; i < n; ++i) {
    if (descs[i].invD || descs[i].n <= 0) continue;
    const TrsmLeftKey key = trsm_left_key(descs[i]);
    if (std::find(seen.begin(), seen.end(), key) != seen.end()) continue;
    seen.push_back(key);
    bytes += (size_t)((descs[i].n + 63) / 64) * 4096 * sizeof(double);
  }
  return bytes;
}

// Left-side solves, one workgroup per 16 columns of every B. Diagonal-block
// inverses come from the descriptor or are computed once per distinct (L,
// triangle, unit) into ws. The lower and the upper descriptors go to their own
// instantiation of the kernel, each grouped 64 at a time in submission order.
void launch_trsm_left_batch(const TrsmLeftDesc* descs, int n, hipStream_t stream, double* ws) {
  if (n <= 0) return;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)dtrsm_left_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)dtrsm_left_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  std::vector<std::pair<TrsmLeftKey, const double*>> seen;  // (L, triangle) -> inverse blocks
  std::vector<const double*> inv(n, nullptr);
  std::vector<int> order[2];  // descriptor indices per triangle
  size_t off = 0;
  for (int i = 0; i < n; ++i) {
    const bool up = descs[i].upper != 0;
    order[up].push_back(i);
    if (descs[i].n <= 0 || descs[i].nrhs <= 0) continue;
    if (descs[i].invD) { inv[i] = descs[i].invD; continue; }
    const TrsmLeftKey key = trsm_left_key(descs[i]);
    auto it = std::find_if(seen.begin(), seen.end(), [&](const auto& e) { return e.first == key; });
    if (it != seen.end()) { inv[i] = it->second; continue; }
    int nblk = (descs[i].n + 63) / 64;
    double* blk = ws + off;
    off += (size_t)nblk * 4096;
    if (up)
      launch_trtri_diag_upper(descs[i].L, descs[i].ldl, descs[i].n, blk, stream, descs[i].unit != 0);
    else
      launch_trtri_diag(descs[i].L, descs[i].ldl, descs[i].n, blk, stream, descs[i].unit != 0);
    seen.emplace_back(key, blk);
    inv[i] = blk;
  }
  for (int up = 0; up < 2; ++up) {
    const std::vector<int>& idx = order[up];
    const int nd = (int)idx.size();
    for (int s0 = 0; s0 < nd; s0 += kMaxTrsmLeftBatch) {
      const int cnt = std::min(kMaxTrsmLeftBatch, nd - s0);
      TrsmLeftArgs a;
      a.count = cnt;
      a.prio = t_launch_prio;
      int total = 0, maxn = 0;
      for (int i = 0; i < cnt; ++i) {
        a.d[i] = descs[idx[s0 + i]];
        a.d[i].invD = inv[idx[s0 + i]];
        a.block_start[i] = total;
        if (a.d[i].n <= 0 || a.d[i].nrhs <= 0) continue;
        total += (a.d[i].nrhs + 15) / 16;
        maxn = std::max(maxn, a.d[i].n);
      }
      a.block_start[cnt] = total;
      if (total == 0) continue;
      if (maxn > kTrsmMaxCols) fatal("dtrsm left tile kernel: n=%d exceeds the LDS-resident strip limit %d", maxn, kTrsmMaxCols);
      const size_t lds = ((size_t)((maxn + 63) / 64) * 64 * 16 + 1024) * sizeof(double);
      if (up)
        hipLaunchKernelGGL(dtrsm_left_kernel<true>, dim3(total), dim3(kTrsmThreads), lds, stream, a);
      else
        hipLaunchKernelGGL(dtrsm_left_kernel<false>, dim3(total), dim3(kTrsmThreads), lds, stream, a);
    }
  }
}

// ================================== tile GETRF without pivoting (A = L U)
// Right-looking, blocked by 64 columns, three launches per block column j:
//   dgetrf_diag_kernel   one workgroup: A_jj := L_jj \ U_jj in registers, then
//                        inv(L_jj) (unit lower) and inv(U_jj) the same way
//   dgetrf_panel_kernel  one workgroup per 64 x 64 block of the block column
//                        below (A_ij := A_ij inv(U_jj)) and of the block row to
//                        the right (A_jk := inv(L_jj) A_jk): one 64^3 product on
//                        v_mfma_f64_16x16x4f64 from LDS
//   the grouped NN GEMM  A_ik -= A_ij A_jk over the trailing part
// No pivoting: a zero pivot is reported and the factorization goes on with
// inf / nan. 50 KB (diagonal) and 75 KB (panel) of LDS: either fits beside one
// resident 128 x 128 GEMM workgroup.
constexpr int kGetrfLd = 65;   // F of the diagonal kernel: [column][row], one pad
constexpr int kGetrfLdA = 80;  // MFMA A operand [k][row]: the two k of a 32-lane half land 32 banks apart
constexpr int kGetrfLdB = 66;  // MFMA B operand [column][k]: 16 columns x 2 k on 32 distinct bank pairs

__global__ __launch_bounds__(256) void dgetrf_diag_kernel(double* A, int lda, int j, int w, double* invL, double* invU, int* info, int info_base, int prio) {
  __shared__ double F[64 * kGetrfLd];      // F[c][r] = (L\U)(r, c), identity-padded past w
  __shared__ double Pn[2 * 16 * kGetrfLd];  // the two panel broadcast buffers
  __shared__ double rcp[64];  // 1 / U(c, c)
  __shared__ int bad_s;
  PARSEC_WAVE_PRIO(prio);
  double* T = A + (size_t)j * lda + j;
  const int r = threadIdx.x & 63;
  const int v = threadIdx.x >> 6;
  // thread (r, v): row r, columns 16v .. 16v+15
  double a[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = 16 * v + i;
    a[i] = (r < w && c < w) ? T[(size_t)c * lda + r] : (r == c ? 1.0 : 0.0);
  }
  if (threadIdx.x == 0) bad_s = 0x7fffffff;
  __syncthreads();
#pragma unroll 1
  for (int p = 0; p < 4; ++p) {
    double* pn = Pn + (p & 1) * 16 * kGetrfLd;
    if (v == p) {
      // wave p factors its 64 x 16 panel: lane jc holds row jc of U
      int bad = 0x7fffffff;
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int jc = 16 * p + jj;
        const double d = readlane_d(a[jj], jc);
        if (d == 0.0 && bad == 0x7fffffff) bad = jc + 1;  // the padding's pivots are 1
        const double rd = 1.0 / d;
        if (r > jc) a[jj] *= rd;
        const double lv = r > jc ? a[jj] : 0.0;
#pragma unroll
        for (int i = jj + 1; i < 16; ++i) a[i] = __builtin_fma(-lv, readlane_d(a[i], jc), a[i]);
        if (r == jc) rcp[jc] = rd;
      }
      if (r == 0 && bad != 0x7fffffff) atomicMin(&bad_s, bad);
#pragma unroll
      for (int i = 0; i < 16; ++i) pn[i * kGetrfLd + r] = a[i];
    }
    __syncthreads();
    if (v > p) {
      // the columns to the right: row 16p+s of U is final once the rows above it
      // were applied; every row below takes its multiple (solve and update in one)
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int js = 16 * p + s;
        const double l = r > js ? pn[s * kGetrfLd + r] : 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = __builtin_fma(-l, readlane_d(a[i], js), a[i]);
      }
    }
  }
  if (threadIdx.x == 0 && bad_s != 0x7fffffff && info) {
    const int val = info_base + j + bad_s;
    const int old = atomicCAS(info, 0, val);
    if (old != 0 && val < old) atomicMin(info, val);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = 16 * v + i;
    if (r < w && c < w) T[(size_t)c * lda + r] = a[i];
    F[c * kGetrfLd + r] = a[i];
  }
  __syncthreads();
  // The inverses by the same elimination on the identity, again with a row per
  // lane and 16 columns per wave: X = inv(L) from L X = I, and Y = inv(U)^T from
  // U^T Y = I (U^T is lower, with U's diagonal). Row js of either is final when
  // step js starts; the rows below take their multiple of it. Columns 16v.. of a
  // row js < 16v are still zero, so wave v starts at js = 16v.
  double x[16], y[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = y[i] = (r == 16 * v + i) ? 1.0 : 0.0;
#pragma unroll 1
  for (int js = 16 * v; js < 64; ++js) {
    const double l = r > js ? F[js * kGetrfLd + r] : 0.0;  // L(r, js)
    const double u = r > js ? F[r * kGetrfLd + js] : 0.0;  // U(js, r) = U^T(r, js)
    const double rd = rcp[js];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      x[i] = __builtin_fma(-l, readlane_d(x[i], js), x[i]);
      const double yj = readlane_d(y[i], js) * rd;
      y[i] = r == js ? yj : __builtin_fma(-u, yj, y[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int c = 16 * v + i;
    if (invL) invL[(size_t)c * 64 + r] = x[i];  // inv(L)(r, c)
    if (invU) invU[(size_t)r * 64 + c] = y[i];  // inv(U)(c, r) = Y(r, c)
  }
}

// blockIdx.x < nrb: block i of the column panel, A_ij := A_ij inv(U_jj);
// else block k of the row panel, A_jk := inv(L_jj) A_jk. The diagonal block is a
// full 64 x 64 one (there is no panel after a ragged one).
__global__ __launch_bounds__(256) void dgetrf_panel_kernel(double* A, int lda, int n, int j, const double* __restrict__ invL, const double* __restrict__ invU, int nrb, int prio) {
  __shared__ double As[64 * kGetrfLdA];  // As[k][row]: the left factor of the product
  __shared__ double Bs[64 * kGetrfLdB];  // Bs[column][k]: the right factor
  PARSEC_WAVE_PRIO(prio);
  const bool below = (int)blockIdx.x < nrb;
  const int o = j + 64 + 64 * (below ? (int)blockIdx.x : (int)blockIdx.x - nrb);
  const int wb = min(64, n - o);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  // the block of A: rows r0.., columns c0.., mr x nc valid
  const int r0 = below ? o : j, c0 = below ? j : o;
  const int mr = below ? wb : 64, nc = below ? 64 : wb;
  double* __restrict__ Ab = A + (size_t)c0 * lda + r0;
  for (int idx = tid; idx < 4096; idx += 256) {
    const int lo = idx & 63, hi = idx >> 6;
    if (below) {
      As[hi * kGetrfLdA + lo] = lo < mr ? Ab[(size_t)hi * lda + lo] : 0.0;  // A_ij(row lo, k hi)
      Bs[hi * kGetrfLdB + lo] = invU[hi * 64 + lo];                         // inv(U)(k lo, column hi)
    } else {
      As[hi * kGetrfLdA + lo] = invL[hi * 64 + lo];                         // inv(L)(row lo, k hi)
      Bs[hi * kGetrfLdB + lo] = hi < nc ? Ab[(size_t)hi * lda + lo] : 0.0;  // A_jk(k lo, column hi)
    }
  }
  __syncthreads();
  // wave wv: rows 16wv .. 16wv+15 of the product, four 16-column accumulators
  double4_t acc[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) acc[u] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int kk = 0; kk < 64; kk += 4) {
    const double av = As[(kk + fk) * kGetrfLdA + 16 * wv + fr];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Bs[(16 * u + fr) * kGetrfLdB + kk + fk], acc[u], 0, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = 16 * u + fr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int rr = 16 * wv + fk + 4 * q;
      if (rr < mr && c < nc) Ab[(size_t)c * lda + rr] = acc[u][q];
    }
  }
}

size_t getrf_workspace_bytes(const GetrfDesc& g) {
  const size_t nblk = (size_t)((g.n + 63) / 64);
  return ((g.invL_out ? 0 : nblk) + (g.invU_out ? 0 : nblk)) * 4096 * sizeof(double);
}

void launch_getrf_nopiv(const GetrfDesc& g, hipStream_t stream, double* ws) {
  if (g.n <= 0) return;
  if (g.n > kTrsmMaxCols) fatal("dgetrf tile kernel: n=%d exceeds the tile limit %d", g.n, kTrsmMaxCols);
  if (g.lda < g.n) fatal("dgetrf tile kernel: lda=%d < n=%d", g.lda, g.n);
  const int nblk = (g.n + 63) / 64;
  double* il = g.invL_out ? g.invL_out : ws;
  double* iu = g.invU_out ? g.invU_out : ws + (g.invL_out ? 0 : (size_t)nblk * 4096);
  for (int j = 0; j < g.n; j += 64) {
    const int jb = std::min(64, g.n - j);
    double* bl = il + (size_t)(j / 64) * 4096;
    double* bu = iu + (size_t)(j / 64) * 4096;
    hipLaunchKernelGGL(dgetrf_diag_kernel, dim3(1), dim3(256), 0, stream, g.A, g.lda, j, jb, bl, bu, g.info, g.info_base, t_launch_prio);
    const int rest = g.n - j - jb;
    if (rest <= 0) break;
    const int nrb = (rest + 63) / 64;
    hipLaunchKernelGGL(dgetrf_panel_kernel, dim3(2 * nrb), dim3(256), 0, stream, g.A, g.lda, g.n, j, (const double*)bl, (const double*)bu, nrb, t_launch_prio);
    GemmDesc e{};
    e.A = g.A + (size_t)j * g.lda + j + jb;
    e.B = g.A + (size_t)(j + jb) * g.lda + j;
    e.C = g.A + (size_t)(j + jb) * g.lda + j + jb;
    e.m = rest; e.n = rest; e.k = jb;
    e.lda = e.ldb = e.ldc = g.lda;
    e.alpha = -1.0; e.beta = 1.0;
    launch_gemm_batch(&e, 1, stream);
  }
}

__global__ void set_identity_kernel(double* W, int n, int ldw) {
  const int j = blockIdx.y;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) W[(size_t)j * ldw + i] = i == j ? 1.0 : 0.0;
}

constexpr int kMaxCopyBatch = 48;
constexpr int kMaxScan = 8;
struct CopyBatchArgs {
  int count;
  int prio;
  int rows[kMaxCopyBatch], cols[kMaxCopyBatch], ld_src[kMaxCopyBatch], ld_dst[kMaxCopyBatch];
  const double* src[kMaxCopyBatch];
  double* dst[kMaxCopyBatch];
  // condition estimate of the panel solves (PARSEC_DPOTRF_TRSM=auto): job j
  // maxes |L| and |W| into scan_slot[j][0 / 1] (workspace, zeroed before the
  // launch). Unpacked: L lower (scan_L), W lower (scan_W). Packed panel tile
  // (scan_packed): W = its lower part incl. the diagonal, L = its strict upper
  // part transposed with the diagonal 1 / W(i, i).
  int nscan;
  int scan_n[kMaxScan], scan_ldl[kMaxScan], scan_ldw[kMaxScan], scan_packed[kMaxScan];
  const double* scan_L[kMaxScan];
  const double* scan_W[kMaxScan];
  unsigned long long* scan_slot[kMaxScan];
  // unpack jobs: Wu (n x n, ld n) = the lower part incl. the diagonal of a
  // packed panel tile, zeros above: what the W-GEMM and the substitution's
  // diagonal blocks read
  int nunpack;
  int up_n[kMaxScan], up_ld[kMaxScan];
  const double* up_src[kMaxScan];
  double* up_dst[kMaxScan];
};
static_assert(sizeof(CopyBatchArgs) <= 4096, "CopyBatchArgs exceeds the kernel argument limit");

// blockIdx.y = tile, then the scan jobs, then the unpack jobs; blockIdx.x
// strides over columns; one wave-row per column.
__global__ __launch_bounds__(256) void copy_tiles_kernel(const CopyBatchArgs a) {
  PARSEC_WAVE_PRIO(a.prio);
  const int t = blockIdx.y;
  if (t >= a.count + a.nscan) {
    const int j = t - a.count - a.nscan;
    const int n = a.up_n[j];
    const size_t ld = a.up_ld[j];
    const double* __restrict__ P = a.up_src[j];
    double* __restrict__ W = a.up_dst[j];
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += gridDim.x * 4)
      for (int r = threadIdx.x & 63; r < n; r += 64) W[(size_t)c * n + r] = r >= c ? P[(size_t)c * ld + r] : 0.0;
    return;
  }
  if (t >= a.count) {
    const int j = t - a.count;
    const int n = a.scan_n[j];
    const double* __restrict__ L = a.scan_L[j];
    const double* __restrict__ W = a.scan_W[j];
    const size_t ldl = a.scan_ldl[j], ldw = a.scan_ldw[j];
    double mL = 0.0, mW = 0.0;
    if (a.scan_packed[j]) {
      for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += gridDim.x * 4)
        for (int r = threadIdx.x & 63; r < n; r += 64) {
          const double v = fabs(W[(size_t)c * ldw + r]);
          if (r >= c) mW = fmax(mW, v);
          if (r < c) mL = fmax(mL, v);
          if (r == c && v > 0.0) mL = fmax(mL, 1.0 / v);
        }
    } else {
      for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += gridDim.x * 4)
        for (int r = c + (threadIdx.x & 63); r < n; r += 64) {
          mL = fmax(mL, fabs(L[(size_t)c * ldl + r]));
          mW = fmax(mW, fabs(W[(size_t)c * ldw + r]));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mL = fmax(mL, __shfl_xor(mL, o));
      mW = fmax(mW, __shfl_xor(mW, o));
    }
    if ((threadIdx.x & 63) == 0 && (mL > 0.0 || mW > 0.0)) {
      // non-negative doubles order like their bit patterns: integer max
      unsigned long long* slot = a.scan_slot[j];
      __hip_atomic_fetch_max(slot, (unsigned long long)__double_as_longlong(mL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(slot + 1, (unsigned long long)__double_as_longlong(mW), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return;
  }
  const int rows = a.rows[t], cols = a.cols[t], lds = a.ld_src[t], ldd = a.ld_dst[t];
  const double* __restrict__ s = a.src[t];
  double* __restrict__ d = a.dst[t];
  if (lds == rows && ldd == rows && (((uintptr_t)s | (uintptr_t)d) % 16) == 0 && ((size_t)rows * cols) % 2 == 0) {
    // a whole contiguous tile (the panel solve's B tiles): 16-byte vectors,
    // four loads in flight per thread before the stores
    const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(s);
    uint4* __restrict__ d4 = reinterpret_cast<uint4*>(d);
    const size_t n = (size_t)rows * cols / 2, stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {
      const uint4 v0 = s4[i], v1 = s4[i + stride], v2 = s4[i + 2 * stride], v3 = s4[i + 3 * stride];
      d4[i] = v0;
      d4[i + stride] = v1;
      d4[i + 2 * stride] = v2;
      d4[i + 3 * stride] = v3;
    }
    for (; i < n; i += stride) d4[i] = s4[i];
    return;
  }
  for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < cols; c += gridDim.x * 4)
    for (int r = threadIdx.x & 63; r < rows; r += 64) d[(size_t)c * ldd + r] = s[(size_t)c * lds + r];
}

// Packed panel tile (PotrfDesc::pack_w): P(r, c) = L(c, r) for r < c, through
// a 64 x 64 LDS tile (coalesced on both sides); blocks below the diagonal exit.
__global__ __launch_bounds__(256) void pack_upper_lt_kernel(double* __restrict__ P, int ldp, const double* __restrict__ L, int ldl, int n) {
  __shared__ double t[64][65];
  const int br = blockIdx.x, bc = blockIdx.y;  // P block (br, bc), br <= bc
  if (br > bc) return;
  const int r0 = br * 64, c0 = bc * 64;
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int cc = e >> 6, rr = e & 63;  // read L(c0 + rr, r0 + cc): column r0 + cc of L, contiguous in rr
    const int lr = c0 + rr, lc = r0 + cc;
    t[cc][rr] = (lr < n && lc < n) ? L[(size_t)lc * ldl + lr] : 0.0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < 4096; e += 256) {
    const int cc = e >> 6, rr = e & 63;  // write P(r0 + rr, c0 + cc) = L(c0 + cc, r0 + rr) = t[rr][cc]
    const int pr = r0 + rr, pc = c0 + cc;
    if (pr < n && pc < n && pr < pc) P[(size_t)pc * ldp + pr] = t[rr][cc];
  }
}

size_t potrf_workspace_bytes(const PotrfDesc& p) {
  if (!p.W_out) return 4096 * sizeof(double);
  const size_t inv = p.invD_out ? 0 : (size_t)((p.n + 63) / 64) * 4096;
  const size_t tmp = (size_t)p.n * p.n / 2 + 4096;  // doubling products, <= n^2/4 (+ a partial group)
  return (inv + tmp) * sizeof(double);
}

// X = L^-1 (n x n lower, ld ldx, zero above the diagonal) from the inverses of
// L's 64x64 diagonal blocks by recursive doubling: groups of g blocks pair up,
// inv([A 0; B C]) = [inv(A) 0; -inv(C) B inv(A)  inv(C)], each level two
// grouped MFMA GEMMs over all pairs (log2(n/64) levels, no sequential solve).
void launch_trsm_w_batch(const TrsmGemmDesc* d, int n, hipStream_t stream, double* ws);
static void launch_lower_inverse(const double* L, int lda, int n, const double* invD, double* X, int ldx, double* tmp, hipStream_t stream) {
  const int nblk = (n + 63) / 64;
  (void)hipMemset2DAsync(X, (size_t)ldx * sizeof(double), 0, (size_t)n * sizeof(double), n, stream);
  for (int b0 = 0; b0 < nblk; b0 += kMaxCopyBatch) {
    CopyBatchArgs ca;
    ca.count = std::min(kMaxCopyBatch, nblk - b0);
    ca.prio = t_launch_prio;
    ca.nscan = 0;
    ca.nunpack = 0;
    for (int i = 0; i < ca.count; ++i) {
      const int b = b0 + i, w = std::min(64, n - 64 * b);
      ca.rows[i] = w; ca.cols[i] = w; ca.ld_src[i] = 64; ca.ld_dst[i] = ldx;
      ca.src[i] = invD + (size_t)b * 4096;
      ca.dst[i] = X + (size_t)64 * b * ldx + 64 * b;
    }
    hipLaunchKernelGGL(copy_tiles_kernel, dim3(16, ca.count), dim3(256), 0, stream, ca);
  }
  std::vector<GemmDesc> g1, g2;
  for (int g = 1; g < nblk; g *= 2) {
    g1.clear();
    g2.clear();
    size_t off = 0;
    for (int a0 = 0; a0 + g < nblk; a0 += 2 * g) {
      const int ra = 64 * a0, rc = 64 * (a0 + g);
      const int sa = std::min(64 * g, n - ra), sc = std::min(64 * g, n - rc);
      double* T = tmp + off;
      off += (size_t)sc * sa;
      GemmDesc e{};
      // T = L[C rows, A cols] * X_A
      e.A = L + (size_t)ra * lda + rc; e.lda = lda;
      e.B = X + (size_t)ra * ldx + ra; e.ldb = ldx;
      e.C = T; e.ldc = sc;
      e.m = sc; e.n = sa; e.k = sa;
      e.alpha = 1.0; e.beta = 0.0;
      g1.push_back(e);
      // X[C rows, A cols] = -X_C * T
      GemmDesc f{};
      f.A = X + (size_t)rc * ldx + rc; f.lda = ldx;
      f.B = T; f.ldb = sc;
      f.C = X + (size_t)ra * ldx + rc; f.ldc = ldx;
      f.m = sc; f.n = sa; f.k = sc;
      f.alpha = -1.0; f.beta = 0.0;
      g2.push_back(f);
    }
    launch_gemm_batch(g1.data(), (int)g1.size(), stream);
    launch_gemm_batch(g2.data(), (int)g2.size(), stream);
  }
}

// Blocked tile Cholesky (lower). ws needs 4096 doubles unless p.invD_out keeps
// every diagonal-block inverse (then the panel TRSMs can reuse them); with W_out
// and no invD_out it needs every block inverse (potrf_workspace_bytes).
void launch_trsm_inv(const TrsmDesc* descs, const double* const* invD, int n, hipStream_t stream, bool in_place);
void launch_potrf(const PotrfDesc& p, hipStream_t stream, double* ws) {
  const int JB = 64;
  const bool keep_all = p.invD_out || p.W_out;
  double* inv_base = p.invD_out ? p.invD_out : ws;
  for (int j = 0; j < p.n; j += JB) {
    const int jb = std::min(JB, p.n - j);
    double* inv = keep_all ? inv_base + (size_t)(j / JB) * 4096 : ws;
    hipLaunchKernelGGL(dpotrf_diag_inv_kernel, dim3(1), dim3(kDiagThreads), 0, stream, p.A, p.lda, j, jb, inv, p.info);
    const int rest = p.n - j - jb;
    if (rest <= 0) break;
    TrsmDesc t;
    t.L = p.A + (size_t)j * p.lda + j;
    t.B = p.A + (size_t)j * p.lda + j + jb;
    t.m = rest; t.n = jb; t.ldl = p.lda; t.ldb = p.lda; t.trans = 1;
    const double* cinv = inv;
    launch_trsm_inv(&t, &cinv, 1, stream);
    GemmDesc g{};
    g.A = t.B; g.B = t.B; g.C = p.A + (size_t)(j + jb) * p.lda + j + jb;
    g.m = rest; g.n = rest; g.k = jb; g.lda = p.lda; g.ldb = p.lda; g.ldc = p.lda;
    g.alpha = -1.0; g.beta = 1.0; g.transA = 0; g.transB = 1; g.lower_only = 1; g.a_lower = 0;
    launch_gemm_batch(&g, 1, stream);
  }
  if (p.W_out) {
    // W = L^-1 from the diagonal-block inverses just computed
    double* tmp = ws + (p.invD_out ? 0 : (size_t)((p.n + 63) / 64) * 4096);
    launch_lower_inverse(p.A, p.lda, p.n, inv_base, p.W_out, p.ldw, tmp, stream);
    if (p.pack_w) {
      const int nblk = (p.n + 63) / 64;
      hipLaunchKernelGGL(pack_upper_lt_kernel, dim3(nblk, nblk), dim3(256), 0, stream, p.W_out, p.ldw, p.A, p.lda, p.n);
    }
  }
}

// ============================ tile TRTRI, grouped TRMM (L^T B) and tile LAUUM
// The inverse-with-the-Cholesky-factor kernels (DTRTRI / DLAUUM / DPOTRI). All
// three take a lower triangular tile whose strict upper triangle belongs to
// somebody else (the user's symmetric matrix keeps its upper half there): the
// results never depend on it and it is never written.

// dst's lower triangle := src's lower triangle (n x n); zero_upper also clears
// dst's strict upper triangle (a workspace copy that GEMM-like kernels may read
// as a full square). One workgroup per 64 x 64 block.
__global__ __launch_bounds__(256) void copy_lower_kernel(const double* __restrict__ src, int lds, double* __restrict__ dst, int ldd, int n, int zero_upper) {
  const int r0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  if (c0 > r0 && !zero_upper) return;
  const int r = r0 + (threadIdx.x & 63);
  if (r >= n) return;
  for (int cc = threadIdx.x >> 6; cc < 64; cc += 4) {
    const int c = c0 + cc;
    if (c >= n) break;
    if (r >= c)
      dst[(size_t)c * ldd + r] = src[(size_t)c * lds + r];
    else if (zero_upper)
      dst[(size_t)c * ldd + r] = 0.0;
  }
}

// *info := info_base + the 1-based index of the first exactly-zero diagonal entry
// of A (n x n), unless a smaller non-zero value is already there (GetrfDesc's rule)
__global__ __launch_bounds__(256) void dtrtri_info_kernel(const double* __restrict__ A, int lda, int n, int* info, int info_base) {
  __shared__ int bad_s;
  if (threadIdx.x == 0) bad_s = 0x7fffffff;
  __syncthreads();
  int bad = 0x7fffffff;
  for (int i = threadIdx.x; i < n; i += 256)
    if (A[(size_t)i * lda + i] == 0.0) { bad = i + 1; break; }
  if (bad != 0x7fffffff) atomicMin(&bad_s, bad);
  __syncthreads();
  if (threadIdx.x == 0 && bad_s != 0x7fffffff) {
    const int val = info_base + bad_s;
    const int old = atomicCAS(info, 0, val);
    if (old != 0 && val < old) atomicMin(info, val);
  }
}

size_t trtri_workspace_bytes(const TrtriDesc& t) {
  const size_t inv = t.invD ? 0 : (size_t)((t.n + 63) / 64) * 4096;
  const size_t tmp = (size_t)t.n * t.n / 2 + 4096;  // the doubling products of launch_lower_inverse
  return (inv + (size_t)t.n * t.n + tmp) * sizeof(double);
}

// Tile TRTRI: the 64 x 64 diagonal-block inverses (dtrtri_diag_kernel, or the
// caller's), then the block size doubles level by level, X21 = -X22 L21 X11 as
// two grouped MFMA GEMMs over all pairs of a level (launch_lower_inverse). The
// doubling runs in a clean n x n workspace square, because its products read
// the X11 / X22 triangles as full squares (zeros above); the last kernel copies
// the lower triangle to A (in place) or to W_out. L is read only before that
// copy and only below its diagonal blocks, so in place needs no second buffer.
void launch_trtri(const TrtriDesc& t, hipStream_t stream, double* ws) {
  if (t.n <= 0) return;
  if (t.n > kTrsmMaxCols) fatal("dtrtri tile kernel: n=%d exceeds the tile limit %d", t.n, kTrsmMaxCols);
  if (t.lda < t.n || (t.W_out && t.ldw < t.n)) fatal("dtrtri tile kernel: leading dimension below n=%d", t.n);
  const int nblk = (t.n + 63) / 64;
  if (t.info) hipLaunchKernelGGL(dtrtri_info_kernel, dim3(1), dim3(256), 0, stream, (const double*)t.A, t.lda, t.n, t.info, t.info_base);
  const double* inv = t.invD;
  if (!inv) {
    launch_trtri_diag(t.A, t.lda, t.n, ws, stream);
    inv = ws;
    ws += (size_t)nblk * 4096;
  }
  double* X = ws;
  launch_lower_inverse(t.A, t.lda, t.n, inv, X, t.n, X + (size_t)t.n * t.n, stream);
  hipLaunchKernelGGL(copy_lower_kernel, dim3(nblk, nblk), dim3(256), 0, stream, (const double*)X, t.n, t.W_out ? t.W_out : t.A, t.W_out ? t.ldw : t.lda, t.n, 0);
}

constexpr int kMaxTrmmBatch = 64;
struct TrmmArgs {
  int count;
  int prio;
  int block_start[kMaxTrmmBatch + 1];
  TrmmDesc d[kMaxTrmmBatch];
};
static_assert(sizeof(TrmmArgs) <= 4096, "TrmmArgs exceeds the kernel argument limit");

// B := alpha L^T B in place. Row block I of the result needs rows >= I of B
// only, and a workgroup owns 16 columns of B: it loads its whole strip into LDS
// ([row][16], rows zero-padded to a multiple of 16: the layout of
// dtrsm_left_kernel, conflict-free MFMA B-operand reads), and only after the
// barrier the waves write result rows back, so the in-place sweep never meets a
// row it still needs. Wave w takes the 16-row blocks w, 15 - w, 16 + w, ... (the
// work of a block shrinks linearly with its row, so the pairs even it out):
// R_I = sum_{k >= I} L(k, I)^T B(k), v_mfma_f64_16x16x4f64 with L(k, I) read
// from global memory (lane (fr, fk) feeds column I + fr, rows k + 4u + fk: every
// element read lies on or below the diagonal, the diagonal 16 x 16 block is
// masked, the ragged last k block is guarded).
// TrmmDesc::lower: B is lower triangular (LAUUM): elements above its diagonal
// are loaded as zero and not stored, and the row blocks above the strip's first
// column are skipped. 66 VGPRs, no scratch: the waves fit beside a bulk GEMM
// workgroup's; the strip takes n x 128 bytes of LDS (64 KB at n = 512).
__global__ __launch_bounds__(kTrsmThreads) void dtrmm_lt_kernel(const TrmmArgs args) {
  extern __shared__ double P[];  // [rows padded][16]
  PARSEC_WAVE_PRIO(args.prio);
  const int b = blockIdx.x;
  const int di = find_desc(args, args.block_start, b);
  const TrmmDesc& d = args.d[di];
  const int j0 = (b - args.block_start[di]) * 16;
  const int n = d.n, nrhs = d.nrhs;
  const int nrb = (n + 15) / 16;
  const bool lower = d.lower != 0;
  const double alpha = d.alpha;
  double* Bp = d.B;
  const size_t ldb = d.ldb;
  const double* __restrict__ L = d.L;
  const size_t ldl = d.ldl;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  for (int idx = tid; idx < nrb * 256; idx += kTrsmThreads) {
    const int i = idx >> 4, c = j0 + (idx & 15);
    P[idx] = (i < n && c < nrhs && (!lower || i >= c)) ? Bp[(size_t)c * ldb + i] : 0.0;
  }
  __syncthreads();
  const int ib0 = lower ? j0 / 16 : 0;
  for (int t = 0;; ++t) {
    const int ib = ib0 + 8 * t + ((t & 1) ? 7 - wv : wv);
    if (ib0 + 8 * t >= nrb) break;
    if (ib >= nrb) continue;
    const int i0 = ib * 16;
    const int col = i0 + fr;  // column of L this lane feeds as the MFMA A-operand
    const double* __restrict__ Lp = L + (size_t)min(col, n - 1) * ldl;
    double4_t acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // the diagonal block: only k >= column is L
      const int kk = i0 + 4 * u + fk;
      const double av = (kk >= col && kk < n) ? Lp[kk] : 0.0;
      acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, P[kk * 16 + fr], (double4_t){0.0, 0.0, 0.0, 0.0}, 0, 0, 0);
    }
    int k = i0 + 16;
    for (; k + 16 <= n; k += 16) {
      double av[4], bv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = k + 4 * u + fk;
        av[u] = Lp[kk];
        bv[u] = P[kk * 16 + fr];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u], acc[u], 0, 0, 0);
    }
    if (k < n) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int kk = k + 4 * u + fk;
        const double av = kk < n ? Lp[kk] : 0.0;
        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, P[kk * 16 + fr], acc[u], 0, 0, 0);
      }
    }
    const double4_t sum = acc[0] + acc[1] + acc[2] + acc[3];
    const int c = j0 + fr;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = i0 + fk + 4 * q;
      if (r < n && c < nrhs && (!lower || r >= c)) Bp[(size_t)c * ldb + r] = alpha * sum[q];
    }
  }
}

// One grouped launch per 64 descriptors, one workgroup per 16 columns of every B.
void launch_trmm_lt_batch(const TrmmDesc* descs, int n, hipStream_t stream) {
  if (n <= 0) return;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)dtrmm_lt_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  for (int s0 = 0; s0 < n; s0 += kMaxTrmmBatch) {
    const int cnt = std::min(kMaxTrmmBatch, n - s0);
    TrmmArgs a;
    a.count = cnt;
    a.prio = t_launch_prio;
    int total = 0, maxn = 0;
    for (int i = 0; i < cnt; ++i) {
      a.d[i] = descs[s0 + i];
      a.block_start[i] = total;
      if (a.d[i].n <= 0 || a.d[i].nrhs <= 0) continue;
      if (a.d[i].ldl < a.d[i].n || a.d[i].ldb < a.d[i].n) fatal("dtrmm tile kernel: leading dimension below n=%d", a.d[i].n);
      if (a.d[i].lower && a.d[i].nrhs != a.d[i].n) fatal("dtrmm tile kernel: a lower triangular B is square (n=%d, nrhs=%d)", a.d[i].n, a.d[i].nrhs);
      total += (a.d[i].nrhs + 15) / 16;
      maxn = std::max(maxn, a.d[i].n);
    }
    a.block_start[cnt] = total;
    if (total == 0) continue;
    if (maxn > kTrsmMaxCols) fatal("dtrmm tile kernel: n=%d exceeds the LDS-resident strip limit %d", maxn, kTrsmMaxCols);
    const size_t lds = (size_t)((maxn + 15) / 16) * 256 * sizeof(double);
    hipLaunchKernelGGL(dtrmm_lt_kernel, dim3(total), dim3(kTrsmThreads), lds, stream, a);
  }
}

size_t lauum_workspace_bytes(const LauumDesc& l) { return (size_t)l.n * l.n * sizeof(double); }

// Tile LAUUM, A := lower(L^T L) in place. Column strip J of the product reads
// the columns >= J of L that other workgroups are overwriting at the same time.
// The answer chosen here: the lower triangle of L is first copied to a workspace
// square, and the grouped TRMM kernel then multiplies A's own lower triangle by
// that copy's transpose (TrmmDesc::lower: lower-only load and store), so no
// workgroup reads a location another one writes.
void launch_lauum(const LauumDesc& l, hipStream_t stream, double* ws) {
  if (l.n <= 0) return;
  if (l.n > kTrsmMaxCols) fatal("dlauum tile kernel: n=%d exceeds the tile limit %d", l.n, kTrsmMaxCols);
  if (l.lda < l.n) fatal("dlauum tile kernel: lda=%d < n=%d", l.lda, l.n);
  const int nblk = (l.n + 63) / 64;
  hipLaunchKernelGGL(copy_lower_kernel, dim3(nblk, nblk), dim3(256), 0, stream, (const double*)l.A, l.lda, ws, l.n, l.n, 1);
  TrmmDesc t{ws, l.A, l.n, l.n, l.n, l.lda, 1.0, 1};
  launch_trmm_lt_batch(&t, 1, stream);
}

// ====================================== tile POTRF (+W) in n/64 + 1 launches
// Right-looking blocked Cholesky of an n x n tile (n % 64 == 0) by 64-column
// steps, ONE launch per step: the launch of step j holds every work item that
// depends only on step j-1's results, each item a 256-thread workgroup that
// recomputes the panel blocks it needs instead of waiting for another workgroup
// (no grid barrier, no inter-workgroup hand-off: the kernel boundary is the only
// synchronisation, 1.5 us on MI355X against ~5-20 us for an in-kernel barrier
// with the cross-XCD L2 write-backs it needs). With D_j = L_jj, iD_j = D_j^-1
// (64 x 64, kept in invD) and P_x = A_xj iD_j^T (= L_xj):
//   DIAG   (j+1)        D = A_{j+1,j+1} - P_{j+1} P_{j+1}^T, factor D, invert it
//   TRAIL  (r, c)       A_rc -= P_r P_c^T               j < c <= r, (r,c) != (j+1,j+1)
//   LW     (r)          A_{r,j-1} := P_r of step j-1     (written one step late: step
//                                                       j no longer reads column j-1)
// and, when W = L^-1 is wanted, a right-looking forward substitution L X = I
// carried along in the W buffer (R = the right-hand sides, X_jc = iD_j R_jc):
//   RUPD   (r, c)       R_rc -= P_r X_jc                 r > j >= c (X_jj = iD_j)
//   XW     (c)          W_{j-1,c} := iD_{j-1} R_{j-1,c}  (row j-1 is final)
// The first launch factors D_0 and zeroes W, the last one writes the final panel
// and X rows. Every item runs 2-3 64^3 block products on v_mfma_f64_16x16x4f64
// (4 waves, a 32 x 32 quadrant each) from LDS; DIAG adds the 64 x 64 factor +
// inverse of diag_factor_inv. Critical path per step: one launch boundary + DIAG.
#ifndef PARSEC_POTRF_KPL
#define PARSEC_POTRF_KPL 78
#endif
// LDS ld of a staged 64x64 block: 78 (156 dwords) keeps the step kernel at 78 KB,
// so it fits beside ONE bulk GEMM workgroup padded to 82 KB (device_hip_bulk_gemm_per_cu
// = 1: at most one bulk workgroup per CU); 80 (160 dwords = 32 mod 64) is the
// conflict-free stride of round 2 (80 KB)
constexpr int kPL = PARSEC_POTRF_KPL;
typedef double Blk[64][kPL];  // operand form: S[k][m] = op(m, k)

// S[k][m] = G(m, k) (col-major, ld) or, transposed, S[k][m] = G(k, m)
__device__ __forceinline__ void stage_blk(Blk& S, const double* __restrict__ G, int ld, bool t) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int p = tid + 256 * e;
    const int hi = p >> 5, lo = (p & 31) * 2;
    const double2_t v = *reinterpret_cast<const double2_t*>(G + (size_t)hi * ld + lo);
    if (!t) {
      *reinterpret_cast<double2_t*>(&S[hi][lo]) = v;
    } else {
      S[lo][hi] = v.x;
      S[lo + 1][hi] = v.y;
    }
  }
}

__device__ __forceinline__ void acc_zero(double4_t (&acc)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (double4_t){0.0, 0.0, 0.0, 0.0};
}

// acc (this wave's quadrant of C) += sign * sum_k S_a[k][m] S_b[k][n]
__device__ __forceinline__ void mma_blk(double4_t (&acc)[2][2], const Blk& Sa, const Blk& Sb, double sign) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qm = (w & 1) * 32, qn = (w >> 1) * 32;
  const int r = lane & 15, kq = lane >> 4;
#pragma unroll 4
  for (int kk = 0; kk < 64; kk += 4) {
    double y[2], x[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) y[j] = Sa[kk + kq][qm + j * 16 + r];
#pragma unroll
    for (int i = 0; i < 2; ++i) x[i] = sign * Sb[kk + kq][qn + i * 16 + r];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[i], y[j], acc[i][j], 0, 0, 0);
  }
}

// (m, n) of accumulator element q of tile (i, j) for this lane
#define PARSEC_ACC_MN(i, j, q)                                     \
  const int m = qm + (j) * 16 + (lane & 15);                       \
  const int n = qn + (i) * 16 + (lane >> 4) + 4 * (q)

// acc -> LDS: S[n][m] = C(m, n) (operand form of C as an NT operand) or, with
// t, S[m][n] = C(m, n) (C as the B operand of an NN product)
__device__ __forceinline__ void acc_to_blk(const double4_t (&acc)[2][2], Blk& S, bool t) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qm = (w & 1) * 32, qn = (w >> 1) * 32;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        PARSEC_ACC_MN(i, j, q);
        if (t) S[m][n] = acc[i][j][q];
        else S[n][m] = acc[i][j][q];
      }
}

// acc = C (global, col-major ldc) or 0
__device__ __forceinline__ void acc_load(double4_t (&acc)[2][2], const double* __restrict__ C, int ldc) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qm = (w & 1) * 32, qn = (w >> 1) * 32;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        PARSEC_ACC_MN(i, j, q);
        acc[i][j][q] = C ? C[(size_t)n * ldc + m] : 0.0;
      }
}

__device__ __forceinline__ void acc_store(const double4_t (&acc)[2][2], double* __restrict__ C, int ldc, bool lower) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qm = (w & 1) * 32, qn = (w >> 1) * 32;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        PARSEC_ACC_MN(i, j, q);
        if (lower && m < n) continue;
        C[(size_t)n * ldc + m] = acc[i][j][q];
      }
}
#undef PARSEC_ACC_MN

// 16 x 16 x kn MFMA product into one accumulator tile: acc(m, n) += sign *
// sum_k Sa[k][m] Sb[k][n] (LDS, leading dimensions lda_s / ldb_s, k from k0).
// Lane layout of acc: m = lane & 15, n = (lane >> 4) + 4 q.
__device__ __forceinline__ void mfma16(double4_t& acc, const double* Sa, int lda_s, const double* Sb, int ldb_s, int k0, int kn, double sign) {
  const int lane = threadIdx.x & 63;
  const int r = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < kn; kk += 4) {
    const double y = Sa[(k0 + kk + kq) * lda_s + r];
    const double x = sign * Sb[(k0 + kk + kq) * ldb_s + r];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
  }
}

// Factor the 64 x 64 SPD block held in LDS (Dl[c][r] = D(r, c), ld kPL) in
// place and invert the factor: L (lower part) -> T (global, ldt), X = L^-1 ->
// invD (64 x 64, col-major). Four iterations over 16-column panels with a
// one-panel lookahead; in iteration q
//   all waves   apply panel q-1's rank-16 update to column block q, one 16 x 16
//               tile each (v_mfma_f64_16x16x4f64 from LDS), then one barrier
//               (spread = false: wave q updates the whole block itself);
//   wave q      factors panel q (rows in lanes; the next pivot column through
//               v_readlane, the other columns through an LDS broadcast: the
//               only serial chain) and stores it;
//   the others  apply panel q-1's update to the tiles right of column block q,
//               wave q-1 inverts its 16 x 16 diagonal block X_{q-1,q-1} (forward
//               substitution, lane = column) and wave j < q-2 forms X_{q-2,j};
// then X_33 beside row 2 and the known parts of row 3, then the rest of row 3.
// Only the panel chain and one column-block update per panel are serial; the
// rest of the update and the inverse run beside them.
// `pool` (kDiagPoolDoubles, not overlapping Dl) holds X block-packed (the 10
// lower 16 x 16 blocks, row-major), the diagonal blocks of X col-major, per-wave
// scratch and the broadcast buffers.
constexpr int kDiagPoolDoubles = 2560 + 1024 + 1024 + 64 + 128 + 1;
__device__ __forceinline__ int xblk(int i, int j) { return (i * (i + 1) / 2 + j) * 256; }  // block (i >= j) of X
// Diagnostics (PARSEC_POTRF_STAMPS=1): wall clock (100 MHz) at the phase
// boundaries of the last diagonal factorization, read by parsec_amd_potrf_stamps
__device__ long long g_potrf_stamps[16];
static int g_potrf_stamp_mode = -1;
#define PARSEC_STAMP(k) do { if (stamp && threadIdx.x == 0) g_potrf_stamps[k] = wall_clock64(); } while (0)

// X_ij (tile of the inverse, i > j) by wave-local MFMA: T = sum_k L_ik X_kj,
// X_ij = -X_ii T (Xc block i as the A operand)
__device__ __forceinline__ void inv_tile(const double* Dl, double* Xb, const double* Xc, double* Tw, int i, int j) {
  const int lane = threadIdx.x & 63;
  double4_t t = (double4_t){0.0, 0.0, 0.0, 0.0};
  for (int k = j; k < i; ++k)  // Sa[kk][m] = L(16i + m, 16k + kk); Sb[kk][n] = X(16k + kk, 16j + n)
    mfma16(t, Dl + 16 * k * kPL + 16 * i, kPL, Xb + xblk(k, j), 16, 0, 16, 1.0);
#pragma unroll
  for (int q = 0; q < 4; ++q) Tw[((lane >> 4) + 4 * q) + 16 * (lane & 15)] = t[q];  // row-major T: B operand Sb[k][n] = T(k, n)
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's own LDS writes are visible to it
  double4_t x = (double4_t){0.0, 0.0, 0.0, 0.0};
  mfma16(x, Xc + 256 * i, 16, Tw, 16, 0, 16, -1.0);
#pragma unroll
  for (int q = 0; q < 4; ++q) Xb[xblk(i, j) + (lane & 15) * 16 + (lane >> 4) + 4 * q] = x[q];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
}

// X_pp = L_pp^-1 (16 x 16 diagonal block p of the factor in Dl, pivots' 1/L(i,i)
// in dinv): lane c < 16 owns column c, s_i -= L(i, k) x_k as soon as x_k is known
__device__ __forceinline__ void diag_block_inverse(const double* Dl, double* Xb, double* Xc, const double* dinv, int p) {
  const int lane = threadIdx.x & 63;
  if (lane < 16) {
    const int b0 = 16 * p;
    double sv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) sv[i] = (i == lane) ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      sv[k] *= dinv[b0 + k];
#pragma unroll
      for (int i = k + 1; i < 16; ++i) sv[i] = __builtin_fma(-Dl[(b0 + k) * kPL + b0 + i], sv[k], sv[i]);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      Xb[xblk(p, p) + i * 16 + lane] = sv[i];
      Xc[p * 256 + lane * 16 + i] = sv[i];
    }
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
}

// Row 3 of the inverse, X_3j = -X_33 T_3j with T_3j = sum_{k=j..2} L_3k X_kj,
// split so the serial tail is short: while X_33 and row 2 are formed, wave 2
// computes T_32 = L_32 X_22 (B-operand form in its scratch) and the k < 2 parts
// of T_30 and T_31 (accumulator layout, parked in the X_30 / X_31 slots)
__device__ __forceinline__ void row3_partials(const double* Dl, double* Xb, double* Tw) {
  const int lane = threadIdx.x & 63;
  double4_t t = (double4_t){0.0, 0.0, 0.0, 0.0};
  mfma16(t, Dl + 32 * kPL + 48, kPL, Xb + xblk(2, 2), 16, 0, 16, 1.0);
#pragma unroll
  for (int q = 0; q < 4; ++q) Tw[((lane >> 4) + 4 * q) + 16 * (lane & 15)] = t[q];
  double4_t t0 = (double4_t){0.0, 0.0, 0.0, 0.0}, t1 = t0;
  mfma16(t0, Dl + 48, kPL, Xb + xblk(0, 0), 16, 0, 16, 1.0);
  mfma16(t1, Dl + 16 * kPL + 48, kPL, Xb + xblk(1, 1), 16, 0, 16, 1.0);
  mfma16(t0, Dl + 16 * kPL + 48, kPL, Xb + xblk(1, 0), 16, 0, 16, 1.0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    Xb[xblk(3, 0) + q * 64 + lane] = t0[q];
    Xb[xblk(3, 1) + q * 64 + lane] = t1[q];
  }
}
__device__ __forceinline__ void row3_finish(const double* Dl, double* Xb, const double* Xc, double* Tw, int j) {
  const int lane = threadIdx.x & 63;
  if (j < 2) {
    double4_t t;
#pragma unroll
    for (int q = 0; q < 4; ++q) t[q] = Xb[xblk(3, j) + q * 64 + lane];
    mfma16(t, Dl + 32 * kPL + 48, kPL, Xb + xblk(2, j), 16, 0, 16, 1.0);
#pragma unroll
    for (int q = 0; q < 4; ++q) Tw[((lane >> 4) + 4 * q) + 16 * (lane & 15)] = t[q];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);
  }
  double4_t x = (double4_t){0.0, 0.0, 0.0, 0.0};
  mfma16(x, Xc + 256 * 3, 16, Tw, 16, 0, 16, -1.0);
#pragma unroll
  for (int q = 0; q < 4; ++q) Xb[xblk(3, j) + (lane & 15) * 16 + (lane >> 4) + 4 * q] = x[q];
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);
}

__device__ __forceinline__ void diag_factor_inv(double* __restrict__ Dl, double* __restrict__ pool, double* __restrict__ T, int ldt, double* __restrict__ invD, int* info, int info_base, bool stamp, bool spread = false) {
  PARSEC_STAMP(1);
  double* Xb = pool;                    // X, block-packed: Xb[xblk(i, j) + m * 16 + n] = X(16i + m, 16j + n)
  double* Xc = pool + 2560;             // 4 diagonal blocks, col-major 16 x 16: Xc[b*256 + k*16 + m] = X(16b+m, 16b+k)
  double* Tw = Xc + 1024;               // per-wave 16 x 16 scratch (row-major)
  double* dinv = Tw + 1024;             // 1 / L(i, i)
  double* colb = dinv + 64;             // column broadcast buffers of the panel wave (2 x 64)
  int* bad_s = reinterpret_cast<int*>(colb + 128);
  const int lane = threadIdx.x & 63;
  const int v = threadIdx.x >> 6;
  const int r = lane;
  if (threadIdx.x == 0) *bad_s = 0x7fffffff;
  __syncthreads();
  PARSEC_STAMP(2);
  // rank-16 update of tile (R, C) by panel p
  auto upd_tile = [&](int R, int C, int p) {
    double4_t acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = Dl[(16 * C + (lane >> 4) + 4 * q) * kPL + 16 * R + (lane & 15)];
    mfma16(acc, Dl + 16 * R, kPL, Dl + 16 * C, kPL, 16 * p, 16, -1.0);
#pragma unroll
    for (int q = 0; q < 4; ++q) Dl[(16 * C + (lane >> 4) + 4 * q) * kPL + 16 * R + (lane & 15)] = acc[q];
  };
  // unrolled: every v_readlane below gets a constant lane index
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (spread && p >= 1) {
      // panel p-1's update of column block p dealt one tile per wave, so the
      // panel wave starts from a finished block after one barrier
      if (v < 4 - p) upd_tile(p + v, p, p - 1);
      __syncthreads();
    }
    if (v == p) {
      if (p >= 1 && !spread) {  // lookahead: panel p-1's update of this wave's own column block
        // the 4 - p tiles' k-steps interleaved: independent accumulators keep
        // the MFMA pipe fed instead of one dependent chain per tile
        double4_t acc[3];
        const int rr = lane & 15, kq = lane >> 4;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          if (t >= 4 - p) break;
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[t][q] = Dl[(16 * p + (lane >> 4) + 4 * q) * kPL + 16 * (p + t) + rr];
        }
#pragma unroll
        for (int kk = 0; kk < 16; kk += 4) {
          const double x = -Dl[(16 * (p - 1) + kk + kq) * kPL + 16 * p + rr];  // B: column block p
#pragma unroll
          for (int t = 0; t < 3; ++t) {
            if (t >= 4 - p) break;
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, Dl[(16 * (p - 1) + kk + kq) * kPL + 16 * (p + t) + rr], acc[t], 0, 0, 0);
          }
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          if (t >= 4 - p) break;
#pragma unroll
          for (int q = 0; q < 4; ++q) Dl[(16 * p + (lane >> 4) + 4 * q) * kPL + 16 * (p + t) + rr] = acc[t][q];
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
      }
      double a[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) a[i] = Dl[(16 * p + i) * kPL + r];
      int bad = 0x7fffffff;
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const int j = 16 * p + jj;
        double d = readlane_d(a[jj], j);
        if (d <= 0.0 && bad == 0x7fffffff) bad = j + 1;
        d = d <= 0.0 ? 1.0 : d;
        const double rs = rsqrt_nr(d);
        const double lv = (r == j) ? d * rs : (r > j ? a[jj] * rs : 0.0);
        a[jj] = lv;
        if (r == j) dinv[j] = rs;
        // next pivot column first (the chain, one v_readlane), the other
        // columns off it: the column goes through LDS and comes back as
        // broadcast reads (no SGPR pressure, all reads in flight at once)
        if (jj + 1 < 16) a[jj + 1] -= lv * readlane_d(lv, j + 1);
        if (jj + 2 < 16) {
          colb[(jj & 1) * 64 + r] = lv;
#pragma unroll
          for (int i = jj + 2; i < 16; ++i) a[i] -= lv * colb[(jj & 1) * 64 + 16 * p + i];
        }
      }
      if (r == 0 && bad != 0x7fffffff) atomicMin(bad_s, bad);
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        Dl[(16 * p + i) * kPL + r] = a[i];
        if (r >= 16 * p + i) T[(size_t)(16 * p + i) * ldt + r] = a[i];  // L is final: straight out
      }
      if (stamp && lane == 0) g_potrf_stamps[3 + 2 * p] = wall_clock64();
    } else if (p >= 1) {
      // panel p-1's update of the tiles right of column block p: (R, C), p < C <= R,
      // dealt to the three other waves
      const int nt = (3 - p) * (4 - p) / 2;
      const int me = (v - p + 3) & 3;  // 0..2 among the other waves
      for (int t = me; t < nt; t += 3) {
        int R = p + 1, u = t;
        while (u > R - (p + 1)) { u -= R - p; ++R; }
        upd_tile(R, p + 1 + u, p - 1);
      }
      // off the panel chain: the wave that factored panel p-1 inverts its
      // diagonal block X_{p-1,p-1} while wave p factors panel p
      if (v == p - 1) diag_block_inverse(Dl, Xb, Xc, dinv, p - 1);
      // row p-2 of the inverse (its diagonal block was inverted one iteration
      // ago): wave j < p-2 takes X_{p-2,j}
      if (p >= 3 && v < p - 2) inv_tile(Dl, Xb, Xc, Tw + 256 * v, p - 2, v);
    }
    __syncthreads();
    PARSEC_STAMP(4 + 2 * p);
  }
  if (threadIdx.x == 0 && *bad_s != 0x7fffffff && info) atomicCAS(info, 0, info_base + *bad_s);
  // X_33 beside row 2 of the inverse and the parts of row 3 already known, then
  // the rest of row 3
  if (v == 3) diag_block_inverse(Dl, Xb, Xc, dinv, 3);
  else if (v < 2) inv_tile(Dl, Xb, Xc, Tw + 256 * v, 2, v);
  else row3_partials(Dl, Xb, Tw + 512);
  __syncthreads();
  if (v < 3) row3_finish(Dl, Xb, Xc, Tw + 256 * v, v);
  __syncthreads();
  PARSEC_STAMP(11);
  PARSEC_STAMP(12);
  // invD col-major: invD[c * 64 + r] = X(r, c), zero above the diagonal
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int c = 16 * v + k;
    invD[(size_t)c * 64 + r] = r >= c ? Xb[xblk(r >> 4, v) + (r & 15) * 16 + k] : 0.0;
  }
  PARSEC_STAMP(13);
}

// DIAG entry on the triangles: D = A_dd - P P^T with P = A_dj iD^T. iD is lower
// triangular, so column tile c of P only needs k < 16 (c + 1), and only D's 10
// lower 16 x 16 tiles are formed (the factorization never reads the others):
// 40 + 48 MFMAs on the busiest wave instead of 64 + 64 for two full 64^3
// products. On entry S0 = A_dj, S1 = iD (staged, not yet synchronised); on
// exit S1[c][r] = D(r, c) on the lower tiles, S0 free.
#ifndef PARSEC_DIAG_TRI
#define PARSEC_DIAG_TRI 1
#endif
constexpr bool g_diag_tri = PARSEC_DIAG_TRI != 0;
__device__ __forceinline__ void diag_enter_tri(Blk& S0, Blk& S1, const double* __restrict__ Add, int lda) {
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, kq = lane >> 4;
  // this wave's D tiles (row tile dm, column tile dn): 3 / 3 / 2 / 2
  int dm[3], dn[3], nd;
  if (w == 0) { dm[0] = 3; dn[0] = 0; dm[1] = 3; dn[1] = 1; dm[2] = 3; dn[2] = 2; nd = 3; }
  else if (w == 1) { dm[0] = 2; dn[0] = 0; dm[1] = 2; dn[1] = 1; dm[2] = 2; dn[2] = 2; nd = 3; }
  else if (w == 2) { dm[0] = 1; dn[0] = 0; dm[1] = 1; dn[1] = 1; dm[2] = 0; dn[2] = 0; nd = 2; }
  else { dm[0] = 0; dn[0] = 0; dm[1] = 3; dn[1] = 3; dm[2] = 0; dn[2] = 0; nd = 2; }
  double4_t dacc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int q = 0; q < 4; ++q) dacc[t][q] = t < nd ? Add[(size_t)(16 * dn[t] + kq + 4 * q) * lda + 16 * dm[t] + r] : 0.0;
  __syncthreads();  // S0, S1 staged
  // P tiles: row tiles 2 (w & 1) + {0, 1}; column tiles {0, 3} (waves 0, 1) or
  // {1, 2} (waves 2, 3): 4 (1 + 4) or 4 (2 + 3) k-steps x 2 row tiles = 40
  const int m0 = 32 * (w & 1);
  const int nc[2] = {(w >> 1) ? 1 : 0, (w >> 1) ? 2 : 3};
  double4_t p[2][2];
  acc_zero(p);
#pragma unroll
  for (int kk = 0; kk < 64; kk += 4) {
    double y[2];
#pragma unroll
    for (int jm = 0; jm < 2; ++jm) y[jm] = S0[kk + kq][m0 + 16 * jm + r];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (kk < 16 * (nc[i] + 1)) {
        const double x = S1[kk + kq][16 * nc[i] + r];
#pragma unroll
        for (int jm = 0; jm < 2; ++jm) p[i][jm] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y[jm], p[i][jm], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // every wave has read A_dj
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int jm = 0; jm < 2; ++jm)
#pragma unroll
      for (int q = 0; q < 4; ++q) S0[16 * nc[i] + kq + 4 * q][m0 + 16 * jm + r] = p[i][jm][q];  // S0[n][m] = P(m, n)
  __syncthreads();
#pragma unroll
  for (int kk = 0; kk < 64; kk += 4) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      if (t < nd) {
        const double y = S0[kk + kq][16 * dm[t] + r];
        const double x = -S0[kk + kq][16 * dn[t] + r];
        dacc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, dacc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 3; ++t)
    if (t < nd)
#pragma unroll
      for (int q = 0; q < 4; ++q) S1[16 * dn[t] + kq + 4 * q][16 * dm[t] + r] = dacc[t][q];  // S1[c][r] = D(r, c)
  __syncthreads();
}

struct PotrfStepArgs {
  double* A;
  double* W;        // optional: W = L^-1 (ldw); also holds the right-hand sides R
  double* invD;     // nb x 4096: iD_j
  int* info;
  int lda, ldw, nb; // nb = n / 64 blocks
  int stamp;        // record phase clocks of the DIAG item (diagnostics)
  int claim;        // critical-path launch: claim the CUs
  int j;            // step (-1: first launch, nb - 1: last launch)
  int pack;         // packed panel tile: W's strict upper triangle receives L^T (PotrfDesc::pack_w)
  // item ranges: [0, n_diag) DIAG, then TRAIL, RUPD, LW, XW, ZERO
  int n_diag, n_trail, n_rupd, n_lw, n_xw, n_zero, n_pack;
  // auto panel solve (optional): the items that finalize blocks of L and W fold
  // their max |.| into est[0] / est[1] (bit patterns), the last launch counts its
  // workgroups in est[2] and the last one publishes max|L| max|W| to est_host
  unsigned long long* est;
  double* est_host;
};

// max |v| of the workgroup folded into est[slot]: non-negative doubles order
// like their bit patterns (integer max); one atomic per wave
__device__ __forceinline__ void est_fold(unsigned long long* est, int slot, double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  if ((threadIdx.x & 63) == 0 && v > 0.0)
    __hip_atomic_fetch_max(est + slot, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double acc_absmax(const double4_t (&acc)[2][2]) {
  double v = 0.0;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) v = fmax(v, fabs(acc[i][j][q]));
  return v;
}
// Last launch of a tile POTRF: the workgroup that retires last publishes the
// estimate (system scope: the host reads it once the launch's event completed)
// and clears the device slots for the next factorization using them.
__device__ __forceinline__ void est_publish(const PotrfStepArgs& a) {
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  unsigned long long* e = a.est;
  const unsigned long long old = __hip_atomic_fetch_add(e + 2, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (old != (unsigned long long)gridDim.x - 1) return;
  const double mL = __longlong_as_double((long long)__hip_atomic_load(e + 0, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT));
  const double mW = __longlong_as_double((long long)__hip_atomic_load(e + 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT));
  __hip_atomic_store(e + 0, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(e + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(e + 2, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double v = mL * mW;
  if (!(v > 0.0)) v = v != v ? __builtin_huge_val() : 2.2250738585072014e-308;  // 0 means "not published"
  __hip_atomic_store(a.est_host, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Prefetch of a 64 x 64 block into registers (8 x 16 B per thread), so its
// global latency overlaps the MFMA work on the LDS buffers, then the LDS store.
struct BlkRegs {
  double2_t v[8];
};
__device__ __forceinline__ void blk_fetch(BlkRegs& R, const double* __restrict__ G, int ld) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int p = tid + 256 * e;
    R.v[e] = *reinterpret_cast<const double2_t*>(G + (size_t)(p >> 5) * ld + (p & 31) * 2);
  }
}
__device__ __forceinline__ void blk_put(Blk& S, const BlkRegs& R, bool t) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int p = tid + 256 * e;
    const int hi = p >> 5, lo = (p & 31) * 2;
    if (!t) {
      *reinterpret_cast<double2_t*>(&S[hi][lo]) = R.v[e];
    } else {
      S[lo][hi] = R.v[e].x;
      S[lo + 1][hi] = R.v[e].y;
    }
  }
}

// S[n][m] = C(m, n) (acc_to_blk operand form) -> G(n, m) = C(m, n): the block
// transposed into global memory, 16-byte stores along G's columns
__device__ __forceinline__ void blk_store_t(const Blk& S, double* __restrict__ G, int ld) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int p = tid + 256 * e;
    const int col = p >> 5, lo = (p & 31) * 2;  // G column col = C row m; G rows lo, lo + 1 = C columns
    *reinterpret_cast<double2_t*>(G + (size_t)col * ld + lo) = (double2_t){S[lo][col], S[lo + 1][col]};
  }
}

// Two 64 x 64 staging blocks (80 KB) in all: a step workgroup then fits on a CU
// next to ONE resident 128 x 128 GEMM workgroup (74 KB of LDS), so critical-path
// work starts as soon as a bulk workgroup retires instead of waiting for a CU to
// drain completely (the 120 KB version waited 1.2 ms per tile POTRF at 16k).
__device__ __forceinline__ void dpotrf_step(const PotrfStepArgs& a, double* pool);
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void dpotrf_step_kernel(const PotrfStepArgs a) {
  __shared__ double pool[2 * 64 * kPL];
  crit_claim(a.claim);
  dpotrf_step(a, pool);
  if (a.est && a.j == a.nb - 1) est_publish(a);
  crit_release(a.claim);
}
__device__ __forceinline__ void dpotrf_step(const PotrfStepArgs& a, double* pool) {
  static_assert(kDiagPoolDoubles <= 64 * kPL, "diag_factor_inv scratch exceeds one staging block");
  __builtin_amdgcn_s_setprio(2);  // the tile POTRF is the critical path
  Blk& S0 = *reinterpret_cast<Blk*>(pool);
  Blk& S1 = *reinterpret_cast<Blk*>(pool + 64 * kPL);
  const int nb = a.nb, j = a.j, lda = a.lda, ldw = a.ldw;
  double* __restrict__ A = a.A;
  auto blkA = [&](int r, int c) { return A + (size_t)(64 * c) * lda + 64 * r; };
  auto blkW = [&](int r, int c) { return a.W + (size_t)(64 * c) * ldw + 64 * r; };
  const double* iD = a.invD + (size_t)(j < 0 ? 0 : j) * 4096;
  int it = blockIdx.x;
  double4_t acc[2][2];
  // ---------------------------------------------------------------- DIAG
  if (it < a.n_diag) {
    const bool stamp = (a.stamp & 1) != 0, spread = (a.stamp & 2) != 0;
    PARSEC_STAMP(0);
    const int d = j + 1;  // block to factor (0 in the first launch)
    if (j < 0) {          // first launch: D_0 = A_00
      stage_blk(S1, blkA(0, 0), lda, false);  // S1[c][r] = D(r, c)
      __syncthreads();
    } else if (g_diag_tri) {
      stage_blk(S0, blkA(d, j), lda, false);
      stage_blk(S1, iD, 64, false);
      diag_enter_tri(S0, S1, blkA(d, d), lda);
    } else {
      acc_load(acc, blkA(d, d), lda);
      stage_blk(S0, blkA(d, j), lda, false);
      stage_blk(S1, iD, 64, false);
      __syncthreads();
      double4_t p[2][2];
      acc_zero(p);
      mma_blk(p, S0, S1, 1.0);  // P = A_dj iD^T
      __syncthreads();
      acc_to_blk(p, S0, false);  // S0 = P (operand form)
      __syncthreads();
      mma_blk(acc, S0, S0, -1.0);  // D = A_dd - P P^T
      acc_to_blk(acc, S1, false);  // S1[c][r] = D(r, c) (S1 = iD no longer read)
      __syncthreads();
    }
    diag_factor_inv(&S1[0][0], &S0[0][0], blkA(d, d), lda, a.invD + (size_t)d * 4096, a.info, 64 * d, stamp, spread);
    return;
  }
  it -= a.n_diag;
  // --------------------------------------------------------------- TRAIL
  if (it < a.n_trail) {
    // lower triangle of the (nb-1-j)^2 trailing blocks in row-major order, minus (0,0)
    const int t = it + 1;
    int rr = (int)((sqrt(8.0 * t + 1.0) - 1.0) * 0.5);
    while ((rr + 1) * (rr + 2) / 2 <= t) ++rr;
    while (rr * (rr + 1) / 2 > t) --rr;
    const int cc = t - rr * (rr + 1) / 2;
    const int r = j + 1 + rr, c = j + 1 + cc;
    BlkRegs rc;
    if (r != c) blk_fetch(rc, blkA(c, j), lda);
    acc_load(acc, blkA(r, c), lda);
    stage_blk(S0, blkA(r, j), lda, false);
    stage_blk(S1, iD, 64, false);
    __syncthreads();
    double4_t pr[2][2], pc[2][2];
    acc_zero(pr);
    mma_blk(pr, S0, S1, 1.0);  // P_r
    __syncthreads();
    if (r != c) {
      blk_put(S0, rc, false);
      __syncthreads();
      acc_zero(pc);
      mma_blk(pc, S0, S1, 1.0);  // P_c
      __syncthreads();
      acc_to_blk(pc, S1, false);
    }
    acc_to_blk(pr, S0, false);
    __syncthreads();
    mma_blk(acc, S0, r != c ? S1 : S0, -1.0);  // A_rc -= P_r P_c^T
    acc_store(acc, blkA(r, c), lda, r == c);
    return;
  }
  it -= a.n_trail;
  // ---------------------------------------------------------------- RUPD
  if (it < a.n_rupd) {
    const int rows = nb - 1 - j;
    const int r = j + 1 + it % rows, c = it / rows;  // c in [0, j]
    BlkRegs rx;
    if (c != j) blk_fetch(rx, blkW(j, c), ldw);
    acc_load(acc, blkW(r, c), ldw);
    stage_blk(S0, blkA(r, j), lda, false);
    stage_blk(S1, iD, 64, false);
    __syncthreads();
    double4_t pr[2][2], x[2][2];
    acc_zero(pr);
    mma_blk(pr, S0, S1, 1.0);  // P_r
    __syncthreads();
    if (c == j) {
      stage_blk(S1, iD, 64, true);  // X_jj = iD as the NN B operand: S1[k][n] = iD(k, n)
    } else {
      blk_put(S0, rx, true);  // R_jc as the NN B operand
      __syncthreads();
      acc_zero(x);
      mma_blk(x, S1, S0, 1.0);  // X_jc = iD R_jc  (S1[k][m] = iD(m, k))
      __syncthreads();
      acc_to_blk(x, S1, true);
    }
    acc_to_blk(pr, S0, false);
    __syncthreads();
    mma_blk(acc, S0, S1, -1.0);  // R_rc -= P_r X_jc
    acc_store(acc, blkW(r, c), ldw, false);
    return;
  }
  it -= a.n_rupd;
  // ------------------------------------------------------------------ LW
  if (it < a.n_lw) {
    const int p = j - 1, r = p + 1 + it;  // the panel of step j - 1
    stage_blk(S0, blkA(r, p), lda, false);
    stage_blk(S1, a.invD + (size_t)p * 4096, 64, false);
    __syncthreads();
    acc_zero(acc);
    mma_blk(acc, S0, S1, 1.0);
    __syncthreads();  // every wave has read S0 (a copy of the block being overwritten)
    acc_store(acc, blkA(r, p), lda, false);
    if (a.est) est_fold(a.est, 0, acc_absmax(acc));  // L(r, p) is final
    if (a.pack && j == nb - 1) {  // packed panel tile: the last panel's L(r, p)^T into W's upper block (p, r)
      acc_to_blk(acc, S0, false);
      __syncthreads();
      blk_store_t(S0, blkW(p, r), ldw);
    }
    return;
  }
  it -= a.n_lw;
  // ------------------------------------------------------------------ XW
  if (it < a.n_xw) {
    // rows [j - 1, ...] that became final: the last launch finishes two rows
    int row = j - 1, c = it;
    if (c >= row + 1) { c -= row + 1; ++row; }
    const double* iDr = a.invD + (size_t)row * 4096;
    if (c == row) {  // diagonal block: iD itself
      double* Wd = blkW(row, row);
      double mw = 0.0, ml = 0.0;
      const double* Ld = blkA(row, row);
      for (int e = threadIdx.x; e < 4096; e += 256) {
        const int rr = e & 63, cc = e >> 6;  // element (rr, cc) of the diagonal block
        const double v = iDr[e];
        // packed panel tile: the strict upper part holds L(row, row)^T
        Wd[(size_t)cc * ldw + rr] = (a.pack && rr < cc) ? Ld[(size_t)rr * lda + cc] : v;
        if (a.est) {
          mw = fmax(mw, fabs(v));
          if (rr >= cc) ml = fmax(ml, fabs(Ld[(size_t)cc * lda + rr]));  // L(row, row), lower
        }
      }
      if (a.est) {
        est_fold(a.est, 0, ml);
        est_fold(a.est, 1, mw);
      }
      return;
    }
    stage_blk(S1, iDr, 64, false);
    stage_blk(S0, blkW(row, c), ldw, true);
    __syncthreads();
    acc_zero(acc);
    mma_blk(acc, S1, S0, 1.0);
    __syncthreads();
    acc_store(acc, blkW(row, c), ldw, false);
    if (a.est) est_fold(a.est, 1, acc_absmax(acc));  // W(row, c) is final
    return;
  }
  it -= a.n_xw;
  // ---------------------------------------------------------------- ZERO
  if (it < a.n_zero) {
    const size_t nn = (size_t)64 * nb;
    for (size_t c = (size_t)it; c < nn; c += (size_t)a.n_zero)
      for (size_t r = threadIdx.x * 2; r < nn; r += 512) *reinterpret_cast<double2_t*>(a.W + c * ldw + r) = (double2_t){0.0, 0.0};
    return;
  }
  it -= a.n_zero;
  // ---------------------------------------------------------------- PACK
  // last launch of a packed panel tile: the L blocks final before it (panels
  // 0 .. nb - 3) go transposed into W's upper blocks, beside the launch's own
  // work -- off the step launches of the critical path (the last panel's block
  // is written by its LW item, the diagonal blocks by the XW items)
  if (it < a.n_pack) {
    int p = 0, rem = it;
    while (rem >= nb - 1 - p) { rem -= nb - 1 - p; ++p; }
    const int r = p + 1 + rem;
    stage_blk(S0, blkA(r, p), lda, false);
    __syncthreads();
    blk_store_t(S0, blkW(p, r), ldw);
  }
}

static int g_potrf_steps = -1;  // PARSEC_POTRF_STEPS=0 restores the 3-launches-per-64-columns tile POTRF

int potrf_steps_mode(int on) {
  const int prev = g_potrf_steps;
  if (on >= 0) g_potrf_steps = on;
  return prev;
}

bool potrf_steps_eligible(const PotrfDesc& p) {
  if (g_potrf_steps < 0) {
    const char* e = getenv("PARSEC_POTRF_STEPS");
    g_potrf_steps = e ? atoi(e) : 1;
  }
  return g_potrf_steps != 0 && p.n % 64 == 0 && p.n >= 64 && p.lda % 2 == 0 && ((uintptr_t)p.A % 16) == 0 &&
         (!p.W_out || (p.ldw % 2 == 0 && ((uintptr_t)p.W_out % 16) == 0));
}

size_t potrf_steps_workspace_bytes(const PotrfDesc& p) { return p.invD_out ? 0 : (size_t)(p.n / 64) * 4096 * sizeof(double); }

// ---------------------------------------------- host-published panel estimates
// Under PARSEC_DPOTRF_TRSM=auto the tile POTRF that writes W = L^-1 publishes
// max|L| max|W| into pinned host memory when its last step launch retires. The
// engine dispatches TRSM(m, k) only after POTRF(k)'s completion event, so the
// TRSM launch reads the estimate on the host and launches the substitution
// kernel only for the panels above the limit: no gated kernel rides the
// critical stream behind every panel GEMM. A W whose estimate is unknown here
// (factored by another process, or not yet published) takes the device-side
// gate (scan in the copy kernel, in-place gated substitution kernel).
namespace {
constexpr uint32_t kEstSlots = 4096;
struct EstimateSlots {
  std::mutex m;
  bool tried = false;
  double* host = nullptr;              // [kEstSlots], pinned; 0 = not published
  unsigned long long* dev = nullptr;   // [kEstSlots][4]: max|L|, max|W|, arrivals, pad
  const double* owner[kEstSlots] = {};
  uint32_t next = 0;
  std::unordered_map<const double*, uint32_t> of_w;
};
EstimateSlots g_est[16];
std::atomic<bool> g_est_any{false};  // some device has estimate slots (forget() is a no-op before)
int g_est_route = -1;  // PARSEC_DPOTRF_TRSM_ESTIMATE: 1 = host-published (default), 0 = device gate only
EstimateSlots* est_slots() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  return &g_est[dev];
}
}  // namespace

int trsm_estimate_route(int on) {
  if (g_est_route < 0) {
    const char* e = getenv("PARSEC_DPOTRF_TRSM_ESTIMATE");
    g_est_route = e ? (atoi(e) != 0) : 1;
  }
  const int prev = g_est_route;
  if (on >= 0) g_est_route = on != 0;
  return prev;
}

// A slot for the POTRF writing W (device / host halves), or false.
static bool est_acquire(const double* W, unsigned long long** dev, double** host) {
  if (trsm_estimate_route(-1) == 0 || parsec::trsm_inverse_mode(-1, 0.0) != 1) return false;
  EstimateSlots* e = est_slots();
  if (!e) return false;
  std::lock_guard<std::mutex> lk(e->m);
  if (!e->tried) {
    e->tried = true;
    void* h = nullptr;
    void* d = nullptr;
    if (hipHostMalloc(&h, kEstSlots * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); h = nullptr; }
    if (h && hipMalloc(&d, kEstSlots * 4 * sizeof(unsigned long long)) != hipSuccess) { (void)hipGetLastError(); d = nullptr; }
    if (h && d && hipMemset(d, 0, kEstSlots * 4 * sizeof(unsigned long long)) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
      std::memset(h, 0, kEstSlots * sizeof(double));
      e->host = static_cast<double*>(h);
      e->dev = static_cast<unsigned long long*>(d);
      g_est_any.store(true, std::memory_order_release);
    } else {
      (void)hipGetLastError();
      if (h) (void)hipHostFree(h);
      if (d) (void)hipFree(d);
    }
  }
  if (!e->host) return false;
  const uint32_t slot = e->next++ % kEstSlots;
  if (e->owner[slot]) {
    auto it = e->of_w.find(e->owner[slot]);
    if (it != e->of_w.end() && it->second == slot) e->of_w.erase(it);
  }
  e->owner[slot] = W;
  e->of_w[W] = slot;
  *reinterpret_cast<volatile double*>(&e->host[slot]) = 0.0;
  *dev = e->dev + (size_t)slot * 4;
  *host = e->host + slot;
  return true;
}

// A device buffer was (re)allocated: whatever W it held is gone, so an estimate
// keyed by its address must not be found for the next tile living there (a
// receive buffer recycled from the pool or the zone, a tile re-staged after
// eviction). Called by the zone allocator, device_alloc and the comm engine's
// receive-buffer pool.
void trsm_estimate_forget(const void* p) {
  if (!p || !g_est_any.load(std::memory_order_acquire)) return;
  for (EstimateSlots& e : g_est) {
    std::lock_guard<std::mutex> lk(e.m);
    if (!e.host) continue;
    auto it = e.of_w.find(static_cast<const double*>(p));
    if (it == e.of_w.end()) continue;
    if (e.owner[it->second] == p) e.owner[it->second] = nullptr;
    e.of_w.erase(it);
  }
}

// The published estimate of the POTRF that wrote W (> 0), or 0 when unknown.
static double est_lookup(const double* W) {
  if (trsm_estimate_route(-1) == 0) return 0.0;
  EstimateSlots* e = est_slots();
  if (!e || !e->host) return 0.0;
  std::lock_guard<std::mutex> lk(e->m);
  auto it = e->of_w.find(W);
  if (it == e->of_w.end() || e->owner[it->second] != W) return 0.0;
  const double v = *reinterpret_cast<volatile const double*>(&e->host[it->second]);
  std::atomic_thread_fence(std::memory_order_acquire);
  return v;
}

// tests: the estimate keyed by p on the current device, and every W address
// holding a published one
double trsm_estimate_lookup(const void* p) { return est_lookup(static_cast<const double*>(p)); }
std::vector<uintptr_t> trsm_estimate_known() {
  std::vector<uintptr_t> out;
  EstimateSlots* e = est_slots();
  if (!e) return out;
  std::lock_guard<std::mutex> lk(e->m);
  if (!e->host) return out;
  for (const auto& kv : e->of_w)
    if (e->owner[kv.second] == kv.first && *reinterpret_cast<volatile const double*>(&e->host[kv.second]) > 0.0) out.push_back((uintptr_t)kv.first);
  return out;
}

// Estimates published / taken on the host / left to the device gate (tests, bench)
static std::atomic<uint64_t> g_est_stats[3];

void launch_potrf_steps(const PotrfDesc& p, hipStream_t stream, double* ws) {
  PotrfStepArgs a{};
  a.A = p.A; a.lda = p.lda; a.W = p.W_out; a.ldw = p.ldw; a.info = p.info;
  a.invD = p.invD_out ? p.invD_out : ws;
  if (g_potrf_stamp_mode < 0) {
    const char* e = getenv("PARSEC_POTRF_STAMPS");
    g_potrf_stamp_mode = e ? atoi(e) : 0;
  }
  static int spread = -1;
  if (spread < 0) {
    const char* e = getenv("PARSEC_POTRF_SPREAD");
    spread = e ? atoi(e) : 1;  // profiles/r3_potrf_spread_ab.txt
  }
  a.stamp = (g_potrf_stamp_mode ? 1 : 0) | (spread ? 2 : 0);
  a.claim = t_launch_claim >= 1;
  // PARSEC_POTRF_PACK=0 (measurement only): skip the L^T half of the packed
  // tile -- the substitution routes would then read garbage
  static const bool pack_env = !getenv("PARSEC_POTRF_PACK") || atoi(getenv("PARSEC_POTRF_PACK")) != 0;
  a.pack = p.pack_w && p.W_out && pack_env ? 1 : 0;
  a.est = nullptr;
  a.est_host = nullptr;
  if (p.W_out && est_acquire(p.W_out, &a.est, &a.est_host)) g_est_stats[0].fetch_add(1, std::memory_order_relaxed);
  const int nb = p.n / 64;
  a.nb = nb;
  const bool w = p.W_out != nullptr;
  auto launch = [&](int j) {
    a.j = j;
    const int rows = nb - 1 - j;  // blocks below the diagonal of step j
    if (j < 0) {
      a.n_diag = 1; a.n_trail = 0; a.n_rupd = 0; a.n_lw = 0; a.n_xw = 0;
      a.n_zero = w ? std::min(4 * nb, 256) : 0;
    } else if (j < nb - 1) {
      a.n_diag = 1;
      a.n_trail = rows * (rows + 1) / 2 - 1;
      a.n_rupd = w ? rows * (j + 1) : 0;
      a.n_lw = j >= 1 ? nb - j : 0;
      a.n_xw = (w && j >= 1) ? j : 0;
      a.n_zero = 0;
    } else {  // last launch: the final panel and the last two X rows
      a.n_diag = 0; a.n_trail = 0; a.n_rupd = 0;
      a.n_lw = nb >= 2 ? 1 : 0;
      a.n_xw = w ? (nb >= 2 ? (nb - 1) + nb : 1) : 0;
      a.n_zero = 0;
    }
    if (j == nb - 1 && nb == 1) {  // a single block: X row 0 only
      a.n_lw = 0;
    }
    // packed tile: blocks (r, p), p <= nb - 3, r > p, in the last launch
    a.n_pack = (a.pack && j == nb - 1 && nb >= 3) ? (nb - 2) * (nb - 1) - (nb - 3) * (nb - 2) / 2 : 0;
    const int grid = a.n_diag + a.n_trail + a.n_rupd + a.n_lw + a.n_xw + a.n_zero + a.n_pack;
    if (grid > 0) hipLaunchKernelGGL(dpotrf_step_kernel, dim3(grid), dim3(256), 0, stream, a);
  };
  launch(-1);
  for (int j = 0; j < nb - 1; ++j) launch(j);
  launch(nb - 1);
}

// Workspace of a TRSM-W batch: estimate slots (2 doubles per descriptor), the
// unpacked W of every distinct packed panel tile, then the copies of the B
// tiles (reused chunk after chunk).
struct TrsmWLayout {
  size_t slots = 0, unpack = 0, copies = 0;
};
static size_t al256(size_t b) { return (b + 255) / 256 * 256; }
static TrsmWLayout trsm_w_layout(const TrsmGemmDesc* d, int n) {
  TrsmWLayout l;
  l.slots = al256((size_t)n * 2 * sizeof(double));
  std::vector<const double*> seen;
  for (int i = 0; i < n; ++i) {
    l.copies += al256((size_t)d[i].m * d[i].n * sizeof(double));
    if (!d[i].packed || std::find(seen.begin(), seen.end(), d[i].W) != seen.end()) continue;
    seen.push_back(d[i].W);
    l.unpack += al256((size_t)d[i].n * d[i].n * sizeof(double));
  }
  return l;
}
size_t trsm_w_workspace_bytes(const TrsmGemmDesc* d, int n) {
  const TrsmWLayout l = trsm_w_layout(d, n);
  return l.slots + l.unpack + l.copies;
}

// B := B W^T for every descriptor: copy the B tiles into the workspace, then one
// grouped GEMM writes B from (copy x W^T). Panel-solve modes:
//  * blocked: every panel with its factor by substitution (blocked TRSM with W's
//    diagonal 64-blocks as the inverted diagonal blocks);
//  * auto, estimate published by the local POTRF (est_lookup): the panels above
//    the limit by substitution, the others through W -- decided here, no gate;
//  * auto, estimate unknown (W from another process): the copy kernel estimates
//    each W's conditioning (max|L| * max|W|) into workspace slots, the GEMM skips
//    the panels above the limit and the in-place gated substitution kernel behind
//    it solves exactly those.
// A packed panel tile (TrsmGemmDesc::packed: W below and on the diagonal, L^T
// above -- the one tile POTRF sends) is unpacked into the workspace by the first
// copy launch: the GEMM reads W from there, the substitution reads L from the
// tile's upper part and its diagonal blocks from the unpacked W.
static const bool g_trsm_tri = !getenv("PARSEC_TRSM_TRI") || atoi(getenv("PARSEC_TRSM_TRI")) != 0;
static bool trsm_substitutable(const TrsmGemmDesc& t) {
  // the substitution kernel keeps a panel of n columns in LDS
  return t.L && t.ldl > 0 && t.n <= kTrsmMaxCols && t.n % 64 == 0 && t.ldw >= t.n;
}
static bool trsm_gateable(const TrsmGemmDesc& t) { return trsm_substitutable(t); }

// Every B tile is copied into the workspace first, W unpacked there, and the
// GEMM reads both (running it in place measured 22 % slower at config 2:
// profiles/r6_trsm_inplace.txt).
void launch_trsm_w_batch(const TrsmGemmDesc* d, int n, hipStream_t stream, double* ws) {
  const int mode = parsec::trsm_inverse_mode(-1, 0.0);
  const double limit = parsec::trsm_inverse_limit();
  const TrsmWLayout lay = trsm_w_layout(d, n);
  char* const base = reinterpret_cast<char*>(ws);
  auto* slots = reinterpret_cast<unsigned long long*>(base);
  char* up_next = base + lay.slots;
  char* const copies = base + lay.slots + lay.unpack;
  // distinct W tiles of the batch: unpacked copy (packed tiles that a
  // substitution needs), gate slot
  struct WInfo {
    const double* W;
    int ldw;
    bool packed;
    const double* Wu = nullptr;  // unpacked W (lower, zeros above): the substitution's diagonal blocks
    int ldu = 0;
    unsigned long long* slot = nullptr;
    bool unpack = false;
  };
  std::vector<WInfo> wi;
  auto info_of = [&](const TrsmGemmDesc& t) -> int {
    for (size_t i = 0; i < wi.size(); ++i)
      if (wi[i].W == t.W) return (int)i;
    wi.push_back(WInfo{t.W, t.ldw, t.packed != 0});
    if (!t.packed) { wi.back().Wu = t.W; wi.back().ldu = t.ldw; }
    return (int)wi.size() - 1;
  };
  std::vector<int> subst_i, subst_w;    // solved by substitution, decided on the host (desc, W)
  std::vector<TrsmGemmDesc> via_w;      // through W
  std::vector<uint8_t> gated;           // ... with the device-side gate
  std::vector<int> slot_of;             // via_w index -> wi index
  for (int i = 0; i < n; ++i) {
    const TrsmGemmDesc& t = d[i];
    int route = 0;  // 0 W, 1 substitution, 2 W gated on the device
    if (mode == 2 && trsm_substitutable(t)) {
      route = 1;
    } else if (mode == 1 && trsm_substitutable(t)) {
      const double e = est_lookup(t.W);
      if (e > 0.0) {
        route = e > limit ? 1 : 0;
        g_est_stats[1].fetch_add(1, std::memory_order_relaxed);
      } else if (trsm_gateable(t)) {
        route = 2;
        g_est_stats[2].fetch_add(1, std::memory_order_relaxed);
      }
    }
    const int wix = info_of(t);
    WInfo& w = wi[wix];
    if (route == 2 && !w.slot) w.slot = slots + 2 * wix;
    if (route != 0 && w.packed && !w.unpack) {  // the substitution reads W's diagonal blocks unpacked
      w.unpack = true;
      w.Wu = reinterpret_cast<const double*>(up_next);
      w.ldu = t.n;
      up_next += al256((size_t)t.n * t.n * sizeof(double));
    }
    if (route == 1) {
      subst_i.push_back(i);
      subst_w.push_back(wix);
    } else {
      via_w.push_back(t);
      gated.push_back(route == 2);
      slot_of.push_back(wix);
    }
  }
  // the GEMM reads W unpacked (lower, zeros above)
  for (WInfo& w : wi)
      if (w.packed && !w.unpack) {
        w.unpack = true;
        w.Wu = reinterpret_cast<const double*>(up_next);
        for (int i = 0; i < n; ++i)
          if (d[i].W == w.W) { w.ldu = d[i].n; up_next += al256((size_t)d[i].n * d[i].n * sizeof(double)); break; }
      }
  // estimate slots start from zero (the scan jobs max into them)
  int nslots = 0;
  for (const WInfo& w : wi) nslots += w.slot ? 1 : 0;
  if (nslots) (void)hipMemsetAsync(slots, 0, wi.size() * 2 * sizeof(unsigned long long), stream);
  // scan / unpack jobs ride the first copy launch (extra launches beyond kMaxScan)
  std::vector<int> pend_scan, pend_unpack;
  for (int j = 0; j < (int)wi.size(); ++j) {
    if (wi[j].slot) pend_scan.push_back(j);
    if (wi[j].unpack) pend_unpack.push_back(j);
  }
  auto add_jobs = [&](CopyBatchArgs& ca, int& maxc) {
    ca.nscan = 0;
    ca.nunpack = 0;
    while (!pend_scan.empty() && ca.nscan < kMaxScan) {
      const WInfo& w = wi[pend_scan.back()];
      // the descriptor data of this W (any descriptor naming it)
      const TrsmGemmDesc* t = nullptr;
      for (int i = 0; i < n && !t; ++i) if (d[i].W == w.W) t = &d[i];
      const int j = ca.nscan++;
      ca.scan_n[j] = t->n; ca.scan_ldl[j] = t->ldl; ca.scan_ldw[j] = t->ldw; ca.scan_packed[j] = t->packed;
      ca.scan_L[j] = t->L; ca.scan_W[j] = t->W; ca.scan_slot[j] = w.slot;
      maxc = std::max(maxc, t->n);
      pend_scan.pop_back();
    }
    while (!pend_unpack.empty() && ca.nunpack < kMaxScan) {
      const WInfo& w = wi[pend_unpack.back()];
      const TrsmGemmDesc* t = nullptr;
      for (int i = 0; i < n && !t; ++i) if (d[i].W == w.W) t = &d[i];
      const int j = ca.nunpack++;
      ca.up_n[j] = t->n; ca.up_ld[j] = t->ldw; ca.up_src[j] = t->W; ca.up_dst[j] = const_cast<double*>(w.Wu);
      maxc = std::max(maxc, t->n);
      pend_unpack.pop_back();
    }
  };
  // jobs that cannot wait for a chunk's copy launch: before everything else
  while (pend_scan.size() > (size_t)kMaxScan || pend_unpack.size() > (size_t)kMaxScan ||
         (via_w.empty() && (!pend_scan.empty() || !pend_unpack.empty()))) {
    CopyBatchArgs ca;
    ca.count = 0;
    ca.prio = t_launch_prio;
    int maxc = 1;
    add_jobs(ca, maxc);
    if (ca.nscan + ca.nunpack > 0)
      hipLaunchKernelGGL(copy_tiles_kernel, dim3(std::min(256, (maxc + 3) / 4), ca.nscan + ca.nunpack), dim3(256), 0, stream, ca);
  }
  for (size_t s0 = 0; s0 < via_w.size(); s0 += kMaxCopyBatch) {
    const int cnt = (int)std::min<size_t>(kMaxCopyBatch, via_w.size() - s0);
    std::vector<TrsmDesc> fb;  // gated substitution solves of this chunk
    CopyBatchArgs ca;
    ca.count = 0;
    ca.nscan = 0;
    ca.nunpack = 0;
    ca.prio = t_launch_prio;
    std::vector<GemmDesc> g(cnt);
    char* p = copies;
    int maxc = 1;
    add_jobs(ca, maxc);
    for (int i = 0; i < cnt; ++i) {
      const TrsmGemmDesc& t = via_w[s0 + i];
      const WInfo& w = wi[slot_of[s0 + i]];
      GemmDesc& e = g[i];
      const int c = ca.count++;
      ca.rows[c] = t.m; ca.cols[c] = t.n; ca.ld_src[c] = t.ldb; ca.ld_dst[c] = t.m;
      ca.src[c] = t.B; ca.dst[c] = reinterpret_cast<double*>(p);
      maxc = std::max(maxc, t.n);
      e.A = ca.dst[c]; e.lda = t.m;
      p += al256((size_t)t.m * t.n * sizeof(double));
      e.B = w.Wu; e.ldb = w.ldu;  // W unpacked (lower, zeros above)
      e.C = t.B; e.ldc = t.ldb;
      e.m = t.m; e.n = t.n; e.k = t.n;
      e.alpha = 1.0; e.beta = 0.0; e.transA = 0; e.transB = 1; e.lower_only = 0; e.a_lower = 0;  // B (L^-1)^T
      e.b_upper = g_trsm_tri ? 1 : 0;  // (L^-1)^T is upper triangular: output column block j needs k < (j+1) BN only
      e.gate = 0;
      if (gated[s0 + i]) {
        e.gate = 1;
        e.Cin = reinterpret_cast<const double*>(w.slot);  // the estimate slots (beta 0: never read as C)
        TrsmDesc x{};
        x.L = t.L; x.ldl = t.ldl; x.B = t.B; x.ldb = t.ldb; x.m = t.m; x.n = t.n; x.trans = 1;
        x.invD = w.Wu; x.invD_ld = w.ldu; x.packed = t.packed;
        x.gate = 1;
        x.gate_slot = reinterpret_cast<const double*>(w.slot);
        fb.push_back(x);
      }
    }
    if (ca.count + ca.nscan + ca.nunpack > 0)
      hipLaunchKernelGGL(copy_tiles_kernel, dim3(std::min(256, (maxc + 3) / 4), ca.count + ca.nscan + ca.nunpack), dim3(256), 0, stream, ca);
    launch_gemm_batch(g.data(), cnt, stream);
    if (!fb.empty()) {
      std::vector<const double*> inv(fb.size());
      for (size_t i = 0; i < fb.size(); ++i) inv[i] = fb[i].invD;
      launch_trsm_inv(fb.data(), inv.data(), (int)fb.size(), stream, true);
    }
  }
  if (!subst_i.empty()) {
    std::vector<TrsmDesc> subst;
    std::vector<const double*> inv;
    for (size_t k = 0; k < subst_i.size(); ++k) {
      const TrsmGemmDesc& t = d[subst_i[k]];
      const WInfo& w = wi[subst_w[k]];
      TrsmDesc x{};
      x.L = t.L; x.ldl = t.ldl; x.B = t.B; x.ldb = t.ldb; x.m = t.m; x.n = t.n; x.trans = 1;
      x.invD = w.Wu; x.invD_ld = w.ldu; x.packed = t.packed;
      subst.push_back(x);
      inv.push_back(w.Wu);
    }
    launch_trsm_inv(subst.data(), inv.data(), (int)subst.size(), stream);
  }
}

// counters: [0] estimates published by POTRF, [1] panel decisions taken on the
// host, [2] panels left to the device gate
void trsm_estimate_stats(uint64_t out[3], bool reset) {
  for (int i = 0; i < 3; ++i) out[i] = reset ? g_est_stats[i].exchange(0) : g_est_stats[i].load();
}

}  // namespace kern

namespace kern {
size_t potrf_workspace_bytes(const PotrfDesc& p);
size_t potrf_steps_workspace_bytes(const PotrfDesc& p);
bool potrf_steps_eligible(const PotrfDesc& p);
int potrf_steps_mode(int on);
void launch_potrf_steps(const PotrfDesc& p, hipStream_t stream, double* ws);
size_t trsm_w_workspace_bytes(const TrsmGemmDesc* d, int n);
void launch_trsm_w_batch(const TrsmGemmDesc* d, int n, hipStream_t stream, double* ws);
void launch_qr_panel(const QrPanelDesc* descs, int n, hipStream_t stream);
void launch_stencil7_batch(const StencilDesc* d, int n, hipStream_t stream);
void launch_qr_panel_blocked(const QrPanelDesc* descs, int n, hipStream_t stream, double* ws);
size_t qr_panel_workspace_bytes(const QrPanelDesc* descs, int n);
void launch_qr_apply(const QrApplyDesc* descs, int n, hipStream_t stream, double* ws);
size_t qr_apply_workspace_bytes(const QrApplyDesc* descs, int n);
}  // namespace kern

size_t kernel_batch_workspace_bytes(const KernelBatch& b) {
  size_t w = 0;
  for (auto& p : b.potrf) w = std::max(w, kern::potrf_steps_eligible(p) ? kern::potrf_steps_workspace_bytes(p) : kern::potrf_workspace_bytes(p));
  for (auto& g : b.getrf) w = std::max(w, kern::getrf_workspace_bytes(g));
  if (!b.lu_panel.empty()) w = std::max(w, kern::lu_panel_workspace_bytes());
  for (auto& t : b.trtri) w = std::max(w, kern::trtri_workspace_bytes(t));
  for (auto& l : b.lauum) w = std::max(w, kern::lauum_workspace_bytes(l));
  if (!b.trsm_w.empty()) w = std::max(w, kern::trsm_w_workspace_bytes(b.trsm_w.data(), (int)b.trsm_w.size()));
  if (!b.qr_panel.empty()) w = std::max(w, kern::qr_panel_workspace_bytes(b.qr_panel.data(), (int)b.qr_panel.size()));
  w = std::max(w, kern::trsm_workspace_bytes(b.trsm.data(), (int)b.trsm.size()));
  w = std::max(w, kern::trsm_left_workspace_bytes(b.trsm_left.data(), (int)b.trsm_left.size()));
  return std::max(w, kern::qr_apply_workspace_bytes(b.qr_apply.data(), (int)b.qr_apply.size()));
}

void launch_kernel_batch(KernelBatch& b, hipStream_t stream, int device_ordinal, void* ws) {
  (void)device_ordinal;
  struct PrioScope {
    int prev, prev_pad, prev_claim, prev_yield;
    PrioScope(bool on, int pad, int claim, bool yield)
        : prev(kern::t_launch_prio), prev_pad(kern::t_launch_pad), prev_claim(kern::t_launch_claim), prev_yield(kern::t_launch_yield) {
      kern::t_launch_prio = on ? 1 : 0;
      kern::t_launch_pad = pad;
      kern::t_launch_claim = claim;
      kern::t_launch_yield = yield ? 1 : 0;
    }
    ~PrioScope() {
      kern::t_launch_prio = prev;
      kern::t_launch_pad = prev_pad;
      kern::t_launch_claim = prev_claim;
      kern::t_launch_yield = prev_yield;
    }
  } prio_scope(b.critical, b.one_per_cu ? kern::kBulkPadBytes : 0, b.claim_cus, b.bulk_yield);
  // critical-path kernels first: a POTRF's fused update, POTRF, then TRSM, then the GEMM/SYRK updates
  if (!b.pre_gemm.empty()) kern::launch_gemm_batch(b.pre_gemm.data(), (int)b.pre_gemm.size(), stream);
  for (auto& p : b.potrf) {
    if (kern::potrf_steps_eligible(p)) kern::launch_potrf_steps(p, stream, static_cast<double*>(ws));
    else kern::launch_potrf(p, stream, static_cast<double*>(ws));
  }
  for (auto& g : b.getrf) kern::launch_getrf_nopiv(g, stream, static_cast<double*>(ws));
  for (auto& g : b.lu_panel) kern::launch_lu_panel(g, stream, static_cast<double*>(ws), kern::t_launch_prio);
  if (!b.qr_panel.empty()) kern::launch_qr_panel_blocked(b.qr_panel.data(), (int)b.qr_panel.size(), stream, static_cast<double*>(ws));
  if (!b.trsm.empty()) kern::launch_trsm_batch(b.trsm.data(), (int)b.trsm.size(), stream, static_cast<double*>(ws));
  if (!b.trsm_w.empty()) kern::launch_trsm_w_batch(b.trsm_w.data(), (int)b.trsm_w.size(), stream, static_cast<double*>(ws));
  // GESSM / SSSSM: the interchanges, then the unit lower solves; their updates are GEMMs
  if (!b.laswp.empty()) kern::launch_laswp_batch(b.laswp.data(), (int)b.laswp.size(), stream, kern::t_launch_prio);
  if (!b.trsm_left.empty()) kern::launch_trsm_left_batch(b.trsm_left.data(), (int)b.trsm_left.size(), stream, static_cast<double*>(ws));
  if (!b.qr_apply.empty()) kern::launch_qr_apply(b.qr_apply.data(), (int)b.qr_apply.size(), stream, static_cast<double*>(ws));
  // the inverse kernels (DTRTRI / DLAUUM): a round's TRMMs are one grouped launch
  for (auto& t : b.trtri) kern::launch_trtri(t, stream, static_cast<double*>(ws));
  if (!b.trmm.empty()) kern::launch_trmm_lt_batch(b.trmm.data(), (int)b.trmm.size(), stream);
  for (auto& l : b.lauum) kern::launch_lauum(l, stream, static_cast<double*>(ws));
  if (!b.gemm.empty()) kern::launch_gemm_batch(b.gemm.data(), (int)b.gemm.size(), stream);
  if (!b.stencil.empty()) kern::launch_stencil7_batch(b.stencil.data(), (int)b.stencil.size(), stream);
  for (auto& g : b.generic) g(stream);
}

// Device-to-device byte copy as a kernel (16-byte vectors, grid-stride): used for
// pulls from peer-process (IPC) allocations so the copy is an ordinary kernel in
// stream order on this process's queue.
__global__ __launch_bounds__(256) void copy_bytes_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
__global__ void copy_tail_kernel(char* __restrict__ dst, const char* __restrict__ src, size_t n) {
  for (size_t i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}

int device_copy_kernel(void* dst, const void* src, size_t bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const bool aligned = ((uintptr_t)dst % 16 == 0) && ((uintptr_t)src % 16 == 0);
  size_t n16 = aligned ? bytes / 16 : 0;
  if (n16) {
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (n16 + 255) / 256);
    hipLaunchKernelGGL(copy_bytes_kernel, dim3(blocks), dim3(256), 0, s, static_cast<uint4*>(dst), static_cast<const uint4*>(src), n16);
  }
  const size_t done = n16 * 16;
  if (bytes > done) hipLaunchKernelGGL(copy_tail_kernel, dim3(1), dim3(256), 0, s, static_cast<char*>(dst) + done, static_cast<const char*>(src) + done, bytes - done);
  return (int)hipGetLastError();
}

// Multi-source gather: ONE launch moves up to kMaxGather transfers, each from
// another peer's IPC mapping. Across xGMI every peer GPU sits behind its own
// link, so the transfers of one launch pull over up to 7 links at once while
// the process keeps one copy stream (one hardware queue). Workgroups are split
// between the transfers in proportion to their size (at most 64 per transfer,
// 4 x 16-byte loads in flight per thread: ~1 MiB in flight per link).
constexpr int kMaxGather = 16;
struct GatherArgs {
  int count;
  int wg_start[kMaxGather + 1];
  uint4* dst[kMaxGather];
  const uint4* src[kMaxGather];
  unsigned long long n16[kMaxGather];
};
static_assert(sizeof(GatherArgs) <= 4096, "GatherArgs exceeds the kernel argument limit");
__global__ __launch_bounds__(256) void gather_kernel(const GatherArgs a) {
  int t = 0;
  while (t + 1 < a.count && (int)blockIdx.x >= a.wg_start[t + 1]) ++t;
  const int w = (int)blockIdx.x - a.wg_start[t], nw = a.wg_start[t + 1] - a.wg_start[t];
  uint4* __restrict__ d = a.dst[t];
  const uint4* __restrict__ s = a.src[t];
  const size_t n = a.n16[t], stride = (size_t)nw * 256;
  size_t i = (size_t)w * 256 + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    const uint4 v0 = s[i], v1 = s[i + stride], v2 = s[i + 2 * stride], v3 = s[i + 3 * stride];
    d[i] = v0;
    d[i + stride] = v1;
    d[i + 2 * stride] = v2;
    d[i + 3 * stride] = v3;
  }
  for (; i < n; i += stride) d[i] = s[i];
}

int device_gather_kernel(void* const* dst, const void* const* src, const size_t* bytes, int n, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n;) {
    GatherArgs a{};
    int wg = 0;
    for (; i < n && a.count < kMaxGather; ++i) {
      const bool aligned = ((uintptr_t)dst[i] % 16 == 0) && ((uintptr_t)src[i] % 16 == 0) && bytes[i] % 16 == 0;
      if (!aligned || bytes[i] == 0) {  // odd sizes / offsets: a copy kernel of its own, same stream
        if (bytes[i] && device_copy_kernel(dst[i], src[i], bytes[i], stream) != 0) return -1;
        continue;
      }
      const int k = a.count++;
      a.dst[k] = static_cast<uint4*>(dst[i]);
      a.src[k] = static_cast<const uint4*>(src[i]);
      a.n16[k] = bytes[i] / 16;
      a.wg_start[k] = wg;
      wg += (int)std::min<size_t>(64, std::max<size_t>(1, a.n16[k] / (256 * 16)));
    }
    if (!a.count) continue;
    a.wg_start[a.count] = wg;
    hipLaunchKernelGGL(gather_kernel, dim3(wg), dim3(256), 0, st, a);
  }
  return (int)hipGetLastError();
}

// Panel-solve mode of the tile Cholesky (device.hpp trsm_inverse_mode).
// PARSEC_DPOTRF_TRSM = inverse | auto | blocked, PARSEC_DPOTRF_TRSM_LIMIT = the
// estimate above which auto solves by substitution (scripts/trsm_inverse_numerics.py,
// profiles/r4_trsm_inverse_numerics.txt).
static std::atomic<int> g_trsm_mode{-1};
static std::atomic<double> g_trsm_limit{0.0};
static void trsm_mode_init() {
  static std::once_flag once;
  std::call_once(once, [] {
    int m = 1;
    if (const char* e = getenv("PARSEC_DPOTRF_TRSM")) m = !strcmp(e, "inverse") ? 0 : !strcmp(e, "blocked") ? 2 : 1;
    double lim = 1e6;
    if (const char* e = getenv("PARSEC_DPOTRF_TRSM_LIMIT")) lim = atof(e);
    int exp = -1;
    g_trsm_mode.compare_exchange_strong(exp, m);
    double z = 0.0;
    g_trsm_limit.compare_exchange_strong(z, lim > 0 ? lim : 1e6);
  });
}
int trsm_inverse_mode(int mode, double limit) {
  trsm_mode_init();
  const int prev = g_trsm_mode.load();
  if (mode >= 0) g_trsm_mode.store(mode);
  if (limit > 0) g_trsm_limit.store(limit);
  return prev;
}
double trsm_inverse_limit() {
  trsm_mode_init();
  return g_trsm_limit.load(std::memory_order_relaxed);
}

}  // namespace parsec

// ------------------------------------------------- C entry points (tests/bench)
namespace {
std::mutex g_ws_m;
void* g_ws = nullptr;
size_t g_ws_bytes = 0;
void* test_ws(size_t bytes) {
  std::lock_guard<std::mutex> g(g_ws_m);
  if (g_ws_bytes < bytes) {
    (void)hipDeviceSynchronize();
    if (g_ws) (void)hipFree(g_ws);
    (void)hipMalloc(&g_ws, bytes);
    g_ws_bytes = bytes;
  }
  return g_ws;
}
}  // namespace

extern "C" {
int parsec_amd_gemm_tile_policy(int p) { return parsec::kern::gemm_tile_policy(p); }
int parsec_amd_gemm_splitk(int on) { return parsec::kern::gemm_splitk(on); }
int parsec_amd_gemm_mainloop(int mode) { return parsec::kern::gemm_mainloop(mode); }
int parsec_amd_gemm_pipeline(int mode) { return parsec::kern::gemm_pipeline(mode); }
int parsec_amd_dgemm_batch(const parsec::GemmDesc* descs, int n, void* stream) {
  // PARSEC_GEMM_PAD_TEST=1: launch like a DPOTRF bulk stream (padded LDS: one
  // 128x128 workgroup per CU) -- kernel benchmarks of the in-DAG regime
  const int prev = parsec::kern::t_launch_pad;
  if (parsec::kern::gemm_policy().pad_test) parsec::kern::t_launch_pad = parsec::kern::kBulkPadBytes;
  parsec::kern::launch_gemm_batch(descs, n, (hipStream_t)stream);
  parsec::kern::t_launch_pad = prev;
  return (int)hipGetLastError();
}
// Test hook, like PARSEC_GEMM_PAD_TEST above and not part of the public
// interface (include/parsec.h): the same launch as a bulk stream of an engine
// with cu_yield on issues it, i.e. the workgroups poll their CU's claim count
// once per k-tile (tests/test_gemm_pipeline_gpu.py)
int parsec_amd_dgemm_batch_yield(const parsec::GemmDesc* descs, int n, void* stream) {
  const int prev = parsec::kern::t_launch_yield;
  parsec::kern::t_launch_yield = 1;
  const int rc = parsec_amd_dgemm_batch(descs, n, stream);
  parsec::kern::t_launch_yield = prev;
  return rc;
}
// BLAS-style single DGEMM, C = alpha op(A) op(B) + beta C, column major, on
// `stream` (the signature a BODY dyld= or a DTD chore calls; reference
// stress.jdf resolves cublasDgemm the same way). Returns a hipError_t.
int parsec_amd_dgemm(char transa, char transb, int m, int n, int k, double alpha, const double* A, int lda, const double* B, int ldb, double beta,
                     double* C, int ldc, void* stream) {
  parsec::GemmDesc d{};
  d.A = A; d.B = B; d.C = C;
  d.m = m; d.n = n; d.k = k;
  d.lda = lda; d.ldb = ldb; d.ldc = ldc;
  d.alpha = alpha; d.beta = beta;
  d.transA = (transa == 'T' || transa == 't' || transa == 'C' || transa == 'c');
  d.transB = (transb == 'T' || transb == 't' || transb == 'C' || transb == 'c');
  if (m <= 0 || n <= 0) return 0;
  return parsec_amd_dgemm_batch(&d, 1, stream);
}
int parsec_amd_dtrsm_batch(const parsec::TrsmDesc* descs, int n, void* stream) {
  void* ws = test_ws(parsec::kern::trsm_workspace_bytes(descs, n) + 64);
  parsec::kern::launch_trsm_batch(descs, n, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
// B := alpha op(L)^-1 B for a batch; descriptors without invD get their
// diagonal-block inverses computed into cached scratch
int parsec_amd_dtrsm_left_batch(const parsec::TrsmLeftDesc* descs, int n, void* stream) {
  void* ws = test_ws(parsec::kern::trsm_left_workspace_bytes(descs, n) + 64);
  parsec::kern::launch_trsm_left_batch(descs, n, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
int parsec_amd_dpotrf_tile(double* A, int n, int lda, int* info, void* stream) {
  parsec::PotrfDesc p{A, n, lda, info};
  if (parsec::kern::potrf_steps_eligible(p)) {
    void* ws = test_ws(parsec::kern::potrf_steps_workspace_bytes(p) + 64);
    parsec::kern::launch_potrf_steps(p, (hipStream_t)stream, static_cast<double*>(ws));
    return (int)hipGetLastError();
  }
  void* ws = test_ws(4096 * sizeof(double));
  parsec::kern::launch_potrf(p, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
// Tile LU without pivoting; invL / invU (optional) receive the diagonal-block inverses
int parsec_amd_dgetrf_nopiv_tile(double* A, int n, int lda, int* info, double* invL, double* invU, void* stream) {
  parsec::GetrfDesc g{A, n, lda, info, invL, invU};
  void* ws = test_ws(parsec::kern::getrf_workspace_bytes(g) + 64);
  parsec::kern::launch_getrf_nopiv(g, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
// Tile TRTRI (lower, non-unit): A := L^-1 in place, or W (ld ldw) := L^-1
int parsec_amd_dtrtri_tile(double* A, int n, int lda, int* info, int info_base, double* W, int ldw, void* stream) {
  parsec::TrtriDesc t{A, n, lda, info, info_base, W, ldw, nullptr};
  void* ws = test_ws(parsec::kern::trtri_workspace_bytes(t) + 64);
  parsec::kern::launch_trtri(t, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
// B := alpha L^T B for a batch, one grouped launch
int parsec_amd_dtrmm_lt_batch(const parsec::TrmmDesc* descs, int n, void* stream) {
  parsec::kern::launch_trmm_lt_batch(descs, n, (hipStream_t)stream);
  return (int)hipGetLastError();
}
// Tile LAUUM: A := lower(L^T L) in place
int parsec_amd_dlauum_tile(double* A, int n, int lda, void* stream) {
  parsec::LauumDesc l{A, n, lda};
  void* ws = test_ws(parsec::kern::lauum_workspace_bytes(l) + 64);
  parsec::kern::launch_lauum(l, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
// Tile Cholesky that also writes W = L^-1 (ld ldw)
int parsec_amd_dpotrf_tile_w(double* A, int n, int lda, int* info, double* W, int ldw, void* stream, int pack) {
  parsec::PotrfDesc p{A, n, lda, info};
  p.W_out = W;
  p.ldw = ldw;
  p.pack_w = pack ? 1 : 0;
  if (parsec::kern::potrf_steps_eligible(p)) {
    void* ws = test_ws(parsec::kern::potrf_steps_workspace_bytes(p) + 64);
    parsec::kern::launch_potrf_steps(p, (hipStream_t)stream, static_cast<double*>(ws));
    return (int)hipGetLastError();
  }
  void* ws = test_ws(parsec::kern::potrf_workspace_bytes(p));
  parsec::kern::launch_potrf(p, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
// Phase clocks of the last stamped diagonal factorization (PARSEC_POTRF_STAMPS=1)
int parsec_amd_potrf_stamps(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(parsec::kern::g_potrf_stamps), sizeof(long long) * 16, 0, hipMemcpyDeviceToHost);
}
// Select the tile POTRF: 1 = n/64 + 1 fused step launches (default), 0 = the
// 3-launches-per-64-columns path; < 0 queries. Returns the previous setting.
int parsec_amd_potrf_steps(int on) {
  parsec::kern::potrf_steps_eligible(parsec::PotrfDesc{nullptr, 0, 0, nullptr});
  const int prev = parsec::kern::potrf_steps_mode(on);
  return prev;
}
// B := B W^T for a batch (the DPOTRF panel solve through the inverse)
int parsec_amd_trsm_w_batch(const parsec::TrsmGemmDesc* d, int n, void* stream) {
  void* ws = test_ws(parsec::kern::trsm_w_workspace_bytes(d, n) + 64);
  parsec::kern::launch_trsm_w_batch(d, n, (hipStream_t)stream, static_cast<double*>(ws));
  return (int)hipGetLastError();
}
}
