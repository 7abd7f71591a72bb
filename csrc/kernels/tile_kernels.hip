// CDNA4 (gfx950) fp64 kernels that share the per-CU claim table g_crit_cu: the
// grouped DGEMM with its launcher, the two tile POTRFs and the W-GEMM panel
// solve. The other families live beside it: trsm_kernels.hip (TRSM, diagonal
// block inverses), lu_kernels.hip, inverse_kernels.hip (TRTRI / TRMM / LAUUM),
// copy_kernels.hip; the host-only parts in gemm_plan.cpp (launch planner),
// trsm_estimate.cpp, kernel_batch.cpp (batch dispatcher) and kernel_capi.cpp
// (C entry points); shared device helpers in device_helpers.hpp.
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
//  * POTRF of a tile: per 64-column block, ONE wave factors the diagonal block
//    (row per lane in registers, column broadcast through LDS, no block barriers)
//    and inverts it, then the panel TRSM and the lower-only GEMM update run
//    stream-ordered.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "device_helpers.hpp"
#include "kernels.hpp"
#include "launch_settings.hpp"

namespace parsec {
namespace kern {

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

// ---- Cooperative CU yield. A critical-path workgroup (tile POTRF step, the
// critical TRSM / SYRK GEMMs) counts itself into g_crit_cu[its CU] while it
// runs; a bulk GEMM workgroup on the same CU polls that count once per k-tile
// and sleeps while it is non-zero, so the critical workgroup gets the CU's MFMA
// / LDS / issue bandwidth to itself (beside bulk waves it ran 2-4x slower:
// profiles/r4_chain16_breakdown.txt). Only the CUs that host critical work
// pause; a pause is bounded (kYieldMaxPolls) so a stale count can never stall
// bulk work. One counter per CU: XCC id x (CU, SH, SE) bits of HW_ID.
// The grouped DGEMM kernel and the tile-POTRF step kernel address the table by
// symbol, and the build has no relocatable device code: that is why they (and
// the launchers around them) share this translation unit. Handing the table to
// the step kernel by pointer, as the QR kernels take it (crit_cu_table), would
// change two hot kernels.
__device__ int g_crit_cu[8 * 256];

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

// The diagonal-block kernels stay in one translation unit: the tile POTRF's
// and the lower non-unit inverse share the LDS variables of one block_potrf64
// instantiation, and the compiler lays these out per module -- apart, both
// compile to different code (profiles/kernel_layer_split.txt).
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

// resident 128x128 workgroups of the launch being issued: half when bulk
// launches are padded to one workgroup per CU (LaunchSettings::pad)
static int gemm_slots() {
  static const int device_slots = [] {
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) return 2 * ncu;
    return 512;
  }();
  const int slots = gemm_policy().slots > 0 ? gemm_policy().slots : device_slots;
  return launch_settings().pad ? std::max(1, slots / 2) : slots;
}

// Issues the plan: every launch is driven by its record, and the record is
// what the launch log keeps.
void launch_gemm_batch(const GemmDesc* descs, int n, hipStream_t stream) {
  const LaunchSettings& ls = launch_settings();
  const GemmPlanEnv env{gemm_policy(), gemm_slots(), ls.pad, ls.yield != 0, ls.claim >= 2};
  std::vector<GemmDesc> sorted;
  for (const GemmLaunch& l : gemm_plan(descs, n, env, sorted)) {
    const GemmLaunchRecord& r = l.rec;
    GemmBatchArgs a;
    a.count = r.descs;
    a.prio = ls.prio;
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
    gemm_launch_log_append(r);
    if (r.bm == 128) launch_gemm_shape<128, 128, 16, 2, 4>(r, a, stream);
    else launch_gemm_shape<64, 64, 16, 2, 2>(r, a, stream);
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

void launch_lower_inverse(const double* L, int lda, int n, const double* invD, double* X, int ldx, double* tmp, hipStream_t stream) {
  const int nblk = (n + 63) / 64;
  (void)hipMemset2DAsync(X, (size_t)ldx * sizeof(double), 0, (size_t)n * sizeof(double), n, stream);
  for (int b0 = 0; b0 < nblk; b0 += kMaxCopyBatch) {
    CopyBatchArgs ca;
    ca.count = std::min(kMaxCopyBatch, nblk - b0);
    ca.prio = launch_settings().prio;
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
  a.claim = launch_settings().claim >= 1;
  // PARSEC_POTRF_PACK=0 (measurement only): skip the L^T half of the packed
  // tile -- the substitution routes would then read garbage
  static const bool pack_env = !getenv("PARSEC_POTRF_PACK") || atoi(getenv("PARSEC_POTRF_PACK")) != 0;
  a.pack = p.pack_w && p.W_out && pack_env ? 1 : 0;
  a.est = nullptr;
  a.est_host = nullptr;
  if (p.W_out && trsm_estimate_acquire(p.W_out, &a.est, &a.est_host)) trsm_estimate_count(0);
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
//  * auto, estimate published by the local POTRF (trsm_estimate_lookup): the panels above
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
      const double e = trsm_estimate_lookup(t.W);
      if (e > 0.0) {
        route = e > limit ? 1 : 0;
        trsm_estimate_count(1);
      } else if (trsm_gateable(t)) {
        route = 2;
        trsm_estimate_count(2);
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
    ca.prio = launch_settings().prio;
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
    ca.prio = launch_settings().prio;
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

// Phase clocks of the last stamped diagonal factorization (PARSEC_POTRF_STAMPS=1)
int potrf_stamps_read(long long* out) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_potrf_stamps), sizeof(long long) * 16, 0, hipMemcpyDeviceToHost);
}

}  // namespace kern
}  // namespace parsec
