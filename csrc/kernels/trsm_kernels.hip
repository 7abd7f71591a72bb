// CDNA4 (gfx950) fp64 triangular solves of a tile.
//  * TRSM (B := B L^-T, right/lower/trans) = blocked MFMA solve with precomputed
//    inverses of the 64x64 diagonal blocks: R_j = B_j - X_<j L_j,<j^T ; X_j = R_j invD_j^T.
//    Each workgroup owns 16 rows and keeps its row panel in LDS with a stride of 16
//    doubles, which makes every MFMA operand read bank-conflict free.
//  * Left-side solves (B := alpha op(L)^-1 B, lower or upper, unit or not, and
//    their right-side transposes): one workgroup per 16 columns of B.
// The inverses come from launch_trtri_diag / launch_trtri_diag_upper (tile_kernels.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_helpers.hpp"
#include "kernels.hpp"
#include "launch_settings.hpp"

namespace parsec {
namespace kern {

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

static constexpr int kTrsmRows = 16;

// invD[i] must already hold the inverted diagonal blocks of descs[i].L.
// in_place: the small-LDS variant (every n a multiple of 64; see dtrsm_inv_kernel)
void launch_trsm_inv(const TrsmDesc* descs, const double* const* invD, int n, hipStream_t stream, bool in_place) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute((const void*)dtrsm_inv_kernel<kTrsmRows, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    attr = true;
  }
  for (int s0 = 0; s0 < n; s0 += kMaxTrsmBatch) {
    int cnt = std::min(kMaxTrsmBatch, n - s0);
    TrsmInvArgs a;
    a.count = cnt;
    a.prio = launch_settings().prio;
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
    launch_trtri_diag(descs[i].L, descs[i].ldl, descs[i].n, blk, stream);
    seen.emplace_back(descs[i].L, blk);
    inv[i] = blk;
  }
  launch_trsm_inv(descs, inv.data(), n, stream);
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
      a.prio = launch_settings().prio;
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

}  // namespace kern
}  // namespace parsec
