// CDNA4 (gfx950) fp64 kernels that invert with the Cholesky factor (DTRTRI /
// DLAUUM / DPOTRI): tile TRTRI, the grouped TRMM B := alpha L^T B and tile LAUUM.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_helpers.hpp"
#include "kernels.hpp"
#include "launch_settings.hpp"

namespace parsec {
namespace kern {

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
    a.prio = launch_settings().prio;
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

}  // namespace kern
}  // namespace parsec
