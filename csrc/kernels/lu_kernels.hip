// CDNA4 (gfx950) kernels of the tile LU with incremental (pairwise) pivoting
// (dgetrf_incpiv.jdf / dgetrs_incpiv.jdf): the pivoted factorization of a tile
// (GETRF) or of an upper triangle stacked on a tile (TSTRF), and the grouped row
// interchanges of GESSM / SSSSM. The solves and updates of those tasks are the
// left-side tile solve and the grouped DGEMM of tile_kernels.hip.
//
// Factorization, blocked by 64 columns. Per strip j (w <= 64 columns):
//   dlu_strip_kernel     ONE workgroup factors the strip with partial pivoting.
//                        Candidates: the w rows of the diagonal block and every
//                        row below (GETRF: the rest of the tile; TSTRF: the
//                        bottom tile -- the rows of the top tile below the
//                        diagonal block are zero in these columns and stay so).
//   dlaswp_pair_kernel   the strip's interchanges on the columns left (L) and
//                        right of it
//   dtrsm_left_kernel    the block row right of it, with the unit lower block
//   the grouped NN GEMM  the rows below, right of the strip
// Nothing waits for another workgroup: the launches are stream-ordered and the
// strip kernel is a single workgroup with block barriers only.
//
// Strip kernel layout. 256 threads; the strip goes through in sub-strips of 16
// columns. A thread owns rows tid, tid + 256, .. (RPT of them: 1, 2, 3 or 5, for
// up to 64 + 1024 = 1088 stacked rows) and holds their 16 sub-strip entries in
// registers: 32 RPT VGPRs (160 at RPT = 5), under the 256 a one-wave-per-SIMD
// workgroup may use beside one resident 128 x 128 GEMM workgroup (4 waves of at
// most 256). Per column: the argmax of |x| (in-register, wave butterfly, one
// exchange of the 4 wave results through LDS), the pivot row and the diagonal
// row trade places through a 2 x 16 LDS buffer, every row below takes its
// multiple of the pivot row from that buffer: two barriers per column. After a
// sub-strip the other columns of the strip are brought up to date in global
// memory (L2-resident): interchanges, the 16-row triangular solve (a column per
// thread), then the rank-16 update of the rows below with the multipliers still
// in registers and the solved rows in LDS. LDS: 11 KB.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <utility>

#include "../device/device.hpp"

namespace parsec {
namespace kern {

void launch_gemm_batch(const GemmDesc* descs, int n, hipStream_t stream);                             // tile_kernels.hip
void launch_trsm_left_batch(const TrsmLeftDesc* descs, int n, hipStream_t stream, double* ws);        // tile_kernels.hip

constexpr int kLuThreads = 256;
constexpr int kLuSub = 16;

struct LuStripArgs {
  double* Tp;   // the diagonal block (w x w): its upper triangle lives here
  double* Lp;   // ... and its strict lower triangle here (GETRF: == Tp)
  double* Bp;   // the hb rows below, first column of the strip
  double* piv;  // the strip's w pivots
  int* info;
  int ldt, ldl, ldb;
  int w, hb;
  int zero_rows;  // TSTRF: rows of L (from the diagonal block down) whose strict lower part is cleared first
  int piv_top;    // pivot value of diagonal-block row r: piv_top + r + 1
  int piv_bot;    // ... of row i below: piv_bot + i + 1
  int info_base;
  int prio;
};

template <int RPT>
__global__ __launch_bounds__(kLuThreads) __attribute__((amdgpu_waves_per_eu(2))) void dlu_strip_kernel(const LuStripArgs a) {
  __shared__ double red_v[kLuThreads / 64];
  __shared__ int red_r[kLuThreads / 64];
  __shared__ double rowbuf[2][kLuSub];     // [0]: the diagonal row, [1]: the pivot row
  __shared__ double Ls[kLuSub][kLuSub + 1];  // the sub-strip's diagonal block (multipliers below its diagonal)
  __shared__ double U12[kLuSub][64];       // the solved rows right of the sub-strip
  __shared__ int pivl[64];                 // pivot rows of the strip (stacked row index)
  if (a.prio) __builtin_amdgcn_s_setprio(2);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = a.w, rows = a.w + a.hb;
  // entry (r, c) of the stacked strip: r < w a row of the diagonal block
  auto at = [&](int r, int c) -> double* {
    if (r < w) return c >= r ? a.Tp + (size_t)c * a.ldt + r : a.Lp + (size_t)c * a.ldl + r;
    return a.Bp + (size_t)c * a.ldb + (r - w);
  };
  if (a.zero_rows > 0) {
    for (int idx = tid; idx < w * a.zero_rows; idx += kLuThreads) {
      const int c = idx / a.zero_rows, r = idx - c * a.zero_rows;
      if (r > c) a.Lp[(size_t)c * a.ldl + r] = 0.0;
    }
    __syncthreads();
  }
#pragma unroll 1
  for (int c0 = 0; c0 < w; c0 += kLuSub) {
    const int cw = min(kLuSub, w - c0);
    double x[RPT][kLuSub];
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int rl = tid + kLuThreads * q;
#pragma unroll
      for (int i = 0; i < kLuSub; ++i) x[q][i] = (rl >= c0 && rl < rows && i < cw) ? *at(rl, c0 + i) : 0.0;
    }
    // one column; c is a compile-time constant so that x stays in registers
    auto column = [&](auto cidx) {
      constexpr int c = decltype(cidx)::value;
      {  // a column past a ragged strip's end holds zeros: it keeps its row, divides nothing, and is never stored
        const int cc = c0 + c;
        // the candidate of largest magnitude, the smallest row among equals
        double best = -1.0;
        int brow = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
          const int rl = tid + kLuThreads * q;
          const double v = __builtin_fabs(x[q][c]);
          if (rl >= cc && rl < rows && v > best) { best = v; brow = rl; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double ob = __shfl_xor(best, off);
          const int orow = __shfl_xor(brow, off);
          if (ob > best || (ob == best && orow < brow)) { best = ob; brow = orow; }
        }
        if (lane == 0) { red_v[wave] = best; red_r[wave] = brow; }
        __syncthreads();
        best = red_v[0];
        brow = red_r[0];
#pragma unroll
        for (int k = 1; k < kLuThreads / 64; ++k) {
          const double ob = red_v[k];
          const int orow = red_r[k];
          if (ob > best || (ob == best && orow < brow)) { best = ob; brow = orow; }
        }
        // every candidate exactly zero: the row itself is the pivot, nothing is divided
        const bool zero = !(best > 0.0);
        const int prow = zero ? cc : brow;
        if (tid == 0) {
          pivl[cc] = prow;
          if (zero && a.info && cc < w) {
            const int val = a.info_base + cc + 1;
            const int old = atomicCAS(a.info, 0, val);
            if (old != 0 && val < old) atomicMin(a.info, val);
          }
        }
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
          const int rl = tid + kLuThreads * q;
          if (rl == cc) {
#pragma unroll
            for (int i = 0; i < kLuSub; ++i) rowbuf[0][i] = x[q][i];
          }
          if (rl == prow) {
#pragma unroll
            for (int i = 0; i < kLuSub; ++i) rowbuf[1][i] = x[q][i];
          }
        }
        __syncthreads();
        const double d = rowbuf[1][c];
#pragma unroll
        for (int q = 0; q < RPT; ++q) {
          const int rl = tid + kLuThreads * q;
          if (prow != cc && (rl == cc || rl == prow)) {
#pragma unroll
            for (int i = 0; i < kLuSub; ++i) x[q][i] = rowbuf[rl == cc ? 1 : 0][i];
          }
          if (!zero && rl > cc && rl < rows) {
            const double l = x[q][c] / d;
            x[q][c] = l;
#pragma unroll
            for (int i = c + 1; i < kLuSub; ++i) x[q][i] = __builtin_fma(-l, rowbuf[1][i], x[q][i]);
          }
        }
      }
    };
    [&]<int... Cs>(std::integer_sequence<int, Cs...>) { (column(std::integral_constant<int, Cs>{}), ...); }(std::make_integer_sequence<int, kLuSub>{});
    // the sub-strip is final: store it, keep its diagonal block for the solve
#pragma unroll
    for (int q = 0; q < RPT; ++q) {
      const int rl = tid + kLuThreads * q;
      if (rl >= c0 && rl < rows) {
#pragma unroll
        for (int i = 0; i < kLuSub; ++i)
          if (i < cw) *at(rl, c0 + i) = x[q][i];
        if (rl < c0 + kLuSub) {
#pragma unroll
          for (int i = 0; i < kLuSub; ++i) Ls[rl - c0][i] = x[q][i];
        }
      }
    }
    __syncthreads();
    if (tid < cw) {
      const int r = pivl[c0 + tid];
      a.piv[c0 + tid] = (double)(r < w ? a.piv_top + r + 1 : a.piv_bot + (r - w) + 1);
    }
    // the other columns of the strip, a column per thread: the interchanges in
    // sequence, then (right of the sub-strip) the solve of rows c0 .. c0+cw-1
    if (tid < w && (tid < c0 || tid >= c0 + cw)) {
#pragma unroll 1
      for (int p = 0; p < cw; ++p) {
        const int r1 = c0 + p, r2 = pivl[r1];
        if (r2 != r1) {
          double* p1 = at(r1, tid);
          double* p2 = at(r2, tid);
          const double t = *p1;
          *p1 = *p2;
          *p2 = t;
        }
      }
      if (tid >= c0 + cw) {
        // rows c0 .. c0+cw-1 of this column lie above the diagonal: contiguous in T
        double* colp = a.Tp + (size_t)tid * a.ldt + c0;
        double u[kLuSub];
#pragma unroll
        for (int p = 0; p < kLuSub; ++p) u[p] = p < cw ? colp[p] : 0.0;
        // forward substitution, a column of Ls per (rolled) step: u stays in
        // registers under static indices, the final u[q] comes out by selects
#pragma unroll 1
        for (int q = 0; q < kLuSub - 1; ++q) {
          double uq = 0.0;
#pragma unroll
          for (int p = 0; p < kLuSub - 1; ++p) uq = p == q ? u[p] : uq;
#pragma unroll
          for (int p = 1; p < kLuSub; ++p) u[p] = __builtin_fma(p > q ? -Ls[p][q] : 0.0, uq, u[p]);
        }
#pragma unroll
        for (int p = 0; p < kLuSub; ++p) {
          if (p < cw) colp[p] = u[p];
          U12[p][tid - (c0 + cw)] = u[p];
        }
      }
    }
    __syncthreads();
    // the rows below the sub-strip: rank-16 update of the strip's later columns
    const int nrest = w - c0 - cw;
    if (nrest > 0) {
#pragma unroll
      for (int q = 0; q < RPT; ++q) {
        const int rl = tid + kLuThreads * q;
        if (rl >= c0 + cw && rl < rows) {
          for (int t = 0; t < nrest; ++t) {
            double* ptr = at(rl, c0 + cw + t);
            double v = *ptr;
#pragma unroll
            for (int p = 0; p < kLuSub; ++p) v = __builtin_fma(-x[q][p], U12[p][t], v);
            *ptr = v;
          }
        }
      }
    }
    __syncthreads();
  }
}

constexpr int kMaxLaswpBatch = 48;
struct LaswpArgs {
  int count;
  int prio;
  int block_start[kMaxLaswpBatch + 1];
  LaswpDesc d[kMaxLaswpBatch];
};
static_assert(sizeof(LaswpArgs) <= 4096, "LaswpArgs exceeds the kernel argument limit");

// a column per thread, 64 columns per workgroup; the interchanges of a column
// are applied in sequence (a pivot vector is no index map: rows repeat)
__global__ __launch_bounds__(64) void dlaswp_pair_kernel(const LaswpArgs a) {
  if (a.prio) __builtin_amdgcn_s_setprio(2);
  int di = 0;
  while (di + 1 < a.count && a.block_start[di + 1] <= (int)blockIdx.x) ++di;
  const LaswpDesc& d = a.d[di];
  const int col = ((int)blockIdx.x - a.block_start[di]) * 64 + (int)threadIdx.x;
  if (col >= d.ncols) return;
  double* tc = d.top + (size_t)col * d.ldt;
  double* bc = d.bot ? d.bot + (size_t)col * d.ldb : nullptr;
  const int total = d.mt + (d.bot ? max(d.h, 0) : 0);
  const int k1 = min(d.k1, d.mt);
  for (int p = max(d.k0, 0); p < k1; ++p) {
    const double v = d.piv[p];
    if (!(v >= 1.0 && v <= (double)total)) continue;  // not a row of the pair (nan included): no interchange
    const int r = (int)v - 1;
    if (r == p) continue;
    double* o = r < d.mt ? tc + r : bc + (r - d.mt);
    const double t = tc[p];
    tc[p] = *o;
    *o = t;
  }
}

void launch_laswp_batch(const LaswpDesc* descs, int n, hipStream_t stream, int prio) {
  for (int s0 = 0; s0 < n; s0 += kMaxLaswpBatch) {
    const int cnt = std::min(kMaxLaswpBatch, n - s0);
    LaswpArgs a;
    a.count = cnt;
    a.prio = prio;
    int total = 0;
    for (int i = 0; i < cnt; ++i) {
      a.d[i] = descs[s0 + i];
      a.block_start[i] = total;
      const LaswpDesc& d = a.d[i];
      if (d.ncols <= 0 || d.mt <= 0 || d.k1 <= d.k0) continue;
      if (d.ldt < d.mt || (d.bot && d.ldb < d.h)) fatal("dlaswp pair kernel: leading dimension below the row count (ldt=%d mt=%d ldb=%d h=%d)", d.ldt, d.mt, d.ldb, d.h);
      total += (d.ncols + 63) / 64;
    }
    a.block_start[cnt] = total;
    if (total == 0) continue;
    hipLaunchKernelGGL(dlaswp_pair_kernel, dim3(total), dim3(64), 0, stream, a);
  }
}

// L (strict lower triangle, n x n) := that of A
__global__ __launch_bounds__(256) void lu_copy_strict_lower_kernel(const double* __restrict__ A, int lda, double* __restrict__ L, int ldl, int n) {
  const int c = blockIdx.x;
  for (int r = c + 1 + (int)threadIdx.x; r < n; r += 256) L[(size_t)c * ldl + r] = A[(size_t)c * lda + r];
}

size_t lu_panel_workspace_bytes() { return 4096 * sizeof(double); }  // the inverse of one 64 x 64 unit lower block

void launch_lu_panel(const LuPanelDesc& g, hipStream_t stream, double* ws, int prio) {
  const int n = g.n;
  if (n <= 0) return;
  const bool ts = g.B != nullptr;
  if (n > kLuMaxTile || (ts && g.h > kLuMaxTile)) fatal("pivoted LU tile kernel: n=%d h=%d exceeds the tile limit %d", n, g.h, kLuMaxTile);
  if (g.ldt < n || g.ldl < n || (ts && (g.h <= 0 || g.ldb < g.h)) || g.pivcol < 0) fatal("pivoted LU tile kernel: bad shape (n=%d ldt=%d ldl=%d h=%d ldb=%d)", n, g.ldt, g.ldl, g.h, g.ldb);
  double* piv = g.L + (size_t)g.pivcol * g.ldl;
  for (int j = 0; j < n; j += 64) {
    const int w = std::min(64, n - j);
    const int rest = n - j - w;
    LuStripArgs a;
    a.Tp = g.T + (size_t)j * g.ldt + j;
    a.Lp = ts ? g.L + (size_t)j * g.ldl + j : a.Tp;
    a.Bp = ts ? g.B + (size_t)j * g.ldb : a.Tp + w;
    a.piv = piv + j;
    a.info = g.info;
    a.ldt = g.ldt;
    a.ldl = ts ? g.ldl : g.ldt;
    a.ldb = ts ? g.ldb : g.ldt;
    a.w = w;
    a.hb = ts ? g.h : rest;
    a.zero_rows = ts ? n - j : 0;
    a.piv_top = j;
    a.piv_bot = ts ? n : j + w;
    a.info_base = g.info_base + j;
    a.prio = prio;
    const int rows = a.w + a.hb;
    if (rows <= kLuThreads) hipLaunchKernelGGL(dlu_strip_kernel<1>, dim3(1), dim3(kLuThreads), 0, stream, a);
    else if (rows <= 2 * kLuThreads) hipLaunchKernelGGL(dlu_strip_kernel<2>, dim3(1), dim3(kLuThreads), 0, stream, a);
    else if (rows <= 3 * kLuThreads) hipLaunchKernelGGL(dlu_strip_kernel<3>, dim3(1), dim3(kLuThreads), 0, stream, a);
    else hipLaunchKernelGGL(dlu_strip_kernel<5>, dim3(1), dim3(kLuThreads), 0, stream, a);
    // the strip's interchanges on the columns left of it (L: L1 above L2) and right of it
    LaswpDesc sw[2];
    int ns = 0;
    if (j > 0) sw[ns++] = LaswpDesc{ts ? g.L : g.T, ts ? g.B : nullptr, piv, ts ? g.ldl : g.ldt, g.ldb, n, ts ? g.h : 0, j, j, j + w};
    if (rest > 0)
      sw[ns++] = LaswpDesc{g.T + (size_t)(j + w) * g.ldt, ts ? g.B + (size_t)(j + w) * g.ldb : nullptr, piv, g.ldt, g.ldb, n, ts ? g.h : 0, rest, j, j + w};
    launch_laswp_batch(sw, ns, stream, prio);
    if (rest <= 0) break;
    double* urow = g.T + (size_t)(j + w) * g.ldt + j;  // the block row right of the strip
    TrsmLeftDesc t{a.Lp, urow, w, rest, a.ldl, g.ldt, 1.0, 0, 0, 1, 0, nullptr};
    launch_trsm_left_batch(&t, 1, stream, ws);
    GemmDesc e{};
    e.A = a.Bp;
    e.B = urow;
    e.C = a.Bp + (size_t)w * a.ldb;
    e.m = a.hb; e.n = rest; e.k = w;
    e.lda = a.ldb; e.ldb = g.ldt; e.ldc = a.ldb;
    e.alpha = -1.0; e.beta = 1.0;
    launch_gemm_batch(&e, 1, stream);
  }
  if (!ts && n > 1) hipLaunchKernelGGL(lu_copy_strict_lower_kernel, dim3(n - 1), dim3(256), 0, stream, (const double*)g.T, g.ldt, g.L, g.ldl, n);
}

}  // namespace kern
}  // namespace parsec

// ------------------------------------------------- C entry points (tests)
namespace {
double* lu_test_ws() {
  static double* ws = [] {
    void* p = nullptr;
    (void)hipMalloc(&p, parsec::kern::lu_panel_workspace_bytes() + 64);
    return static_cast<double*>(p);
  }();
  return ws;
}
}  // namespace

extern "C" {
// Tile LU with partial pivoting: A (n x n) := L\U, the strict lower triangle of
// L := that of the factor, rows 0 .. n-1 of column n-1 of L := the pivots
int parsec_amd_dgetrf_piv_tile(double* A, int n, int lda, double* L, int ldl, int* info, void* stream) {
  parsec::LuPanelDesc g{A, lda, nullptr, 0, 0, n, L, ldl, n - 1, info, 0};
  parsec::kern::launch_lu_panel(g, (hipStream_t)stream, lu_test_ws());
  return (int)hipGetLastError();
}
// Pivoted LU of [U (n x n upper); A2 (h x n)]; L as above with pivots 1 .. n + h
int parsec_amd_dtstrf_tile(double* U, int ldu, double* A2, int lda2, int h, int n, double* L, int ldl, int* info, void* stream) {
  parsec::LuPanelDesc g{U, ldu, A2, lda2, h, n, L, ldl, n - 1, info, 0};
  parsec::kern::launch_lu_panel(g, (hipStream_t)stream, lu_test_ws());
  return (int)hipGetLastError();
}
// The interchanges piv[0 .. npiv-1] on [top (mt rows); bot (h rows, may be null)], ncols columns
int parsec_amd_dlaswp_pair(double* top, int ldt, int mt, double* bot, int ldb, int h, int ncols, const double* piv, int npiv, void* stream) {
  parsec::LaswpDesc d{top, bot, piv, ldt, ldb, mt, h, ncols, 0, npiv};
  parsec::kern::launch_laswp_batch(&d, 1, (hipStream_t)stream);
  return (int)hipGetLastError();
}
}
