// CDNA4 (gfx950) kernels of the tile LU: without pivoting (dgetrf_nopiv.jdf,
// the second half of this file) and with incremental (pairwise) pivoting
// (dgetrf_incpiv.jdf / dgetrs_incpiv.jdf): the pivoted factorization of a tile
// (GETRF) or of an upper triangle stacked on a tile (TSTRF), and the grouped row
// interchanges of GESSM / SSSSM. The solves and updates of those tasks are the
// left-side tile solve of trsm_kernels.hip and the grouped DGEMM of tile_kernels.hip.
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

#include "device_helpers.hpp"
#include "kernels.hpp"
#include "launch_settings.hpp"

namespace parsec {
namespace kern {

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

void launch_laswp_batch(const LaswpDesc* descs, int n, hipStream_t stream) {
  for (int s0 = 0; s0 < n; s0 += kMaxLaswpBatch) {
    const int cnt = std::min(kMaxLaswpBatch, n - s0);
    LaswpArgs a;
    a.count = cnt;
    a.prio = launch_settings().prio;
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

void launch_lu_panel(const LuPanelDesc& g, hipStream_t stream, double* ws) {
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
    a.prio = launch_settings().prio;
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
    launch_laswp_batch(sw, ns, stream);
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
    hipLaunchKernelGGL(dgetrf_diag_kernel, dim3(1), dim3(256), 0, stream, g.A, g.lda, j, jb, bl, bu, g.info, g.info_base, launch_settings().prio);
    const int rest = g.n - j - jb;
    if (rest <= 0) break;
    const int nrb = (rest + 63) / 64;
    hipLaunchKernelGGL(dgetrf_panel_kernel, dim3(2 * nrb), dim3(256), 0, stream, g.A, g.lda, g.n, j, (const double*)bl, (const double*)bu, nrb, launch_settings().prio);
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

}  // namespace kern
}  // namespace parsec
