// Device helpers shared by the kernel files (csrc/kernels/*.hip): the vector
// types, the descriptor lookup of the grouped kernels, the XCD remap, the CU
// key of the claim table, one MFMA tile product and the 64 x 64 diagonal-block
// factor / inverse. All __device__ __forceinline__: the build has no
// relocatable device code, so every kernel inlines its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace parsec {
namespace kern {

typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double double2_t __attribute__((ext_vector_type(2)));

// raised issue priority for the waves of a critical launch (LaunchSettings::prio)
#define PARSEC_WAVE_PRIO(p) do { if (p) __builtin_amdgcn_s_setprio(2); } while (0)

// index of this wave's CU in the per-CU claim table: XCC id x (CU, SH, SE) bits of HW_ID
__device__ __forceinline__ int cu_key() {
  // HW_REG_HW_ID (4) bits [15:8] = CU_ID, SH_ID, SE_ID; HW_REG_XCC_ID (20) bits [3:0]
  const unsigned hw = __builtin_amdgcn_s_getreg((7 << 11) | (8 << 6) | 4);
  const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);
  return (int)(((xcc & 7u) << 8) | (hw & 0xffu));
}

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

constexpr int kDiagThreads = 256;  // workgroup of the diagonal-block kernels (block_potrf64)
constexpr int kTrsmThreads = 512;  // workgroup of the TRSM / TRMM strip kernels

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

}  // namespace kern
}  // namespace parsec
