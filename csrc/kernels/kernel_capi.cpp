// C entry points of the tile, TRSM, LU and inverse kernels (tests, bench, the
// Python bindings; parsec_amd_dgemm and the two loop knobs are public:
// include/parsec.h, included here so that it is checked against kernels.hpp)
// and the test workspace they share. Host code only.
#include <hip/hip_runtime_api.h>

#include <mutex>

#include "kernels.hpp"
#include "launch_settings.hpp"
#include "parsec.h"

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
  parsec::kern::LaunchSettings s = parsec::kern::launch_settings();
  if (parsec::kern::gemm_policy().pad_test) s.pad = parsec::kern::kBulkPadBytes;
  const parsec::kern::LaunchScope scope(s);
  parsec::kern::launch_gemm_batch(descs, n, (hipStream_t)stream);
  return (int)hipGetLastError();
}
// Test hook, like PARSEC_GEMM_PAD_TEST above and not part of the public
// interface (include/parsec.h): the same launch as a bulk stream of an engine
// with cu_yield on issues it, i.e. the workgroups poll their CU's claim count
// once per k-tile (tests/test_gemm_pipeline_gpu.py)
int parsec_amd_dgemm_batch_yield(const parsec::GemmDesc* descs, int n, void* stream) {
  parsec::kern::LaunchSettings s = parsec::kern::launch_settings();
  s.yield = 1;
  const parsec::kern::LaunchScope scope(s);
  return parsec_amd_dgemm_batch(descs, n, stream);
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
int parsec_amd_potrf_stamps(long long* out) { return parsec::kern::potrf_stamps_read(out); }
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
// Tile LU with partial pivoting: A (n x n) := L\U, the strict lower triangle of
// L := that of the factor, rows 0 .. n-1 of column n-1 of L := the pivots
int parsec_amd_dgetrf_piv_tile(double* A, int n, int lda, double* L, int ldl, int* info, void* stream) {
  parsec::LuPanelDesc g{A, lda, nullptr, 0, 0, n, L, ldl, n - 1, info, 0};
  parsec::kern::launch_lu_panel(g, (hipStream_t)stream, static_cast<double*>(test_ws(parsec::kern::lu_panel_workspace_bytes() + 64)));
  return (int)hipGetLastError();
}
// Pivoted LU of [U (n x n upper); A2 (h x n)]; L as above with pivots 1 .. n + h
int parsec_amd_dtstrf_tile(double* U, int ldu, double* A2, int lda2, int h, int n, double* L, int ldl, int* info, void* stream) {
  parsec::LuPanelDesc g{U, ldu, A2, lda2, h, n, L, ldl, n - 1, info, 0};
  parsec::kern::launch_lu_panel(g, (hipStream_t)stream, static_cast<double*>(test_ws(parsec::kern::lu_panel_workspace_bytes() + 64)));
  return (int)hipGetLastError();
}
// The interchanges piv[0 .. npiv-1] on [top (mt rows); bot (h rows, may be null)], ncols columns
int parsec_amd_dlaswp_pair(double* top, int ldt, int mt, double* bot, int ldb, int h, int ncols, const double* piv, int npiv, void* stream) {
  parsec::LaswpDesc d{top, bot, piv, ldt, ldb, mt, h, ncols, 0, npiv};
  parsec::kern::launch_laswp_batch(&d, 1, (hipStream_t)stream);
  return (int)hipGetLastError();
}
}
