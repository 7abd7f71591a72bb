// Host interface of the kernel layer (csrc/kernels): every launcher,
// workspace-size function and knob that is used outside the file defining it,
// and the C entry points of the kernel files, declared ONCE. Every file that
// defines or calls one of them includes this header, so a changed parameter
// list is a compile error and not a silent mismatch at link time.
// The descriptor structs and KernelBatch live in device/device.hpp; the
// per-thread launch settings in launch_settings.hpp.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../device/device.hpp"

namespace parsec {

// Panel solve of the tile Cholesky: 0 = always through W = L^-1, 1 = auto (W
// unless max|L| * max|W| > limit, then blocked substitution), 2 = always
// blocked substitution. Returns the previous mode; limit <= 0 keeps it.
int trsm_inverse_mode(int mode, double limit);
double trsm_inverse_limit();

namespace kern {

// ------------------------------------------------------------- grouped DGEMM
constexpr int kMaxGemmBatch = 40;    // descriptors of one launch (the kernel-argument limit)
constexpr int kBulkPadBytes = 8192;  // extra dynamic LDS of a padded bulk 128x128 launch (LaunchSettings::pad)
void launch_gemm_batch(const GemmDesc* descs, int n, hipStream_t stream);
// What the host decides for one grouped-DGEMM launch: the tile shape, the
// operand mode, the tile / workgroup counts and the kernel. The launch is
// issued from this record, and the launch log keeps it.
struct GemmLaunchRecord {
  int bm, bn;
  int descs;        // descriptors of the launch
  int total_tiles;  // tiles of all descriptors
  int main_tiles;   // tiles run whole; the other total_tiles - main_tiles are split ksplit ways along K
  int ksplit;
  int grid;         // workgroups
  int pad_bytes;    // extra dynamic LDS (one bulk workgroup per CU)
  uint8_t transA, transB;
  uint8_t full;     // unchecked loads
  uint8_t epilogue; // 0 plain (C preload when |alpha| = 1), 1 atomic
  uint8_t rotated;  // rotated k loop (gemm_mainloop)
  uint8_t pipelined; // rotated loop with the pinned body (gemm_pipeline)
};
// The launches launch_gemm_batch would issue for these descriptors on `slots`
// resident 128 x 128 workgroups under the current policy settings, in order,
// to out (room for n); returns their number. one_per_cu: a padded bulk launch
// (half the slots), bulk_yield / claim: as a yielding bulk stream or a
// claiming critical stream (claim >= 2) launches. Host code only: no device is
// touched and no descriptor pointer is dereferenced.
int gemm_launch_plan(const GemmDesc* descs, int n, int slots, bool one_per_cu, bool bulk_yield, int claim, GemmLaunchRecord* out);
constexpr int kGemmLaunchLogSize = 64;
// Per-thread record of the last kGemmLaunchLogSize grouped-DGEMM launches,
// written only while switched on: on 1 / 0, < 0 queries; returns the previous setting.
int gemm_launch_log(int on);
// Copies the calling thread's records, oldest first, to out (room for
// kGemmLaunchLogSize) and returns their number; reset empties the record.
int gemm_launch_log_read(GemmLaunchRecord* out, bool reset);
// Round-filling launch chunks on (1) / off (0: fixed launches of 40 descriptors), < 0 queries; returns the previous setting.
int gemm_chunk_fill(int on);
// The launch chunks launch_gemm_batch cuts for count descriptors of one operand
// mode with C of m[i] x n[i], on `slots` resident 128 x 128 workgroups: their
// lengths go to out (room for count), their number is returned. Host code only.
int gemm_chunk_plan(const int* m, const int* n, int count, int slots, int* out);
// Tile-size policy (0 = auto, 64, 128) / split-K tail of the 128x128 kernel
// (1 / 0) / k loop of the full register-staged launches (0 plain, 1 rotated);
// < 0 queries; each returns the previous setting.
int gemm_tile_policy(int p);
int gemm_splitk(int on);
int gemm_mainloop(int mode);
// Body of the rotated k loop, consulted only when gemm_mainloop is 1: 0 = the
// compiler's order inside a k-tile, 1 = the pinned order (fragment reads a
// kk-group of MFMAs ahead of their use), < 0 queries; returns the previous setting.
int gemm_pipeline(int mode);
// Whether a bm x bn x bk tile launch may take the pinned body for a descriptor
// with these transposes and leading dimensions: its per-thread operand offsets
// are 32-bit byte offsets, which span bk columns of A (bm of a transposed A)
// and bn columns of B (bk of a transposed B); 0 keeps the compiler-scheduled
// body. Host code only.
int gemm_pipeline_fits(int bm, int bn, int bk, int transA, int transB, long long lda, long long ldb);

// Between gemm_plan.cpp (decide) and the launcher beside the kernel (issue).
// Every knob of the grouped-GEMM dispatch: read from the environment once (no
// device needed), changed afterwards by the setters above.
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
GemmPolicy& gemm_policy();
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
std::vector<GemmLaunch> gemm_plan(const GemmDesc* descs, int n, const GemmPlanEnv& env, std::vector<GemmDesc>& sorted);
void gemm_launch_log_append(const GemmLaunchRecord& r);  // no-op while the log is off

// device_hip_cu_yield as the kernels see it (QR sub-panel kernels claim their CUs when > 0)
void set_cu_yield_mode(int m);
int cu_yield_mode();
// device address of the per-CU claim table (for kernels of other translation units)
int* crit_cu_table();

// -------------------------------------------- triangular solves (trsm_kernels.hip)
constexpr int kTrsmMaxCols = 18 * 64;  // LDS bound: (18*64*16 + 1024) doubles < 160 KiB
// invD[i] must already hold the inverted diagonal blocks of descs[i].L.
// in_place: the small-LDS variant (every n a multiple of 64; see dtrsm_inv_kernel)
void launch_trsm_inv(const TrsmDesc* descs, const double* const* invD, int n, hipStream_t stream, bool in_place = false);
void launch_trsm_batch(const TrsmDesc* descs, int n, hipStream_t stream, double* ws);
size_t trsm_workspace_bytes(const TrsmDesc* descs, int n);
void launch_trsm_left_batch(const TrsmLeftDesc* descs, int n, hipStream_t stream, double* ws);
size_t trsm_left_workspace_bytes(const TrsmLeftDesc* descs, int n);

// ------- diagonal-block inverses, tile POTRF, W-GEMM panel solve (tile_kernels.hip)
// Inverses of the 64 x 64 diagonal blocks of L (n x n lower, ld ldl) into invD:
// block b at invD + b * 4096, column-major, padded with the identity
// (unit: L's diagonal is taken as 1 and never read)
void launch_trtri_diag(const double* L, int ldl, int n, double* invD, hipStream_t stream, bool unit = false);
// the same for U (n x n upper): the blocks of invD are upper triangular; U's
// strict lower triangle is never read
void launch_trtri_diag_upper(const double* U, int ldu, int n, double* invD, hipStream_t stream, bool unit = false);
void launch_potrf(const PotrfDesc& p, hipStream_t stream, double* ws);
size_t potrf_workspace_bytes(const PotrfDesc& p);
void launch_potrf_steps(const PotrfDesc& p, hipStream_t stream, double* ws);
size_t potrf_steps_workspace_bytes(const PotrfDesc& p);
bool potrf_steps_eligible(const PotrfDesc& p);
int potrf_steps_mode(int on);
// phase clocks of the last stamped diagonal factorization (PARSEC_POTRF_STAMPS=1); a hipError_t
int potrf_stamps_read(long long* out);
void launch_trsm_w_batch(const TrsmGemmDesc* d, int n, hipStream_t stream, double* ws);
size_t trsm_w_workspace_bytes(const TrsmGemmDesc* d, int n);
// X = L^-1 (n x n lower, ld ldx, zero above the diagonal) from the inverses of
// L's 64x64 diagonal blocks by recursive doubling; tmp: n^2 / 2 + 4096 doubles
void launch_lower_inverse(const double* L, int lda, int n, const double* invD, double* X, int ldx, double* tmp, hipStream_t stream);

// ------------------------------------------ panel estimates (trsm_estimate.cpp)
// auto panel solve: 1 = the TRSM launch decides from the estimate the local
// POTRF published to pinned host memory (default), 0 = always the device-side
// gate; < 0 queries. Returns the previous setting.
int trsm_estimate_route(int on);
// [0] estimates published by tile POTRFs, [1] panel decisions taken on the
// host, [2] panels left to the device-side gate
void trsm_estimate_stats(uint64_t out[3], bool reset);
void trsm_estimate_count(int which);
// a device buffer was (re)allocated: drop a panel estimate keyed by its address
void trsm_estimate_forget(const void* p);
// the published estimate of the POTRF that wrote W = p (> 0), or 0 when unknown
double trsm_estimate_lookup(const void* p);
std::vector<uintptr_t> trsm_estimate_known();
// a slot for the POTRF writing W (device / host halves), or false
bool trsm_estimate_acquire(const double* W, unsigned long long** dev, double** host);

// ------------------------------------------------------ tile LU (lu_kernels.hip)
// tile LU without pivoting; ws: getrf_workspace_bytes(g)
void launch_getrf_nopiv(const GetrfDesc& g, hipStream_t stream, double* ws);
size_t getrf_workspace_bytes(const GetrfDesc& g);
// tile / stacked-pair LU with partial pivoting; ws: lu_panel_workspace_bytes()
constexpr int kLuMaxTile = 1024;
void launch_lu_panel(const LuPanelDesc& g, hipStream_t stream, double* ws);
size_t lu_panel_workspace_bytes();
// the interchanges of a batch, one grouped launch per 48 descriptors
void launch_laswp_batch(const LaswpDesc* descs, int n, hipStream_t stream);

// ------------------------- tile TRTRI / grouped TRMM / tile LAUUM (inverse_kernels.hip)
// ws: *_workspace_bytes
void launch_trtri(const TrtriDesc& t, hipStream_t stream, double* ws);
size_t trtri_workspace_bytes(const TrtriDesc& t);
void launch_trmm_lt_batch(const TrmmDesc* descs, int n, hipStream_t stream);
void launch_lauum(const LauumDesc& l, hipStream_t stream, double* ws);
size_t lauum_workspace_bytes(const LauumDesc& l);

// ------------------------------------------------------- tile QR (qr_kernels.hip)
void launch_qr_panel(const QrPanelDesc* descs, int n, hipStream_t stream);
void launch_qr_panel_blocked(const QrPanelDesc* descs, int n, hipStream_t stream, double* ws);
size_t qr_panel_workspace_bytes(const QrPanelDesc* descs, int n);
void launch_qr_apply(const QrApplyDesc* descs, int n, hipStream_t stream, double* ws);
size_t qr_apply_workspace_bytes(const QrApplyDesc* descs, int n);
// Vout (rows x min(rows, cols), ld rows) := the unit-lower V stored below the
// diagonal of a factored QR diagonal tile A (ld lda): ones on the diagonal,
// zeros above (the layout of QrPanelDesc::Vcopy)
void launch_qr_extract_v(const double* A, int lda, int rows, int cols, double* Vout, hipStream_t stream);

// ------------------------------------------------- stencil (stencil_kernels.hip)
using StencilArgs = StencilDesc;
void launch_stencil7_batch(const StencilDesc* d, int n, hipStream_t stream);
void launch_stencil_init(const StencilInitDesc& d, hipStream_t stream);

}  // namespace kern
}  // namespace parsec

// ------------------------------------------ C entry points (tests, bench, bindings)
// parsec_amd_dgemm, parsec_amd_gemm_mainloop and parsec_amd_gemm_pipeline are
// the public ones (include/parsec.h); kernel_capi.cpp includes both headers.
extern "C" {
int parsec_amd_gemm_tile_policy(int p);
int parsec_amd_gemm_splitk(int on);
int parsec_amd_gemm_mainloop(int mode);
int parsec_amd_gemm_pipeline(int mode);
int parsec_amd_dgemm_batch(const parsec::GemmDesc* descs, int n, void* stream);
int parsec_amd_dgemm_batch_yield(const parsec::GemmDesc* descs, int n, void* stream);
int parsec_amd_dgemm(char transa, char transb, int m, int n, int k, double alpha, const double* A, int lda, const double* B, int ldb, double beta,
                     double* C, int ldc, void* stream);
int parsec_amd_dtrsm_batch(const parsec::TrsmDesc* descs, int n, void* stream);
int parsec_amd_dtrsm_left_batch(const parsec::TrsmLeftDesc* descs, int n, void* stream);
int parsec_amd_dpotrf_tile(double* A, int n, int lda, int* info, void* stream);
int parsec_amd_dpotrf_tile_w(double* A, int n, int lda, int* info, double* W, int ldw, void* stream, int pack);
int parsec_amd_potrf_stamps(long long* out);
int parsec_amd_potrf_steps(int on);
int parsec_amd_trsm_w_batch(const parsec::TrsmGemmDesc* d, int n, void* stream);
int parsec_amd_dgetrf_nopiv_tile(double* A, int n, int lda, int* info, double* invL, double* invU, void* stream);
int parsec_amd_dgetrf_piv_tile(double* A, int n, int lda, double* L, int ldl, int* info, void* stream);
int parsec_amd_dtstrf_tile(double* U, int ldu, double* A2, int lda2, int h, int n, double* L, int ldl, int* info, void* stream);
int parsec_amd_dlaswp_pair(double* top, int ldt, int mt, double* bot, int ldb, int h, int ncols, const double* piv, int npiv, void* stream);
int parsec_amd_dtrtri_tile(double* A, int n, int lda, int* info, int info_base, double* W, int ldw, void* stream);
int parsec_amd_dtrmm_lt_batch(const parsec::TrmmDesc* descs, int n, void* stream);
int parsec_amd_dlauum_tile(double* A, int n, int lda, void* stream);
int parsec_amd_qr_profile(unsigned long long* out);
int parsec_amd_qr_panel(const parsec::QrPanelDesc* d, int n, void* stream);
int parsec_amd_qr_panel_unblocked(const parsec::QrPanelDesc* d, int n, void* stream);
int parsec_amd_qr_apply(const parsec::QrApplyDesc* d, int n, void* ws, void* stream);
size_t parsec_amd_qr_apply_ws(const parsec::QrApplyDesc* d, int n);
int parsec_amd_qr_extract_v(const double* A, int lda, int rows, int cols, double* Vout, void* stream);
}
