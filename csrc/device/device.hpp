// Device framework: registry, CPU / recursive devices, the HIP device engine
// entry points, and the GPU execution context handed to GPU chores.
//
// Parity: device registry with CPU=0, recursive=1, accelerators>=2 and relative
// capability weights (reference mca/device/device.c:194-285,617-666,843-904),
// parsec_get_best_device (device.c:79-189), GPU task staging / exec / pop
// pipeline with event rings (device_cuda_module.c:1961-2763).
// MI355X-first differences: one dedicated manager thread per GPU (no manager
// election), kernel *batching* (all ready tile tasks of one kernel kind are
// launched as ONE grouped kernel so small 512^2 tiles still fill 256 CUs),
// HIP stream priorities for critical-path tasks, and collections that can live
// in HBM permanently.
#pragma once
#include <hip/hip_runtime_api.h>

#include <vector>

#include "../core/runtime.hpp"
#include "../core/info.hpp"

namespace parsec {

// CPU capability from /proc/cpuinfo + cpufreq (reference device.c:678-797)
struct CpuCapability {
  std::string model;
  double ghz = 2.0;
  double dp_flops_per_cycle = 2.0;  // per core
  bool avx512 = false, avx2 = false, fma = false, sse2 = false, flags_seen = false;
  std::string isa() const;
};
CpuCapability cpu_capability();

void devices_init(Context* ctx);
void devices_start(Context* ctx);
void devices_stop(Context* ctx);
void devices_fini(Context* ctx);
bool device_type_enabled(Taskpool* tp, uint32_t type);
int gpu_chore_dispatch(ExecutionStream* es, Task* t, int chore);

// Raw device memory helpers (outside the engine's tile cache).
void* device_alloc(int device_index, size_t bytes);
void device_free(int device_index, void* p);
// Device-resident status words (LAPACK info of a factorization taskpool): a
// per-GPU pool allocated once, so building a taskpool costs no hipMalloc /
// hipMemset / hipFree (each of which synchronises the device). A slot is zero
// when acquired; release reads its final value (one 4-byte copy) and zeroes it.
int* device_status_acquire(int device_index);
int device_status_release(int device_index, int* slot);
// Thread-safe allocation from a GPU's tile-cache zone (no eviction, no memset):
// communication receive buffers. nullptr when the zone is full / no such GPU.
void* device_cache_alloc(int device_index, size_t bytes);
// Returns false when `p` does not belong to the zone (then use device_free).
bool device_cache_free(int device_index, void* p);
// Restrict the calling thread (and the threads it creates later) to the CPUs of
// the NUMA node closest to HIP device `ordinal` (intersected with the current
// affinity). Returns the node, or -1 when unknown / nothing to do.
int bind_thread_to_gpu_numa(int ordinal);
// dst <- src (bytes) as a copy kernel on `stream` (hipStream_t); 0 on success.
int device_copy_kernel(void* dst, const void* src, size_t bytes, void* stream);
// n device-to-device transfers in one launch (multi-source gather of IPC pulls)
int device_gather_kernel(void* const* dst, const void* const* src, const size_t* bytes, int n, void* stream);
int device_memcpy(int dst_dev, void* dst, int src_dev, const void* src, size_t bytes);
// bytes moved by device_memcpy since start / the last reset: H2D, D2H, D2D
void device_memcpy_stats(uint64_t out[3], bool reset);
// The process-wide copy stream of HIP device `ordinal` (created on first use).
hipStream_t gpu_copy_stream(int ordinal);
// A GPU copy chosen as the source of a transfer to `dst_device` (by
// data_start_transfer_ownership_to_copy), pinned with one reader under the data
// lock so its device cannot evict it before the transfer ran (re-chosen when it
// was evicted in between); *pinned says whether the returned copy is held.
// unpin_gpu_copy hands the reader back to the owning device's manager.
DataCopy* pin_gpu_source(Data* d, int dst_device, DataCopy* local, DataCopy* src, uint8_t access, bool* pinned);
void unpin_gpu_copy(DataCopy* c);
int device_hip_ordinal(int device_index);  // -1 if not a HIP device
int first_gpu_device_index();
// Bring the newest version of `d` to the host (device 0), synchronously.
DataCopy* data_pull_to_host(Data* d);
// Make sure every data_in of a CPU task is host-resident and current.
void cpu_stage_in(ExecutionStream* es, Task* t);
// After a CPU body wrote its flows: the host copies become the newest versions.
void cpu_write_epilog(Task* t);

// ------------------------------------------------------------------ batching
// Descriptors that a GPU chore enqueues into the manager's per-round batch
// (KernelBatch below). The launchers that take them: kernels/kernels.hpp.

struct GemmDesc {
  const double* A;
  const double* B;
  double* C;
  int m, n, k;
  int lda, ldb, ldc;
  double alpha, beta;
  uint8_t transA, transB;  // 0 = N, 1 = T
  uint8_t lower_only;      // 1: only C's lower triangle (SYRK)
  uint8_t a_lower;         // 1: op(A) is lower triangular (zeros above): row block i only reads k < (i+1) BM
  uint8_t b_upper;         // 1: op(B) is upper triangular (zeros below): column block j only reads k < (j+1) BN
  // 1: panel solve through W = L^-1 under PARSEC_DPOTRF_TRSM=auto: the
  // workgroups skip when the condition estimate (Cin[0] = max|L|, Cin[1] =
  // max|W|: a gated descriptor has beta 0 and never reads Cin as C) exceeds
  // the launch's limit
  uint8_t gate;
  // optional (zero = off): beta scales Cin (ld ldcin) instead of C, and C2 (ld
  // ldc2) -= every value written to C (fused "W = A1 + V^T A2" / "A1 -= T^T W")
  int ldcin, ldc2;
  const double* Cin;
  double* C2;
};

struct TrsmDesc {  // B := B * op(L)^-1 ; right side, lower, (trans), non-unit
  const double* L;
  double* B;
  int m, n;  // B is m x n, L is n x n
  int ldl, ldb;
  uint8_t trans;  // 1: B * L^-T (the Cholesky panel)
  uint8_t gate = 0;  // 1: run only when the estimate at gate_slot exceeds the limit (fallback of a gated W-GEMM)
  uint8_t packed = 0;  // 1: L is a packed panel tile: L(i, k) = L[i * ldl + k] for i > k (its strict upper part)
  uint8_t pad = 0;
  int invD_ld = 0;   // 0: invD holds contiguous 64x64 blocks; else the diagonal 64-blocks of an n x n matrix (ld invD_ld), e.g. W = L^-1
  const double* invD = nullptr;  // optional: inverses of L's 64x64 diagonal blocks (from POTRF)
  const double* gate_slot = nullptr;  // gate: max|L|, max|W| of the panel (workspace)
};
// B := alpha * op(L)^-1 B ; left side, L lower (default) or upper. L is n x n
// column-major and only the named triangle is read (the other one may hold
// anything: the V of a QR diagonal tile, the other factor of an LU tile), B is
// n x nrhs. With `right`, B is nrhs x n and X op(L) = alpha B is solved instead.
struct TrsmLeftDesc {
  const double* L;
  double* B;
  int n, nrhs;
  int ldl, ldb;
  double alpha;
  uint8_t trans;  // 0: L^-1 B (lower: forward sweep, upper: backward), 1: L^-T B (the other direction)
  uint8_t upper = 0;  // 1: L is upper triangular (the R of a QR factor)
  uint8_t unit = 0;   // 1: the diagonal of L is taken as 1 and never read (the L of an LU factor)
  // 1: right side, B := alpha B op(L)^-1 with B nrhs x n (n stays the order of
  // L, nrhs is the number of ROWS of B): op(L)^T X^T = alpha B^T, the same sweep
  // with the transpose flipped and the strip loaded and stored transposed
  uint8_t right = 0;
  // optional: inverses of L's 64x64 diagonal blocks (of the same triangle),
  // contiguous 4096-double blocks (dtrtri_diag_kernel / dtrtri_diag_upper_kernel)
  const double* invD = nullptr;
};
static_assert(sizeof(TrsmLeftDesc) == 56, "TrsmLeftDesc grew: the left-solve kernel argument block is sized for 64 of them");
static_assert(sizeof(GemmDesc) == 96, "GemmDesc grew: the grouped-GEMM kernel argument block is sized for 40 of them");

struct PotrfDesc {
  double* A;
  int n, lda;
  int* info;  // device pointer (may be null)
  double* invD_out = nullptr;  // optional: keep the 64x64 diagonal-block inverses (ceil(n/64) x 4096 doubles)
  double* W_out = nullptr;     // optional: also write W = L^-1 (n x n, lower triangular, zero above, ld ldw)
  int ldw = 0;
  // packed panel tile: W_out's strict upper triangle holds L^T instead of
  // zeros (W lower incl. the diagonal, L(i, j) = W_out(j, i) for i > j), so the
  // panel solve needs this ONE tile (TrsmGemmDesc::packed)
  uint8_t pack_w = 0;
};

// LU factorization without pivoting of an n x n tile (1 <= n <= 1152, lda >= n):
// A := L\U, L unit lower (its diagonal is not stored), U upper. Nothing outside
// the n x n part is read or written. *info (optional) receives info_base + the
// 1-based index of the first pivot that is exactly zero (the smallest index
// wins, the word is left alone otherwise); the factorization still finishes and
// then holds inf / nan. No pivoting: the matrix must not need it.
struct GetrfDesc {
  double* A;
  int n, lda;
  int* info;  // device pointer (may be null)
  // optional: the inverses of the 64 x 64 diagonal blocks of L (unit lower) and
  // of U, ceil(n/64) x 4096 doubles each, in the layout of dtrtri_diag_kernel /
  // dtrtri_diag_upper_kernel (identity-padded in a ragged last block)
  double* invL_out = nullptr;
  double* invU_out = nullptr;
  int info_base = 0;  // added to the index reported (the tile's first row in the matrix)
};

// LU with partial pivoting of one tile (GETRF: B == nullptr, T the n x n tile,
// A := L\U as DGETRF leaves it) or of a stacked pair (TSTRF: S = [T; B] with T
// n x n upper triangular and B h x n; P S = [L1; L2] U'). 1 <= n, h <= 1024.
// TSTRF: U' overwrites T's upper triangle (T's strict lower triangle is neither
// read nor written), L2 overwrites B, the strict lower triangle of L receives
// L1 (a full unit lower triangle: the interchanges are applied to the computed
// columns of L too). GETRF: the strict lower triangle of L receives a clean
// copy of the multipliers. Pivots: LAPACK ipiv values (1-based, sequential)
// over the stacked rows, 1 .. n a row of T and n+1 .. n+h a row of B, stored as
// doubles in rows 0 .. n-1 of column `pivcol` of L; nothing else of L is
// written. A column whose candidates are all exactly zero keeps its row as the
// pivot and divides nothing; *info (optional) then receives info_base + the
// 1-based column (the smallest index wins, the word is left alone otherwise).
struct LuPanelDesc {
  double* T;
  int ldt;
  double* B;
  int ldb, h;
  int n;
  double* L;
  int ldl, pivcol;
  int* info = nullptr;  // device pointer (may be null)
  int info_base = 0;
};

// Row interchanges of a stacked pair [top (mt rows); bot (h rows, may be null)]
// over ncols columns: for j = k0 .. k1-1 in sequence, row j of the top tile is
// exchanged with row piv[j] (1 .. mt a row of the top tile, mt+1 .. mt+h a row
// of the bottom tile). piv holds doubles (the pivot column of an L tile); an
// entry outside 1 .. mt+h means "no interchange" and is never used as an address.
struct LaswpDesc {
  double* top;
  double* bot;
  const double* piv;
  int ldt, ldb;
  int mt, h;
  int ncols;
  int k0, k1;
};
static_assert(sizeof(LaswpDesc) == 56, "LaswpDesc grew: the interchange kernel argument block is sized for 48 of them");

// Inverse of an n x n lower triangular tile, non-unit diagonal (1 <= n <= 1152,
// lda >= n): A := L^-1 in place, or W_out (ld ldw) := L^-1 with A left intact.
// Only the lower triangle is read and only the lower triangle of the target is
// written; rows n .. ld-1 are never touched. *info (optional) receives info_base
// + the 1-based index of the first diagonal entry that is exactly zero (the
// smallest index wins, the word is left alone otherwise); the kernel still
// finishes and the tile then holds inf / nan.
struct TrtriDesc {
  double* A;
  int n, lda;
  int* info = nullptr;  // device pointer (may be null)
  int info_base = 0;
  double* W_out = nullptr;
  int ldw = 0;
  // optional: the inverses of L's 64 x 64 diagonal blocks (dtrtri_diag_kernel's layout)
  const double* invD = nullptr;
};

// B := alpha L^T B in place; L is n x n lower (its strict upper triangle is
// never read), B is n x nrhs. With `lower`, B is itself n x n lower triangular:
// its strict upper triangle is neither read nor written (the LAUUM product).
struct TrmmDesc {
  const double* L;
  double* B;
  int n, nrhs;
  int ldl, ldb;
  double alpha;
  uint8_t lower = 0;
};
static_assert(sizeof(TrmmDesc) == 48, "TrmmDesc grew: the TRMM kernel argument block is sized for 64 of them");

// A := lower(L^T L) in place for an n x n lower triangular tile (lda >= n); the
// strict upper triangle and rows n .. lda-1 are never touched.
struct LauumDesc {
  double* A;
  int n, lda;
};

// Panel solve through the explicit inverse: B := B * W^T with W = L^-1 from
// POTRF (one grouped MFMA GEMM instead of a sequential blocked solve per tile).
struct TrsmGemmDesc {
  double* B;
  const double* W;
  int m, n;  // B is m x n, W is n x n lower triangular
  int ldb, ldw;
  // optional: the factor itself, for the substitution fallback of
  // PARSEC_DPOTRF_TRSM=auto / blocked (kernels/kernels.hpp trsm_inverse_mode)
  const double* L = nullptr;
  int ldl = 0;
  // 1: W is a packed panel tile (PotrfDesc::pack_w): W below and on the
  // diagonal, L^T above; L = W, ldl = ldw
  uint8_t packed = 0;
};

// Householder QR of a tile (GEQRT: A2 == nullptr) or of a triangle on top of a
// tile (TSQRT: [R = A1 (upper); A2]), compact WY with a full n x n upper T.
struct QrPanelDesc {
  double* A1;
  int lda1;
  double* A2;      // TSQRT only
  int lda2;
  double* T;       // n x n, written upper triangular with zeros below
  int ldt;
  double* Vcopy;   // GEQRT only (optional): clean unit-lower V (m1 x min(m1,n), ld m1)
  int m1;          // GEQRT: rows of the tile (min(m1, n) reflectors)
  int m2, n;       // TSQRT: rows of A2; columns
  // TTQRT: A2 is a zero-padded scratch copy of the upper trapezoid of `tri`
  // (m2 x n, ld ldtri), filled before the panel; V2's upper part goes back after
  double* tri;
  int ldtri;
};

// Apply Q^T (or Q: notrans) of a QR panel: UNMQR (A1 == nullptr: C = A2 := Q^T C
// with C and the unit-lower V both m2 rows, n reflectors) or TSMQR ([A1; A2] :=
// Q^T [A1; A2] with V = [I; V2], V2 m2 x n, A1 n x ncols).
struct QrApplyDesc {
  const double* V;
  int ldv;
  const double* T;
  int ldt;
  double* A1;
  int lda1;
  double* A2;
  int lda2;
  int m2, n, ncols;
  uint8_t notrans = 0;  // 1: apply Q = I - V T V^T instead of Q^T = I - V T^T V^T
};

// One block update of the DTD 3D 7-point stencil (stencil_kernels.hip).
struct StencilDesc {
  const double* u;
  double* out;
  const double* fin[6];  // -x +x -y +y -z +z neighbour planes (nullptr: boundary)
  double* fout[6];       // this block's boundary planes (nullptr: not needed)
  int bx, by, bz;
  double c0, c1;
};

// Initial condition of one stencil block (stencil_init_kernel).
struct StencilInitDesc {
  double* u;
  double* fout[6];
  int bx, by, bz;
  int64_t ox, oy, oz, nx, ny, nz;
};

struct KernelBatch {
  std::vector<GemmDesc> pre_gemm;  // launched before everything else (a POTRF's fused last update)
  std::vector<GemmDesc> gemm;
  std::vector<TrsmDesc> trsm;
  std::vector<TrsmLeftDesc> trsm_left;
  std::vector<PotrfDesc> potrf;
  std::vector<GetrfDesc> getrf;
  std::vector<LuPanelDesc> lu_panel;
  std::vector<LaswpDesc> laswp;  // launched before trsm_left (GESSM / SSSSM: interchange, solve, update)
  std::vector<TrtriDesc> trtri;
  std::vector<TrmmDesc> trmm;
  std::vector<LauumDesc> lauum;
  std::vector<TrsmGemmDesc> trsm_w;
  std::vector<StencilDesc> stencil;
  std::vector<QrPanelDesc> qr_panel;
  std::vector<QrApplyDesc> qr_apply;
  std::vector<std::function<void(hipStream_t)>> generic;  // other kernels, launched in order
  bool critical = false;  // launched on the critical stream: waves at raised issue priority
  bool one_per_cu = false;  // bulk 128x128 GEMMs padded to one workgroup per CU (room for critical kernels)
  // critical-path launch (only tasks at or above the critical threshold): its
  // workgroups claim their CUs, and bulk GEMM waves on a claimed CU pause
  // (kernels: g_crit_cu, bulk_yield) so the chain runs at idle speed
  int claim_cus = 0;  // 1: tile-POTRF steps claim, 2: every kernel of the launch
  bool bulk_yield = false;  // bulk launch: poll the claims
  // every queue, once: a new queue is listed here and nowhere else
  template <class Self, class F>
  static void each_queue(Self& b, F&& f) {
    f(b.pre_gemm); f(b.gemm); f(b.trsm); f(b.trsm_left); f(b.potrf); f(b.getrf); f(b.lu_panel); f(b.laswp);
    f(b.trtri); f(b.trmm); f(b.lauum); f(b.trsm_w); f(b.stencil); f(b.qr_panel); f(b.qr_apply); f(b.generic);
  }
  bool empty() const {
    bool none = true;
    each_queue(*this, [&](const auto& q) { none = none && q.empty(); });
    return none;
  }
  void clear() {
    each_queue(*this, [](auto& q) { q.clear(); });
  }
};

struct HipDevice;

// Handed to a GPU chore body: the stream to launch on and device pointers of
// the task's flows. Bodies may launch directly on `stream` or append to `batch`
// (preferred for tile kernels).
struct GpuExecContext {
  HipDevice* dev = nullptr;
  Device* device = nullptr;
  hipStream_t stream = nullptr;
  int stream_index = 0;
  Task* task = nullptr;
  KernelBatch* batch = nullptr;
  void* flow_ptr[kMaxFlows] = {};
  void* ptr(int flow) const { return flow_ptr[flow]; }
  void* workspace(size_t bytes);  // per-stream scratch (valid until the task completes)
  // per-stream info slot `id` of gpu_stream_infos(), built on first use on
  // this stream (e.g. a library handle bound to `stream`)
  void* info(int id);
};

using GpuHook = std::function<int(GpuExecContext*, Task*)>;

// Flush a batch on a stream (kernels/kernel_batch.cpp).
void launch_kernel_batch(KernelBatch& b, hipStream_t stream, void* workspace);
size_t kernel_batch_workspace_bytes(const KernelBatch& b);

}  // namespace parsec
