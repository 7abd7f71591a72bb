// Dense tiled linear-algebra taskpools (the workloads named in BASELINE.json).
// The reference keeps these in DPLASMA (CHANGELOG.md:82-84); they are part of
// this framework so the benchmark runs end to end.
#pragma once
#include "../data/collections.hpp"
#include "../ptg/ptg.hpp"

#include <functional>

namespace parsec {
namespace algos {

// Tiled Cholesky A = L L^T (lower) on a (Sym)BlockCyclic collection, PTG form.
// `info_host` receives the LAPACK-style info after completion (0 = success).
ptg::PtgTaskpool* dpotrf_new(TiledMatrix* A, int uplo, int* info_host);
// The same factorization from the JDF source algos/jdf/dpotrf_L.jdf, compiled by
// parsec-ptgpp at build time (lower only, W = L^-1 panel solves).
ptg::PtgTaskpool* dpotrf_jdf_new(TiledMatrix* A, int* info_host);
int dpotrf_fuse_syrk(int set);  // SYRK(k-1,k) fused into POTRF(k) in new dpotrf_L.jdf taskpools; set < 0 queries
// Tiled triangular solve B := alpha op(A)^-1 B from the JDF source
// algos/jdf/dtrsm_left.jdf: side Left, uplo Lower, trans NoTrans or Trans, diag
// NonUnit (MatrixSide / MatrixUplo / MatrixTrans / MatrixDiag). A is N x N with
// square tiles, B is N x NRHS with B->mb == A->nb; A and B may be distributed
// differently. Any other request returns nullptr after a warning.
ptg::PtgTaskpool* dtrsm_new(int side, int uplo, int trans, int diag, double alpha, TiledMatrix* A, TiledMatrix* B);
// Solve A X = B with the Cholesky factor L that dpotrf left in A (lower only):
// the L sweep composed with the L^T sweep. B is overwritten with X. Freeing the
// returned taskpool (taskpool_free) frees the two sweeps.
Taskpool* dpotrs_new(int uplo, TiledMatrix* A, TiledMatrix* B);
// dpotrf_jdf_new composed with dpotrs_new. When the factorization fails
// (*info != 0 once it completed) the solve taskpools start empty: B is left
// untouched. One rank only (nullptr otherwise): ranks see only the pivots of
// their own diagonal tiles.
Taskpool* dposv_new(int uplo, TiledMatrix* A, TiledMatrix* B, int* info);
// Tiled inverse of a lower triangular matrix, A := L^-1 in place, from the JDF
// source algos/jdf/dtrtri_L.jdf: uplo Lower, diag NonUnit, A square (M == N)
// with square tiles, double; a ragged last tile is allowed. Only A's lower tiles
// and the lower triangles of its diagonal tiles are read and written.
// `info_host` (optional) receives the 1-based global index of the first diagonal
// entry that is exactly zero (0 = none). Anything else returns nullptr after a
// warning.
ptg::PtgTaskpool* dtrtri_new(int uplo, int diag, TiledMatrix* A, int* info_host);
// A := lower(L^T L) in place from the JDF source algos/jdf/dlauum_L.jdf, L the
// lower triangle of A; the same arguments and the same footprint as dtrtri_new.
ptg::PtgTaskpool* dlauum_new(int uplo, TiledMatrix* A);
// The inverse of an SPD matrix from the Cholesky factor L that dpotrf left in A
// (lower only): dtrtri_new composed with dlauum_new, A := L^-T L^-1. Only the
// lower triangle of the inverse is written (the caller symmetrises it if
// needed). Freeing the returned taskpool (taskpool_free) frees the two parts.
Taskpool* dpotri_new(int uplo, TiledMatrix* A);
// dpotrf_jdf_new composed with dpotri_new. When the factorization fails (*info
// != 0 once it completed) the inverse taskpools start empty: A holds what
// DPOTRF left. `info` is required. One rank only (nullptr otherwise): ranks see
// only the pivots of their own diagonal tiles.
Taskpool* dpoinv_new(int uplo, TiledMatrix* A, int* info);
// Tiled LU factorization WITHOUT pivoting, A = L U, from the JDF source
// algos/jdf/dgetrf_nopiv.jdf: A is square (M == N) with square tiles, double; a
// ragged last tile is allowed. On return A holds L (unit lower, its diagonal not
// stored) and U. The matrix must not need pivoting (diagonally dominant, or
// preconditioned): `info_host` receives the 1-based global index of the first
// pivot that is exactly zero (0 = none); a merely small pivot is not reported.
// Anything else returns nullptr after a warning.
ptg::PtgTaskpool* dgetrf_nopiv_new(TiledMatrix* A, int* info_host);
// Solve op(A) X = B with the factor dgetrf_nopiv_new left in A: trans NoTrans
// (the unit L sweep of dtrsm_left.jdf, then its U sweep) or Trans
// (U^T, then L^T). B is N x NRHS with B->mb == A->nb, any tile width, any
// distribution, and is overwritten with X. Freeing the returned taskpool
// (taskpool_free) frees the two sweeps.
Taskpool* dgetrs_nopiv_new(int trans, TiledMatrix* A, TiledMatrix* B);
// dgetrf_nopiv_new composed with dgetrs_nopiv_new (NoTrans). When the
// factorization meets a zero pivot (*info != 0 once it completed) the solve
// taskpools start empty: B is left untouched. `info` is required. One rank only
// (nullptr otherwise): ranks see only the pivots of their own diagonal tiles.
Taskpool* dgesv_nopiv_new(TiledMatrix* A, TiledMatrix* B, int* info);
// Tiled LU factorization with incremental (pairwise) pivoting from the JDF
// source algos/jdf/dgetrf_incpiv.jdf (PLASMA's / DPLASMA's dgetrf_incpiv): A is
// square with square tiles of at most 1024, double; a ragged last tile is
// allowed. L is the companion collection: same type, tile size (nb x nb), tile
// grid and distribution as A; its tiles (m, k), m >= k, receive a unit lower
// triangle in their strict lower part and the pivots (LAPACK ipiv values over
// the stacked rows of a tile pair, stored as doubles) in their last column.
// `info_host` receives the 1-based global index of the first diagonal entry of
// the final U that is exactly zero (0 = none); a zero pivot divides nothing, so
// the factor never holds inf / nan because of one. Anything else returns
// nullptr after a warning.
ptg::PtgTaskpool* dgetrf_incpiv_new(TiledMatrix* A, TiledMatrix* L, int* info_host);
// Solve A X = B with the factor dgetrf_incpiv_new left in A and L (NoTrans only):
// the recorded interchanges and eliminations applied to B in factorization
// order (dgetrs_incpiv.jdf), then the U sweep of dtrsm_left.jdf. B is N x NRHS
// with B->mb == A->nb, any tile width, any distribution, and is overwritten
// with X. Freeing the returned taskpool (taskpool_free) frees the parts.
Taskpool* dgetrs_incpiv_new(int trans, TiledMatrix* A, TiledMatrix* L, TiledMatrix* B);
// dgetrf_incpiv_new composed with dgetrs_incpiv_new. When U has a zero on its
// diagonal (*info != 0 once the factorization completed) the solve taskpools
// start empty: B is left untouched. `info` is required. One rank only (nullptr
// otherwise): ranks see only the zeros of their own tiles.
Taskpool* dgesv_incpiv_new(TiledMatrix* A, TiledMatrix* L, TiledMatrix* B, int* info);
// Tiled GEMM C = alpha op(A) op(B) + beta C (PTG; B transposed if transB).
ptg::PtgTaskpool* dgemm_new(double alpha, TiledMatrix* A, TiledMatrix* B, double beta, TiledMatrix* C, int transB);
// Tiled QR A = QR (Householder, tile algorithm GEQRT/TSQRT/UNMQR/TSMQR). T holds
// the block reflectors (ib x nb per tile).
ptg::PtgTaskpool* dgeqrf_new(TiledMatrix* A, TiledMatrix* T, int ib);
// The same factorization from the JDF source algos/jdf/dgeqrf.jdf, compiled by
// parsec-ptgpp at build time (the benchmark's taskpool).
ptg::PtgTaskpool* dgeqrf_jdf_new(TiledMatrix* A, TiledMatrix* T);
// B := op(Q) B with the Q that dgeqrf_jdf_new / dgeqrf_new (the flat-tree
// taskpools; NOT dgeqrf_hqr_new) left in A and T, from the JDF source
// algos/jdf/dormqr.jdf: side Left, trans Trans or NoTrans. A is M x N with square
// tiles, T is tiled like A, B is M x NRHS with B->mb == A->mb and any tile width;
// A / T and B may be distributed differently. Any other request returns nullptr
// after a warning.
ptg::PtgTaskpool* dormqr_new(int side, int trans, TiledMatrix* A, TiledMatrix* T, TiledMatrix* B);
// The minimiser of ||A X - B||_F (M >= N) from that factor: Q^T B composed with
// the solve with R (algos/jdf/dtrsm_left.jdf). On return rows 0..N-1 of B hold X
// and rows N..M-1 the residual components, whose column norms are the residual
// norms (LAPACK DGELS convention). A singular R yields inf / nan as in LAPACK.
// Freeing the returned taskpool (taskpool_free) frees its parts.
Taskpool* dgeqrs_new(TiledMatrix* A, TiledMatrix* T, TiledMatrix* B);
// dgeqrf_jdf_new composed with dgeqrs_new: A and T are overwritten with the factor.
Taskpool* dgels_new(TiledMatrix* A, TiledMatrix* T, TiledMatrix* B);
// Hierarchical QR (dgeqrf_hqr.cpp): TS domains of `domain` rows per process row
// (<= 0: all of them, i.e. flat inside a process row),
// TT binary trees over domain heads and across the p_rows process rows (<= 0:
// A's P). TT holds the TT-kernel reflectors (same shape as T).
ptg::PtgTaskpool* dgeqrf_hqr_new(TiledMatrix* A, TiledMatrix* T, TiledMatrix* TT, int domain, int p_rows);
// Collection operators (reference data_dist/matrix/apply.jdf, map_operator.c,
// reduce_col/row.jdf, broadcast.jdf, redistribute/*; see collection_ops.cpp).
using TileOp = std::function<void(TiledMatrix*, int64_t m, int64_t n, void* tile, void* arg)>;
using MapOp = std::function<void(const void* src, void* dst, int64_t m, int64_t n, int64_t rows, int64_t cols)>;
// inout = op(in, inout); `first` is true for the first tile of a chain (inout
// then holds the initial value of the result tile).
using ReduceOp = std::function<void(const void* in, void* inout, int64_t rows, int64_t cols, bool first)>;
ptg::PtgTaskpool* apply_new(TiledMatrix* A, int uplo, TileOp op, void* arg);
ptg::PtgTaskpool* map_operator_new(TiledMatrix* src, TiledMatrix* dst, MapOp op);
ptg::PtgTaskpool* reduce_col_new(TiledMatrix* A, TiledMatrix* res, ReduceOp op);
ptg::PtgTaskpool* reduce_row_new(TiledMatrix* A, TiledMatrix* res, ReduceOp op);
ptg::PtgTaskpool* broadcast_new(TiledMatrix* A, int64_t root_m, int64_t root_n, TiledMatrix* dst);
// Copy the size_row x size_col window at (disi_src, disj_src) of src to
// (disi_dst, disj_dst) of dst (any tile sizes / distributions). Blocking (DTD).
int redistribute(Context* ctx, TiledMatrix* src, TiledMatrix* dst, int64_t size_row, int64_t size_col, int64_t disi_src, int64_t disj_src, int64_t disi_dst,
                 int64_t disj_dst);
// The same copy as a PTG taskpool (algos/jdf/redistribute.jdf, or
// redistribute_reshuffle.jdf when tiles match and the window is tile aligned;
// reference redistribute_wrapper.c). nullptr on invalid arguments.
ptg::PtgTaskpool* redistribute_new(TiledMatrix* src, TiledMatrix* dst, int64_t size_row, int64_t size_col, int64_t disi_src, int64_t disj_src, int64_t disi_dst,
                                   int64_t disj_dst);
// Blocking form of redistribute_new (0 on success, -1 on invalid arguments).
int redistribute_ptg(Context* ctx, TiledMatrix* src, TiledMatrix* dst, int64_t size_row, int64_t size_col, int64_t disi_src, int64_t disj_src,
                     int64_t disi_dst, int64_t disj_dst);
// Diagonal + sub-diagonal tiles of a lower band matrix to LAPACK band storage in
// a 1 x (nt+1) row of (mb+1) x (nb+2) tiles (algos/jdf/diag_band_to_rect.jdf).
ptg::PtgTaskpool* diag_band_to_rect_new(TiledMatrix* A, TiledMatrix* B, int mt, int nt, int mb, int nb, size_t elem_size);
// Tiled C = alpha A B + beta C inserted as DTD tasks (blocking).
// Host DGEMM for CPU bodies (packed panels, AVX2/FMA micro-kernel; host_gemm.cpp)
void host_dgemm(int m, int n, int k, double alpha, const double* A, int lda, const double* B, int ldb, bool transB, double beta, double* C, int ldc);
int dtd_dgemm(Context* ctx, double alpha, TiledMatrix* A, TiledMatrix* B, double beta, TiledMatrix* C, bool use_gpu);

}  // namespace algos
}  // namespace parsec
