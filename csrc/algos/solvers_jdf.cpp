// The solvers built on the left-side triangular sweep that parsec-ptgpp
// generates from algos/jdf/dtrsm_left.jdf (build/gen/dtrsm_left.{h,cpp}), with
// the factorization and the Q^T B they are composed with (dgetrf_nopiv.jdf,
// dormqr.jdf): argument checks, arenas, and the compositions
//   DPOTRS       = solve with L, then with L^T        DPOSV       = DPOTRF, then DPOTRS
//   DGETRS_NOPIV = unit L, then U (or U^T, then L^T)  DGESV_NOPIV = DGETRF_NOPIV, then DGETRS_NOPIV
//   DGEQRS       = Q^T B, then solve with R           DGELS       = DGEQRF, then DGEQRS
//   DGETRS_INCPIV = the recorded L and P, then U      DGESV_INCPIV = DGETRF_INCPIV, then DGETRS_INCPIV
#include "dgetrf_incpiv.h"
#include "dgetrf_nopiv.h"
#include "dgetrs_incpiv.h"
#include "dormqr.h"
#include "dtrsm_left.h"
#include "jdf_glue.hpp"
#include "linalg.hpp"

namespace parsec {
namespace algos {

// One sweep B(0:N, :) := alpha op(T)^-1 B(0:N, :), T the lower or upper triangle
// of A's leading N x N part (internal: dtrsm_new keeps refusing the upper
// triangle and the unit diagonal). *gate (optional) is read when the sweep is
// enqueued: non-zero makes it start with no task at all.
static parsec_dtrsm_left_taskpool_t* sweep_new(bool upper, bool trans, bool unit, double alpha, TiledMatrix* A, TiledMatrix* B, const int* gate = nullptr) {
  parsec_dtrsm_left_taskpool_t* tp = parsec_dtrsm_left_new(A, B, upper, trans, alpha);
  tp->_g_UNIT = unit;
  tp->taskpool_name = std::string("dtrsm_left.jdf (L") + (upper ? "U" : "L") + (trans ? "T" : "N") + (unit ? ", unit)" : ")");
  inv_arena(tp->arenas_datatypes[PARSEC_dtrsm_left_INV_ADT_IDX], A->nb);
  gate_on(tp, gate, &tp->_g_MT);
  return tp;
}

ptg::PtgTaskpool* dtrsm_new(int side, int uplo, int trans, int diag, double alpha, TiledMatrix* A, TiledMatrix* B) {
  if (side != MATRIX_LEFT || uplo != MATRIX_LOWER || diag != MATRIX_NONUNIT ||
      (trans != MATRIX_NOTRANS && trans != MATRIX_TRANS && trans != MATRIX_CONJTRANS)) {
    warning("dtrsm_new: side %s / uplo %s / trans %d / diag %s is not implemented (Left, Lower, NoTrans or Trans, NonUnit only)",
            side == MATRIX_LEFT ? "Left" : side == MATRIX_RIGHT ? "Right" : "?", uplo == MATRIX_LOWER ? "Lower" : uplo == MATRIX_UPPER ? "Upper" : "?", trans,
            diag == MATRIX_NONUNIT ? "NonUnit" : diag == MATRIX_UNIT ? "Unit" : "?");
    return nullptr;
  }
  if (const char* why = solve_problem(A, B)) {
    warning("dtrsm_new: %s", why);
    return nullptr;
  }
  return sweep_new(false, trans != MATRIX_NOTRANS, false, alpha, A, B);
}

Taskpool* dpotrs_new(int uplo, TiledMatrix* A, TiledMatrix* B) {
  if (uplo != MATRIX_LOWER) {
    warning("dpotrs_new: only the lower factor is implemented");
    return nullptr;
  }
  if (const char* why = solve_problem(A, B)) {
    warning("dpotrs_new: %s", why);
    return nullptr;
  }
  return compose_owned("dpotrs", {sweep_new(false, false, false, 1.0, A, B), sweep_new(false, true, false, 1.0, A, B)});
}

Taskpool* dposv_new(int uplo, TiledMatrix* A, TiledMatrix* B, int* info) {
  if (uplo != MATRIX_LOWER) {
    warning("dposv_new: only the lower factor is implemented");
    return nullptr;
  }
  if (const char* why = solve_problem(A, B)) {
    warning("dposv_new: %s", why);
    return nullptr;
  }
  if (!info) {
    warning("dposv_new: info is required (the solve is skipped when the factorization fails)");
    return nullptr;
  }
  // The solve is gated on this process's info word. Ranks see only the pivots
  // of their own diagonal tiles, so on several ranks they could disagree about
  // running the solve.
  if (A->nodes > 1 || B->nodes > 1) {
    warning("dposv_new: not implemented on more than one rank (compose dpotrf and dpotrs after checking info)");
    return nullptr;
  }
  return compose_owned("dposv", {dpotrf_jdf_new(A, info), sweep_new(false, false, false, 1.0, A, B, info), sweep_new(false, true, false, 1.0, A, B, info)});
}

ptg::PtgTaskpool* dgetrf_nopiv_new(TiledMatrix* A, int* info_host) {
  if (info_host) *info_host = 0;
  if (const char* why = factor_problem(A)) {
    warning("dgetrf_nopiv_new: %s", why);
    return nullptr;
  }
  const InfoWords w = info_acquire();
  parsec_dgetrf_nopiv_taskpool_t* tp = parsec_dgetrf_nopiv_new(A, w.hip(), w.cpu);
  tp->taskpool_name = "dgetrf_nopiv.jdf";
  inv_arena(tp->arenas_datatypes[PARSEC_dgetrf_nopiv_INV_ADT_IDX], A->nb);  // of one tile of L or U
  info_attach(tp, w, info_host);
  return tp;
}

// The sweeps with the two triangles of the factor in A: L is unit lower (A's diagonal holds U's)
static Taskpool* lu_l_sweep(bool trans, TiledMatrix* A, TiledMatrix* B, const int* gate) { return sweep_new(false, trans, true, 1.0, A, B, gate); }
static Taskpool* lu_u_sweep(bool trans, TiledMatrix* A, TiledMatrix* B, const int* gate) { return sweep_new(true, trans, false, 1.0, A, B, gate); }

Taskpool* dgetrs_nopiv_new(int trans, TiledMatrix* A, TiledMatrix* B) {
  if (trans != MATRIX_NOTRANS && trans != MATRIX_TRANS) {
    warning("dgetrs_nopiv_new: trans %d is not implemented (NoTrans or Trans only)", trans);
    return nullptr;
  }
  if (const char* why = solve_problem(A, B)) {
    warning("dgetrs_nopiv_new: %s", why);
    return nullptr;
  }
  // A X = B: L then U; A^T X = B: U^T then L^T
  if (trans == MATRIX_TRANS) return compose_owned("dgetrs_nopiv", {lu_u_sweep(true, A, B, nullptr), lu_l_sweep(true, A, B, nullptr)});
  return compose_owned("dgetrs_nopiv", {lu_l_sweep(false, A, B, nullptr), lu_u_sweep(false, A, B, nullptr)});
}

Taskpool* dgesv_nopiv_new(TiledMatrix* A, TiledMatrix* B, int* info) {
  if (const char* why = solve_problem(A, B)) {
    warning("dgesv_nopiv_new: %s", why);
    return nullptr;
  }
  if (!info) {
    warning("dgesv_nopiv_new: info is required (the solve is skipped when the factorization meets a zero pivot)");
    return nullptr;
  }
  // The solve is gated on this process's info word. Ranks see only the pivots
  // of their own diagonal tiles, so on several ranks they could disagree about
  // running the solve.
  if (A->nodes > 1 || B->nodes > 1) {
    warning("dgesv_nopiv_new: not implemented on more than one rank (compose dgetrf_nopiv and dgetrs_nopiv after checking info)");
    return nullptr;
  }
  return compose_owned("dgesv_nopiv", {dgetrf_nopiv_new(A, info), lu_l_sweep(false, A, B, info), lu_u_sweep(false, A, B, info)});
}

ptg::PtgTaskpool* dgetrf_incpiv_new(TiledMatrix* A, TiledMatrix* L, int* info_host) {
  if (info_host) *info_host = 0;
  if (const char* why = incpiv_problem(A, L)) {
    warning("dgetrf_incpiv_new: %s", why);
    return nullptr;
  }
  const InfoWords w = info_acquire();
  parsec_dgetrf_incpiv_taskpool_t* tp = parsec_dgetrf_incpiv_new(A, L, w.hip(), w.cpu);
  tp->taskpool_name = "dgetrf_incpiv.jdf";
  info_attach(tp, w, info_host);
  return tp;
}

// the interchanges and eliminations of the factorization applied to B
static Taskpool* incpiv_forward(TiledMatrix* A, TiledMatrix* L, TiledMatrix* B, const int* gate) {
  parsec_dgetrs_incpiv_taskpool_t* tp = parsec_dgetrs_incpiv_new(A, L, B);
  tp->taskpool_name = "dgetrs_incpiv.jdf";
  gate_on(tp, gate, &tp->_g_MT);
  return tp;
}

// the checks DGETRS_INCPIV and DGESV_INCPIV share
static bool incpiv_solve_refused(const char* who, const TiledMatrix* A, const TiledMatrix* L, const TiledMatrix* B) {
  const char* why = incpiv_problem(A, L);
  if (!why) why = solve_problem(A, B);
  if (why) warning("%s: %s", who, why);
  return why != nullptr;
}

Taskpool* dgetrs_incpiv_new(int trans, TiledMatrix* A, TiledMatrix* L, TiledMatrix* B) {
  if (trans != MATRIX_NOTRANS) {
    warning("dgetrs_incpiv_new: trans %d is not implemented (NoTrans only: a transposed solve runs the chain backwards)", trans);
    return nullptr;
  }
  if (incpiv_solve_refused("dgetrs_incpiv_new", A, L, B)) return nullptr;
  return compose_owned("dgetrs_incpiv", {incpiv_forward(A, L, B, nullptr), lu_u_sweep(false, A, B, nullptr)});
}

Taskpool* dgesv_incpiv_new(TiledMatrix* A, TiledMatrix* L, TiledMatrix* B, int* info) {
  if (incpiv_solve_refused("dgesv_incpiv_new", A, L, B)) return nullptr;
  if (!info) {
    warning("dgesv_incpiv_new: info is required (the solve is skipped when U has a zero on its diagonal)");
    return nullptr;
  }
  // The solve is gated on this process's info word. Ranks see only the zeros
  // of their own tiles, so on several ranks they could disagree about running
  // the solve.
  if (A->nodes > 1 || B->nodes > 1) {
    warning("dgesv_incpiv_new: not implemented on more than one rank (compose dgetrf_incpiv and dgetrs_incpiv after checking info)");
    return nullptr;
  }
  return compose_owned("dgesv_incpiv", {dgetrf_incpiv_new(A, L, info), incpiv_forward(A, L, B, info), lu_u_sweep(false, A, B, info)});
}

static parsec_dormqr_taskpool_t* apply_q_new(bool trans, TiledMatrix* A, TiledMatrix* T, TiledMatrix* B) {
  parsec_dormqr_taskpool_t* tp = parsec_dormqr_new(A, T, B, trans);
  tp->taskpool_name = trans ? "dormqr.jdf (LT)" : "dormqr.jdf (LN)";
  // the clean V of one diagonal tile
  add2arena_rect(tp->arenas_datatypes[PARSEC_dormqr_TILE_ADT_IDX], sizeof(double), A->nb, A->nb, A->nb);
  return tp;
}

ptg::PtgTaskpool* dormqr_new(int side, int trans, TiledMatrix* A, TiledMatrix* T, TiledMatrix* B) {
  if (side != MATRIX_LEFT || (trans != MATRIX_NOTRANS && trans != MATRIX_TRANS)) {
    warning("dormqr_new: side %s / trans %d is not implemented (Left, NoTrans or Trans only)", side == MATRIX_LEFT ? "Left" : side == MATRIX_RIGHT ? "Right" : "?",
            trans);
    return nullptr;
  }
  if (const char* why = qr_solve_problem(A, T, B)) {
    warning("dormqr_new: %s", why);
    return nullptr;
  }
  return apply_q_new(trans == MATRIX_TRANS, A, T, B);
}

// the checks DGEQRS and DGELS share
static bool qr_solve_refused(const char* who, const TiledMatrix* A, const TiledMatrix* T, const TiledMatrix* B) {
  const char* why = qr_solve_problem(A, T, B);
  if (!why && A->m < A->n) why = "M < N (the minimum-norm solution) is not implemented";
  if (why) warning("%s: %s", who, why);
  return why != nullptr;
}

Taskpool* dgeqrs_new(TiledMatrix* A, TiledMatrix* T, TiledMatrix* B) {
  if (qr_solve_refused("dgeqrs_new", A, T, B)) return nullptr;
  return compose_owned("dgeqrs", {apply_q_new(true, A, T, B), sweep_new(true, false, false, 1.0, A, B)});
}

Taskpool* dgels_new(TiledMatrix* A, TiledMatrix* T, TiledMatrix* B) {
  if (qr_solve_refused("dgels_new", A, T, B)) return nullptr;
  return compose_owned("dgels", {dgeqrf_jdf_new(A, T), apply_q_new(true, A, T, B), sweep_new(true, false, false, 1.0, A, B)});
}

}  // namespace algos
}  // namespace parsec
