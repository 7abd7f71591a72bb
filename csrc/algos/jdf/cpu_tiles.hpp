// CPU reference tile routines and small helpers shared by the JDF prologues in
// this directory (dtrsm_left, dgetrf_nopiv, dgetrf_incpiv, dgetrs_incpiv, dtrtri_L,
// dlauum_L, dpotrf_L): plain
// loops on column-major tiles, used by CPU-only runs and tests. One routine per
// operation; the triangle, the transpose, the unit diagonal and the sign are
// arguments. Bodies that only one JDF needs stay in its prologue.
//
// The order of the floating-point operations is part of the contract: CPU
// results are compared bit for bit between builds, so a sum may not be
// re-associated here. Scaling by an alpha of 1.0 and leaving out the division
// by a unit diagonal are exact.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <utility>

/* inverses of the 64 x 64 diagonal blocks of a triangular tile T (n x n, lower or
 * upper; unit: the diagonal is taken as 1 and never read): block b -> D + b * 4096,
 * column-major, padded with the identity (the layout of dtrtri_diag_kernel /
 * dtrtri_diag_upper_kernel) */
static inline void jdf_cpu_diag_inverses(const double* T, int ld, int n, double* D, bool upper, bool unit) {
    for (int c0 = 0, b = 0; c0 < n; c0 += 64, ++b) {
        const int w = std::min(64, n - c0);
        double* X = D + (size_t)b * 4096;
        const double* A = T + c0 + (size_t)c0 * ld;
        for (int c = 0; c < 64; ++c)
            for (int r = 0; r < 64; ++r) X[r + 64 * c] = r == c ? 1.0 : 0.0;
        for (int c = 0; c < w; ++c) {
            X[c + 64 * c] = unit ? 1.0 : 1.0 / A[c + (size_t)c * ld];
            if (!upper) {
                for (int r = c + 1; r < w; ++r) {
                    double s = 0.0;
                    for (int p = c; p < r; ++p) s += A[r + (size_t)p * ld] * X[p + 64 * c];
                    X[r + 64 * c] = unit ? -s : -s / A[r + (size_t)r * ld];
                }
            } else {
                for (int r = c - 1; r >= 0; --r) {
                    double s = 0.0;
                    for (int p = r + 1; p <= c; ++p) s += A[r + (size_t)p * ld] * X[p + 64 * c];
                    X[r + 64 * c] = unit ? -s : -s / A[r + (size_t)r * ld];
                }
            }
        }
    }
}
/* B (n x nrhs) := alpha op(T)^-1 B by substitution, column by column; T lower or
 * upper, op(T) = T or T^T. op(T) is lower, and the rows go top to bottom, when
 * upper == trans. */
static inline void jdf_cpu_left_solve(const double* T, int ld, double* B, int ldb, int n, int nrhs, double alpha, bool upper, bool trans, bool unit) {
    for (int j = 0; j < nrhs; ++j) {
        double* x = B + (size_t)j * ldb;
        if (upper == trans) {
            for (int i = 0; i < n; ++i) {
                double s = alpha * x[i];
                for (int p = 0; p < i; ++p) s -= (trans ? T[p + (size_t)i * ld] : T[i + (size_t)p * ld]) * x[p];
                x[i] = unit ? s : s / T[i + (size_t)i * ld];
            }
        } else {
            for (int i = n - 1; i >= 0; --i) {
                double s = alpha * x[i];
                for (int p = i + 1; p < n; ++p) s -= (trans ? T[p + (size_t)i * ld] : T[i + (size_t)p * ld]) * x[p];
                x[i] = unit ? s : s / T[i + (size_t)i * ld];
            }
        }
    }
}
/* Row interchanges of a stacked pair [top (mt rows); bot (h rows, may be null)]
 * over ncols columns: for j = k0 .. k1-1 in sequence, row j of the top tile is
 * exchanged with row piv[j] (LAPACK ipiv values stored as doubles: 1 .. mt a row
 * of the top tile, mt+1 .. mt+h a row of the bottom tile). An entry outside
 * 1 .. mt+h means "no interchange" and is never used as an address. */
static inline void jdf_cpu_laswp_pair(double* top, int ldt, int mt, double* bot, int ldb, int h, int ncols, const double* piv, int k0, int k1) {
    const int total = mt + (bot && h > 0 ? h : 0);
    for (int j = std::max(k0, 0); j < k1 && j < mt; ++j) {
        const double v = piv[j];
        if (!(v >= 1.0 && v <= (double)total)) continue;
        const int r = (int)v - 1;
        if (r == j) continue;
        double* o = r < mt ? top + r : bot + (r - mt);
        const size_t ldo = r < mt ? ldt : ldb;
        for (int c = 0; c < ncols; ++c) std::swap(top[j + (size_t)c * ldt], o[c * ldo]);
    }
}
/* LU with partial pivoting of the stacked S = [T; B], T n x n and B h x n, the
 * storage format of the GPU kernels (LuPanelDesc).
 *   ts == false (GETRF, h == 0): T := L\U as DGETF2 leaves it.
 *   ts == true  (TSTRF): T is upper triangular and its strict lower triangle is
 *     neither read nor written; U' overwrites its upper triangle, L2 overwrites
 *     B, and L1 -- a full unit lower triangle, because the interchanges are
 *     applied to the computed columns of L too -- goes to the strict lower
 *     triangle of L, which is cleared first. The rows of T below the diagonal are
 *     zero in S and an interchange only moves a row of B onto the diagonal row,
 *     so the candidates of column j are row j of T and the rows of B.
 * piv[j] is the 1-based stacked row exchanged with row j (1 .. n in T, n+1 .. n+h
 * in B). When every candidate of a column is exactly zero the row keeps its
 * place and nothing is divided. Returns the 1-based index of the first such
 * column (a zero on U's diagonal), or 0. */
static inline int jdf_cpu_lu_pair(bool ts, double* T, int ldt, double* B, int ldb, int h, int n, double* L, int ldl, double* piv) {
    double* Lo = ts ? L : T;  /* where row j keeps its computed multipliers (columns < j) */
    const int ldo = ts ? ldl : ldt;
    if (ts)
        for (int c = 0; c < n; ++c)
            for (int r = c + 1; r < n; ++r) L[r + (size_t)c * ldl] = 0.0;
    int info = 0;
    for (int j = 0; j < n; ++j) {
        double best = std::fabs(T[j + (size_t)j * ldt]);
        int p = j;
        if (!ts)
            for (int r = j + 1; r < n; ++r) {
                const double v = std::fabs(T[r + (size_t)j * ldt]);
                if (v > best) { best = v; p = r; }
            }
        for (int r = 0; r < h; ++r) {
            const double v = std::fabs(B[r + (size_t)j * ldb]);
            if (v > best) { best = v; p = n + r; }
        }
        if (best == 0.0) {
            piv[j] = (double)(j + 1);
            if (!info) info = j + 1;
            continue;
        }
        piv[j] = (double)(p + 1);
        if (p != j) {
            double* o = p < n ? T + p : B + (p - n);
            const size_t ldp = p < n ? ldt : ldb;
            for (int c = 0; c < j; ++c) std::swap(Lo[j + (size_t)c * ldo], o[c * ldp]);
            for (int c = j; c < n; ++c) std::swap(T[j + (size_t)c * ldt], o[c * ldp]);
        }
        const double d = T[j + (size_t)j * ldt];
        if (!ts)
            for (int r = j + 1; r < n; ++r) T[r + (size_t)j * ldt] /= d;
        for (int r = 0; r < h; ++r) B[r + (size_t)j * ldb] /= d;
        for (int c = j + 1; c < n; ++c) {
            const double u = T[j + (size_t)c * ldt];
            if (!ts)
                for (int r = j + 1; r < n; ++r) T[r + (size_t)c * ldt] -= T[r + (size_t)j * ldt] * u;
            for (int r = 0; r < h; ++r) B[r + (size_t)c * ldb] -= B[r + (size_t)j * ldb] * u;
        }
    }
    return info;
}
/* GETRF of the tile LU with incremental pivoting: A (n x n) := L\U with partial
 * pivoting; the strict lower triangle of L receives a clean copy of the
 * multipliers and rows 0 .. n-1 of its column pivcol the pivots */
static inline int jdf_cpu_getrf_piv(double* A, int n, int lda, double* L, int ldl, int pivcol) {
    const int info = jdf_cpu_lu_pair(false, A, lda, nullptr, 0, 0, n, nullptr, 0, L + (size_t)pivcol * ldl);
    for (int c = 0; c < n; ++c)
        for (int r = c + 1; r < n; ++r) L[r + (size_t)c * ldl] = A[r + (size_t)c * lda];
    return info;
}
/* TSTRF: pivoted LU of [U (n x n upper); A2 (h x n)], L1 and the pivots into L */
static inline int jdf_cpu_tstrf(double* U, int ldu, double* A2, int lda2, int h, int n, double* L, int ldl, int pivcol) {
    return jdf_cpu_lu_pair(true, U, ldu, A2, lda2, h, n, L, ldl, L + (size_t)pivcol * ldl);
}
/* C (m x n) := beta C - op(A) X, op(A) m x k (A stored k x m when trans) */
static inline void jdf_cpu_update(const double* A, int lda, const double* X, int ldx, double* C, int ldc, int m, int n, int k, double beta, bool trans) {
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < m; ++i) {
            double s = 0.0;
            for (int p = 0; p < k; ++p) s += (trans ? A[p + (size_t)i * lda] : A[i + (size_t)p * lda]) * X[p + (size_t)j * ldx];
            C[i + (size_t)j * ldc] = beta * C[i + (size_t)j * ldc] - s;
        }
}
/* C (m x n) += A B, or -= A B when sub (k inner) */
static inline void jdf_cpu_gemm_nn(const double* A, const double* B, double* C, int m, int n, int k, int ld, bool sub) {
    for (int j = 0; j < n; ++j)
        for (int p = 0; p < k; ++p) {
            const double b = B[p + (size_t)j * ld];
            if (sub)
                for (int i = 0; i < m; ++i) C[i + (size_t)j * ld] -= A[i + (size_t)p * ld] * b;
            else
                for (int i = 0; i < m; ++i) C[i + (size_t)j * ld] += A[i + (size_t)p * ld] * b;
        }
}
/* an info word shared by the CPU bodies of a taskpool: the smaller non-zero index wins */
static inline void jdf_info_min(int* word, int v) {
    int cur = __atomic_load_n(word, __ATOMIC_RELAXED);
    while ((cur == 0 || v < cur) && !__atomic_compare_exchange_n(word, &cur, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}
/* the cubic step term of the factorization priorities (dpotrf_L.jdf): v = 0 leads */
static inline int jdf_prio(int NT, int v) { return (NT - v) * (NT - v) * (NT - v); }
