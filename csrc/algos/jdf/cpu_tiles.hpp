// CPU reference tile routines and small helpers shared by the JDF prologues in
// this directory (dtrsm_left, dgetrf_nopiv, dtrtri_L, dlauum_L, dpotrf_L): plain
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
#include <cstddef>

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
