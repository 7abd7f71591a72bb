/* The inverse with the Cholesky factor through the public C API on one rank: on
 * an N x N SPD matrix S, parsec_dpotrf_New, then parsec_dtrtri_New on the factor
 * L (checked through || X L - I ||), parsec_dlauum_New on a fresh copy of L
 * (against L^T L), parsec_dpotri_New on another (|| S X - I ||), and
 * parsec_dpoinv_New on S itself, which must give the same inverse as factor +
 * dpotri. Only the lower triangle is ever read back. CPU bodies with
 * PARSEC_MCA_device_hip_enabled=0, HIP bodies otherwise.
 *   argv: [N] [nb]   (default 300 64) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parsec.h"

static double s_of(int i, int j, int n) {
  /* symmetric; |off-diagonal| <= 0.5, so a diagonal of n makes it positive definite */
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  double v = (double)((lo * 131 + hi * 71 + (lo * hi) % 13) % 97) / 97.0 - 0.5;
  if (i == j) v += (double)n;
  return v;
}

static double* tile_of(parsec_matrix_block_cyclic_t* M, int m, int n) {
  return (double*)parsec_data_copy_get_ptr(parsec_data_get_copy(M->super.super.data_of(&M->super.super, m, n), 0));
}

/* tiles := the dense column-major D (ld N); with lower_only the strict upper triangle is zero */
static void scatter(parsec_matrix_block_cyclic_t* A, const double* D, int N, int nb, int lower_only) {
  const int NT = (N + nb - 1) / nb;
  for (int m = 0; m < NT; ++m)
    for (int n = 0; n < NT; ++n) {
      double* t = tile_of(A, m, n);
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) {
          const int i = m * nb + r, j = n * nb + c;
          t[(size_t)c * nb + r] = (i < N && j < N && (!lower_only || i >= j)) ? D[(size_t)j * N + i] : 0.0;
        }
    }
}

/* dense lower triangle (zero above) := the tiles */
static void gather_lower(parsec_matrix_block_cyclic_t* A, double* D, int N, int nb) {
  const int NT = (N + nb - 1) / nb;
  for (int m = 0; m < NT; ++m)
    for (int n = 0; n < NT; ++n) {
      const double* t = tile_of(A, m, n);
      for (int c = 0; c < nb && n * nb + c < N; ++c)
        for (int r = 0; r < nb && m * nb + r < N; ++r) {
          const int i = m * nb + r, j = n * nb + c;
          D[(size_t)j * N + i] = i >= j ? t[(size_t)c * nb + r] : 0.0;
        }
    }
}

static void run(parsec_context_t* ctx, parsec_taskpool_t* tp) {
  parsec_context_add_taskpool(ctx, tp);
  parsec_context_start(ctx);
  parsec_context_wait(ctx);
  parsec_taskpool_free(tp);
}

static double fro(const double* D, int N) {
  double s = 0.0;
  for (size_t i = 0; i < (size_t)N * N; ++i) s += D[i] * D[i];
  return sqrt(s);
}

/* || P Q - I ||_F / (|| P ||_F || Q ||_F), dense column-major */
static double identity_residual(const double* P, const double* Q, int N) {
  double nr = 0.0;
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) {
      double s = i == j ? -1.0 : 0.0;
      for (int p = 0; p < N; ++p) s += P[(size_t)p * N + i] * Q[(size_t)j * N + p];
      nr += s * s;
    }
  return sqrt(nr) / (fro(P, N) * fro(Q, N));
}

int main(int argc, char** argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 300;
  const int nb = argc > 2 ? atoi(argv[2]) : 64;
  parsec_context_t* ctx = parsec_init(2, &argc, &argv);
  const int rank = parsec_context_rank(ctx);
  parsec_matrix_block_cyclic_t A;
  parsec_matrix_block_cyclic_init(&A, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nb, N, N, 0, 0, N, N, 1, 1, 1, 1, 0, 0);
  A.mat = parsec_data_allocate((size_t)A.super.nb_local_tiles * nb * nb * sizeof(double));
  parsec_data_collection_set_key(&A.super.super, "A");
  const size_t nn = (size_t)N * N;
  double* S = (double*)malloc(nn * sizeof(double));
  double* L = (double*)malloc(nn * sizeof(double));
  double* X = (double*)malloc(nn * sizeof(double));
  double* Y = (double*)malloc(nn * sizeof(double));
  for (int j = 0; j < N; ++j)
    for (int i = 0; i < N; ++i) S[(size_t)j * N + i] = s_of(i, j, N);

  /* the factor */
  scatter(&A, S, N, nb, 0);
  int info = -1, info_tri = -1, info_inv = -1;
  parsec_taskpool_t* tp = parsec_dpotrf_New(PARSEC_MATRIX_LOWER, &A.super, &info);
  int ok = tp != NULL;
  double res_tri = -1.0, err_lauum = -1.0, res_inv = -1.0, res_inv2 = -1.0, diff = 0.0;
  if (tp) {
    run(ctx, tp);
    gather_lower(&A, L, N, nb);
  }
  ok = ok && info == 0;
  /* X = L^-1 */
  tp = parsec_dtrtri_New(PARSEC_MATRIX_LOWER, PARSEC_MATRIX_NONUNIT, &A.super, &info_tri);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_lower(&A, X, N, nb);
    res_tri = identity_residual(X, L, N);
  }
  /* lower(L^T L) */
  scatter(&A, L, N, nb, 1);
  tp = parsec_dlauum_New(PARSEC_MATRIX_LOWER, &A.super);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_lower(&A, X, N, nb);
    double num = 0.0, den = 0.0;
    for (int j = 0; j < N; ++j)
      for (int i = j; i < N; ++i) {
        double s = 0.0;
        for (int p = i; p < N; ++p) s += L[(size_t)i * N + p] * L[(size_t)j * N + p];
        num += (X[(size_t)j * N + i] - s) * (X[(size_t)j * N + i] - s);
        den += s * s;
      }
    err_lauum = sqrt(num / den);
  }
  /* the inverse from the factor: X := S^-1, symmetrised from its lower triangle */
  scatter(&A, L, N, nb, 1);
  tp = parsec_dpotri_New(PARSEC_MATRIX_LOWER, &A.super);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_lower(&A, X, N, nb);
    for (int j = 0; j < N; ++j)
      for (int i = 0; i < j; ++i) X[(size_t)j * N + i] = X[(size_t)i * N + j];
    res_inv = identity_residual(S, X, N);
  }
  /* the same in one taskpool, from S */
  scatter(&A, S, N, nb, 0);
  tp = parsec_dpoinv_New(PARSEC_MATRIX_LOWER, &A.super, &info_inv);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_lower(&A, Y, N, nb);
    for (int j = 0; j < N; ++j)
      for (int i = 0; i < j; ++i) Y[(size_t)j * N + i] = Y[(size_t)i * N + j];
    res_inv2 = identity_residual(S, Y, N);
    for (size_t i = 0; i < nn; ++i)
      if (fabs(X[i] - Y[i]) > diff) diff = fabs(X[i] - Y[i]);
  }
  /* unsupported requests are refused, not fatal */
  int scratch = 0;
  const int refused = parsec_dtrtri_New(PARSEC_MATRIX_UPPER, PARSEC_MATRIX_NONUNIT, &A.super, &scratch) == NULL &&
                      parsec_dtrtri_New(PARSEC_MATRIX_LOWER, PARSEC_MATRIX_UNIT, &A.super, &scratch) == NULL &&
                      parsec_dlauum_New(PARSEC_MATRIX_UPPER, &A.super) == NULL && parsec_dpotri_New(PARSEC_MATRIX_UPPER, &A.super) == NULL &&
                      parsec_dpoinv_New(PARSEC_MATRIX_LOWER, &A.super, NULL) == NULL;
  /* a well-conditioned matrix (the diagonal dominates: condition number below
   * 2): backward stable inverses stay within a few units of roundoff, and the
   * product within N eps of its own size */
  ok = ok && info_tri == 0 && info_inv == 0 && res_tri >= 0.0 && res_tri < 1e-15 && err_lauum >= 0.0 && err_lauum < N * 2.3e-16 && res_inv >= 0.0 &&
       res_inv < 1e-15 && res_inv2 >= 0.0 && res_inv2 < 1e-15 && diff == 0.0 && refused;
  free(S);
  free(L);
  free(X);
  free(Y);
  parsec_data_free(A.mat);
  parsec_tiled_matrix_destroy(&A.super);
  printf("dpotri capi N %d nb %d info %d %d %d residual dtrtri %.3e dlauum error %.3e residual dpotri %.3e dpoinv %.3e diff %.3e refused %d %s\n", N, nb, info,
         info_tri, info_inv, res_tri, err_lauum, res_inv, res_inv2, diff, refused, ok ? "ok" : "FAILED");
  parsec_fini(&ctx);
  return ok ? 0 : 1;
}
