/* LU without pivoting through the public C API on one rank:
 * parsec_dgetrf_nopiv_New on an N x N column diagonally dominant matrix,
 * parsec_dgetrs_nopiv_New (NoTrans, then Trans on a fresh right-hand side) on an
 * N x NRHS right-hand side (nb x nb/2 tiles), with the normwise backward error
 * of op(A) X = B; and parsec_dgesv_nopiv_New on a fresh copy, which must give the
 * same X as factor + solve. CPU bodies with PARSEC_MCA_device_hip_enabled=0, HIP
 * bodies otherwise.
 *   argv: [N] [nb] [NRHS]   (default 300 64 96) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parsec.h"

static double a_of(int i, int j, int n) {
  /* not symmetric; |off-diagonal| <= 0.5, so a diagonal of n dominates every column */
  double v = (double)((i * 131 + j * 71 + (i * j) % 13) % 97) / 97.0 - 0.5;
  if (i == j) v += (double)n;
  return v;
}
static double b_of(int i, int j) { return (double)((i * 37 + j * 101) % 89) / 89.0 - 0.5; }

static double* tile_of(parsec_matrix_block_cyclic_t* M, int m, int n) {
  return (double*)parsec_data_copy_get_ptr(parsec_data_get_copy(M->super.super.data_of(&M->super.super, m, n), 0));
}

static void fill_a(parsec_matrix_block_cyclic_t* A, int N, int nb) {
  const int NT = (N + nb - 1) / nb;
  for (int m = 0; m < NT; ++m)
    for (int n = 0; n < NT; ++n) {
      double* t = tile_of(A, m, n);
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) t[(size_t)c * nb + r] = (m * nb + r < N && n * nb + c < N) ? a_of(m * nb + r, n * nb + c, N) : 0.0;
    }
}

static void fill_b(parsec_matrix_block_cyclic_t* B, int N, int NRHS, int nb, int nbr) {
  const int NT = (N + nb - 1) / nb, NTB = (NRHS + nbr - 1) / nbr;
  for (int m = 0; m < NT; ++m)
    for (int n = 0; n < NTB; ++n) {
      double* t = tile_of(B, m, n);
      for (int c = 0; c < nbr; ++c)
        for (int r = 0; r < nb; ++r) t[(size_t)c * nb + r] = (m * nb + r < N && n * nbr + c < NRHS) ? b_of(m * nb + r, n * nbr + c) : 0.0;
    }
}

static void run(parsec_context_t* ctx, parsec_taskpool_t* tp) {
  parsec_context_add_taskpool(ctx, tp);
  parsec_context_start(ctx);
  parsec_context_wait(ctx);
  parsec_taskpool_free(tp);
}

/* || op(A) X - B ||_F / (|| A ||_F || X ||_F + || B ||_F) with X gathered from B's tiles */
static double backward_error(parsec_matrix_block_cyclic_t* B, double* X, int N, int NRHS, int nb, int nbr, int trans) {
  const int NT = (N + nb - 1) / nb, NTB = (NRHS + nbr - 1) / nbr;
  for (int m = 0; m < NT; ++m)
    for (int n = 0; n < NTB; ++n) {
      const double* t = tile_of(B, m, n);
      for (int c = 0; c < nbr && n * nbr + c < NRHS; ++c)
        for (int r = 0; r < nb && m * nb + r < N; ++r) X[(size_t)(n * nbr + c) * N + m * nb + r] = t[(size_t)c * nb + r];
    }
  double na = 0.0, nx = 0.0, nbn = 0.0, nr = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) na += a_of(i, j, N) * a_of(i, j, N);
  for (int j = 0; j < NRHS; ++j)
    for (int i = 0; i < N; ++i) {
      double s = -b_of(i, j);
      for (int p = 0; p < N; ++p) s += (trans ? a_of(p, i, N) : a_of(i, p, N)) * X[(size_t)j * N + p];
      nr += s * s;
      nx += X[(size_t)j * N + i] * X[(size_t)j * N + i];
      nbn += b_of(i, j) * b_of(i, j);
    }
  return sqrt(nr) / (sqrt(na) * sqrt(nx) + sqrt(nbn));
}

int main(int argc, char** argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 300;
  const int nb = argc > 2 ? atoi(argv[2]) : 64;
  const int NRHS = argc > 3 ? atoi(argv[3]) : 96;
  const int nbr = nb / 2 > 0 ? nb / 2 : 1;
  parsec_context_t* ctx = parsec_init(2, &argc, &argv);
  const int rank = parsec_context_rank(ctx);
  parsec_matrix_block_cyclic_t A, B;
  parsec_matrix_block_cyclic_init(&A, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nb, N, N, 0, 0, N, N, 1, 1, 1, 1, 0, 0);
  A.mat = parsec_data_allocate((size_t)A.super.nb_local_tiles * nb * nb * sizeof(double));
  parsec_data_collection_set_key(&A.super.super, "A");
  parsec_matrix_block_cyclic_init(&B, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nbr, N, NRHS, 0, 0, N, NRHS, 1, 1, 1, 1, 0, 0);
  B.mat = parsec_data_allocate((size_t)B.super.nb_local_tiles * nb * nbr * sizeof(double));
  parsec_data_collection_set_key(&B.super.super, "B");
  double* X = (double*)malloc((size_t)N * NRHS * sizeof(double));
  double* X2 = (double*)malloc((size_t)N * NRHS * sizeof(double));

  /* factor, then solve both ways */
  fill_a(&A, N, nb);
  fill_b(&B, N, NRHS, nb, nbr);
  int info = -1;
  parsec_taskpool_t* tp = parsec_dgetrf_nopiv_New(&A.super, &info);
  int ok = tp != NULL;
  double err = -1.0, errt = -1.0, err2 = -1.0, diff = 0.0;
  if (ok) {
    run(ctx, tp);
    ok = info == 0;
    tp = parsec_dgetrs_nopiv_New(PARSEC_MATRIX_NOTRANS, &A.super, &B.super);
    ok = ok && tp != NULL;
    if (tp) {
      run(ctx, tp);
      err = backward_error(&B, X, N, NRHS, nb, nbr, 0);
    }
    fill_b(&B, N, NRHS, nb, nbr);
    tp = parsec_dgetrs_nopiv_New(PARSEC_MATRIX_TRANS, &A.super, &B.super);
    ok = ok && tp != NULL;
    if (tp) {
      run(ctx, tp);
      errt = backward_error(&B, X2, N, NRHS, nb, nbr, 1);
    }
  }
  /* the same in one taskpool */
  fill_a(&A, N, nb);
  fill_b(&B, N, NRHS, nb, nbr);
  int info2 = -1;
  tp = parsec_dgesv_nopiv_New(&A.super, &B.super, &info2);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    err2 = backward_error(&B, X2, N, NRHS, nb, nbr, 0);
    for (size_t i = 0; i < (size_t)N * NRHS; ++i)
      if (fabs(X[i] - X2[i]) > diff) diff = fabs(X[i] - X2[i]);
  }
  /* unsupported requests are refused, not fatal */
  int scratch = 0;
  const int refused = parsec_dgetrs_nopiv_New(PARSEC_MATRIX_CONJTRANS, &A.super, &B.super) == NULL && parsec_dgesv_nopiv_New(&A.super, &B.super, NULL) == NULL &&
                      parsec_dgetrf_nopiv_New(&B.super, &scratch) == NULL;
  /* a well-conditioned system (the diagonal dominates by a factor ~N / 0.25 N):
   * a backward stable solve stays within a few units of roundoff */
  ok = ok && info2 == 0 && err >= 0.0 && err < 1e-14 && errt >= 0.0 && errt < 1e-14 && err2 >= 0.0 && err2 < 1e-14 && diff == 0.0 && refused;
  free(X);
  free(X2);
  parsec_data_free(A.mat);
  parsec_data_free(B.mat);
  parsec_tiled_matrix_destroy(&A.super);
  parsec_tiled_matrix_destroy(&B.super);
  printf("dgetrf capi N %d nb %d NRHS %d info %d %d backward error %.3e %.3e %.3e diff %.3e refused %d %s\n", N, nb, NRHS, info, info2, err, errt, err2, diff,
         refused, ok ? "ok" : "FAILED");
  parsec_fini(&ctx);
  return ok ? 0 : 1;
}
