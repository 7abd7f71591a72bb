/* Least squares through the public C API on one rank: parsec_dgels_New factors
 * the M x N matrix A (into A and T) and solves min ||A X - B||_F for an
 * M x NRHS right-hand side (nb x nb/2 tiles); then B is restored and
 * parsec_dgeqrs_New solves again from the stored factor, which must give the
 * same X; parsec_dormqr_New applies Q^T then Q to a third copy, which must give
 * B back. Checked with the normal-equations residual
 * ||A^T (A X - B)|| / (||A||^2 ||X|| + ||A|| ||B||). CPU bodies with
 * PARSEC_MCA_device_hip_enabled=0, HIP bodies otherwise.
 *   argv: [M] [N] [nb] [NRHS]   (default 200 120 32 40) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parsec.h"

static double a_of(int i, int j) {
  /* full column rank: a dominant diagonal on top of pseudo-random entries */
  double v = (double)((i * 131 + j * 71 + (i * j) % 13) % 97) / 97.0 - 0.5;
  if (i == j) v += 4.0;
  return v;
}
static double b_of(int i, int j) { return (double)((i * 37 + j * 101) % 89) / 89.0 - 0.5; }

static double* tile_of(parsec_matrix_block_cyclic_t* M, int m, int n) {
  return (double*)parsec_data_copy_get_ptr(parsec_data_get_copy(M->super.super.data_of(&M->super.super, m, n), 0));
}

static void fill_a(parsec_matrix_block_cyclic_t* A, int M, int N, int nb) {
  const int MT = (M + nb - 1) / nb, NT = (N + nb - 1) / nb;
  for (int m = 0; m < MT; ++m)
    for (int n = 0; n < NT; ++n) {
      double* t = tile_of(A, m, n);
      for (int c = 0; c < nb; ++c)
        for (int r = 0; r < nb; ++r) t[(size_t)c * nb + r] = (m * nb + r < M && n * nb + c < N) ? a_of(m * nb + r, n * nb + c) : 0.0;
    }
}

static void fill_b(parsec_matrix_block_cyclic_t* B, int M, int NRHS, int nb, int nbr) {
  const int MT = (M + nb - 1) / nb, NTB = (NRHS + nbr - 1) / nbr;
  for (int m = 0; m < MT; ++m)
    for (int n = 0; n < NTB; ++n) {
      double* t = tile_of(B, m, n);
      for (int c = 0; c < nbr; ++c)
        for (int r = 0; r < nb; ++r) t[(size_t)c * nb + r] = (m * nb + r < M && n * nbr + c < NRHS) ? b_of(m * nb + r, n * nbr + c) : 0.0;
    }
}

static void gather_b(parsec_matrix_block_cyclic_t* B, double* X, int M, int NRHS, int nb, int nbr) {
  const int MT = (M + nb - 1) / nb, NTB = (NRHS + nbr - 1) / nbr;
  for (int m = 0; m < MT; ++m)
    for (int n = 0; n < NTB; ++n) {
      const double* t = tile_of(B, m, n);
      for (int c = 0; c < nbr && n * nbr + c < NRHS; ++c)
        for (int r = 0; r < nb && m * nb + r < M; ++r) X[(size_t)(n * nbr + c) * M + m * nb + r] = t[(size_t)c * nb + r];
    }
}

static void run(parsec_context_t* ctx, parsec_taskpool_t* tp) {
  parsec_context_add_taskpool(ctx, tp);
  parsec_context_start(ctx);
  parsec_context_wait(ctx);
  parsec_taskpool_free(tp);
}

/* ||A^T (A X - B)||_F / (||A||_F^2 ||X||_F + ||A||_F ||B||_F), X = rows 0..N-1 of G (ld M) */
static double normal_residual(const double* G, int M, int N, int NRHS) {
  double na = 0.0, nx = 0.0, nbn = 0.0, ng = 0.0;
  double* res = (double*)malloc((size_t)M * sizeof(double));
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) na += a_of(i, j) * a_of(i, j);
  for (int j = 0; j < NRHS; ++j) {
    const double* x = G + (size_t)j * M;
    for (int i = 0; i < M; ++i) {
      double s = -b_of(i, j);
      for (int p = 0; p < N; ++p) s += a_of(i, p) * x[p];
      res[i] = s;
      nbn += b_of(i, j) * b_of(i, j);
    }
    for (int p = 0; p < N; ++p) {
      double g = 0.0;
      for (int i = 0; i < M; ++i) g += a_of(i, p) * res[i];
      ng += g * g;
      nx += x[p] * x[p];
    }
  }
  free(res);
  return sqrt(ng) / (na * sqrt(nx) + sqrt(na) * sqrt(nbn));
}

int main(int argc, char** argv) {
  const int M = argc > 1 ? atoi(argv[1]) : 200;
  const int N = argc > 2 ? atoi(argv[2]) : 120;
  const int nb = argc > 3 ? atoi(argv[3]) : 32;
  const int NRHS = argc > 4 ? atoi(argv[4]) : 40;
  const int nbr = nb / 2 > 0 ? nb / 2 : 1;
  parsec_context_t* ctx = parsec_init(2, &argc, &argv);
  const int rank = parsec_context_rank(ctx);
  parsec_matrix_block_cyclic_t A, T, B;
  parsec_matrix_block_cyclic_init(&A, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nb, M, N, 0, 0, M, N, 1, 1, 1, 1, 0, 0);
  A.mat = parsec_data_allocate((size_t)A.super.nb_local_tiles * nb * nb * sizeof(double));
  parsec_data_collection_set_key(&A.super.super, "A");
  parsec_matrix_block_cyclic_init(&T, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nb, M, N, 0, 0, M, N, 1, 1, 1, 1, 0, 0);
  T.mat = parsec_data_allocate((size_t)T.super.nb_local_tiles * nb * nb * sizeof(double));
  memset(T.mat, 0, (size_t)T.super.nb_local_tiles * nb * nb * sizeof(double));
  parsec_data_collection_set_key(&T.super.super, "T");
  parsec_matrix_block_cyclic_init(&B, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nbr, M, NRHS, 0, 0, M, NRHS, 1, 1, 1, 1, 0, 0);
  B.mat = parsec_data_allocate((size_t)B.super.nb_local_tiles * nb * nbr * sizeof(double));
  parsec_data_collection_set_key(&B.super.super, "B");
  double* G = (double*)malloc((size_t)M * NRHS * sizeof(double));
  double* G2 = (double*)malloc((size_t)M * NRHS * sizeof(double));

  /* factor and solve in one taskpool */
  fill_a(&A, M, N, nb);
  fill_b(&B, M, NRHS, nb, nbr);
  double err = -1.0, err2 = -1.0, diff = 0.0, back = 0.0;
  parsec_taskpool_t* tp = parsec_dgels_New(&A.super, &T.super, &B.super);
  int ok = tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_b(&B, G, M, NRHS, nb, nbr);
    err = normal_residual(G, M, N, NRHS);
  }
  /* solve again from the stored factor */
  fill_b(&B, M, NRHS, nb, nbr);
  tp = parsec_dgeqrs_New(&A.super, &T.super, &B.super);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_b(&B, G2, M, NRHS, nb, nbr);
    err2 = normal_residual(G2, M, N, NRHS);
    for (int j = 0; j < NRHS; ++j)
      for (int i = 0; i < N; ++i)
        if (fabs(G[(size_t)j * M + i] - G2[(size_t)j * M + i]) > diff) diff = fabs(G[(size_t)j * M + i] - G2[(size_t)j * M + i]);
  }
  /* Q Q^T B = B */
  fill_b(&B, M, NRHS, nb, nbr);
  parsec_taskpool_t* qt = parsec_dormqr_New(PARSEC_MATRIX_LEFT, PARSEC_MATRIX_TRANS, &A.super, &T.super, &B.super);
  parsec_taskpool_t* q = parsec_dormqr_New(PARSEC_MATRIX_LEFT, PARSEC_MATRIX_NOTRANS, &A.super, &T.super, &B.super);
  ok = ok && qt != NULL && q != NULL;
  if (qt && q) {
    run(ctx, qt);
    run(ctx, q);
    gather_b(&B, G2, M, NRHS, nb, nbr);
    for (int j = 0; j < NRHS; ++j)
      for (int i = 0; i < M; ++i)
        if (fabs(G2[(size_t)j * M + i] - b_of(i, j)) > back) back = fabs(G2[(size_t)j * M + i] - b_of(i, j));
  }
  /* an unsupported request is refused, not fatal */
  const int refused = parsec_dormqr_New(PARSEC_MATRIX_RIGHT, PARSEC_MATRIX_TRANS, &A.super, &T.super, &B.super) == NULL &&
                      parsec_dgeqrs_New(&A.super, &B.super, &B.super) == NULL;
  /* |b| <= 0.5: 1e-13 is the orthogonality threshold of the QR tests */
  ok = ok && err >= 0.0 && err < 1e-14 && err2 >= 0.0 && err2 < 1e-14 && diff < 1e-12 && back < 1e-13 && refused;
  free(G);
  free(G2);
  parsec_data_free(A.mat);
  parsec_data_free(T.mat);
  parsec_data_free(B.mat);
  parsec_tiled_matrix_destroy(&A.super);
  parsec_tiled_matrix_destroy(&T.super);
  parsec_tiled_matrix_destroy(&B.super);
  printf("dgels capi M %d N %d nb %d NRHS %d normal-equations residual %.3e %.3e diff %.3e QQ^TB-B %.3e refused %d %s\n", M, N, nb, NRHS, err, err2, diff, back,
         refused, ok ? "ok" : "FAILED");
  parsec_fini(&ctx);
  return ok ? 0 : 1;
}
