/* LU with incremental pivoting through the public C API on one rank:
 * parsec_dgetrf_incpiv_New on an N x N pseudo-random matrix with a zero diagonal
 * (it needs pivoting: parsec_dgetrf_nopiv_New reports info = 1 on it), then
 * parsec_dgetrs_incpiv_New on an N x NRHS right-hand side (nb x nb/2 tiles) with
 * the normwise backward error of A X = B; parsec_dgesv_incpiv_New on a fresh
 * copy, which must give the same X; and the zero-column rule (info = column + 1,
 * B untouched). CPU bodies with PARSEC_MCA_device_hip_enabled=0, HIP bodies
 * otherwise.
 *   argv: [N] [nb] [NRHS]   (default 300 64 96) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parsec.h"

static int zero_col = -1; /* a column of A filled with zeros, or -1 */

static double unit_hash(unsigned long long x) {
  /* splitmix64: uniform in [-0.5, 0.5) */
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  x ^= x >> 31;
  return (double)(x >> 11) / 9007199254740992.0 - 0.5;
}
static double a_of(int i, int j, int n) {
  if (i == j || j == zero_col) return 0.0;
  return unit_hash((unsigned long long)i * (unsigned long long)n + (unsigned long long)j);
}
static double b_of(int i, int j) { return unit_hash(0x100000000ull + (unsigned long long)i * 4099ull + (unsigned long long)j); }

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

static void gather_b(parsec_matrix_block_cyclic_t* B, double* X, int N, int NRHS, int nb, int nbr) {
  const int NT = (N + nb - 1) / nb, NTB = (NRHS + nbr - 1) / nbr;
  for (int m = 0; m < NT; ++m)
    for (int n = 0; n < NTB; ++n) {
      const double* t = tile_of(B, m, n);
      for (int c = 0; c < nbr && n * nbr + c < NRHS; ++c)
        for (int r = 0; r < nb && m * nb + r < N; ++r) X[(size_t)(n * nbr + c) * N + m * nb + r] = t[(size_t)c * nb + r];
    }
}

/* || A X - B ||_F / (|| A ||_F || X ||_F + || B ||_F) */
static double backward_error(const double* X, int N, int NRHS) {
  double na = 0.0, nx = 0.0, nbn = 0.0, nr = 0.0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) na += a_of(i, j, N) * a_of(i, j, N);
  for (int j = 0; j < NRHS; ++j)
    for (int i = 0; i < N; ++i) {
      double s = -b_of(i, j);
      for (int p = 0; p < N; ++p) s += a_of(i, p, N) * X[(size_t)j * N + p];
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
  parsec_matrix_block_cyclic_t A, L, B;
  parsec_matrix_block_cyclic_init(&A, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nb, N, N, 0, 0, N, N, 1, 1, 1, 1, 0, 0);
  A.mat = parsec_data_allocate((size_t)A.super.nb_local_tiles * nb * nb * sizeof(double));
  parsec_data_collection_set_key(&A.super.super, "A");
  parsec_matrix_block_cyclic_init(&L, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nb, N, N, 0, 0, N, N, 1, 1, 1, 1, 0, 0);
  L.mat = parsec_data_allocate((size_t)L.super.nb_local_tiles * nb * nb * sizeof(double));
  parsec_data_collection_set_key(&L.super.super, "L");
  memset(L.mat, 0x7f, (size_t)L.super.nb_local_tiles * nb * nb * sizeof(double)); /* its contents on entry do not matter */
  parsec_matrix_block_cyclic_init(&B, PARSEC_MATRIX_DOUBLE, PARSEC_MATRIX_TILE, rank, nb, nbr, N, NRHS, 0, 0, N, NRHS, 1, 1, 1, 1, 0, 0);
  B.mat = parsec_data_allocate((size_t)B.super.nb_local_tiles * nb * nbr * sizeof(double));
  parsec_data_collection_set_key(&B.super.super, "B");
  double* X = (double*)malloc((size_t)N * NRHS * sizeof(double));
  double* X2 = (double*)malloc((size_t)N * NRHS * sizeof(double));

  /* the unpivoted factorization stops at the first (zero) diagonal entry */
  fill_a(&A, N, nb);
  int info_nopiv = -1;
  parsec_taskpool_t* tp = parsec_dgetrf_nopiv_New(&A.super, &info_nopiv);
  int ok = tp != NULL;
  if (tp) run(ctx, tp);
  ok = ok && info_nopiv == 1;

  /* factor, then solve */
  fill_a(&A, N, nb);
  fill_b(&B, N, NRHS, nb, nbr);
  int info = -1;
  double err = -1.0, err2 = -1.0, diff = 0.0;
  tp = parsec_dgetrf_incpiv_New(&A.super, &L.super, &info);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    ok = ok && info == 0;
    tp = parsec_dgetrs_incpiv_New(PARSEC_MATRIX_NOTRANS, &A.super, &L.super, &B.super);
    ok = ok && tp != NULL;
    if (tp) {
      run(ctx, tp);
      gather_b(&B, X, N, NRHS, nb, nbr);
      err = backward_error(X, N, NRHS);
    }
  }
  /* the same in one taskpool */
  fill_a(&A, N, nb);
  fill_b(&B, N, NRHS, nb, nbr);
  int info2 = -1;
  tp = parsec_dgesv_incpiv_New(&A.super, &L.super, &B.super, &info2);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_b(&B, X2, N, NRHS, nb, nbr);
    err2 = backward_error(X2, N, NRHS);
    for (size_t i = 0; i < (size_t)N * NRHS; ++i)
      if (fabs(X[i] - X2[i]) > diff) diff = fabs(X[i] - X2[i]);
  }
  /* a column of zeros: info names it and B is left as it was */
  zero_col = N / 2 + 3;
  fill_a(&A, N, nb);
  fill_b(&B, N, NRHS, nb, nbr);
  int info3 = -1, untouched = 1;
  tp = parsec_dgesv_incpiv_New(&A.super, &L.super, &B.super, &info3);
  ok = ok && tp != NULL;
  if (tp) {
    run(ctx, tp);
    gather_b(&B, X2, N, NRHS, nb, nbr);
    for (int j = 0; j < NRHS; ++j)
      for (int i = 0; i < N; ++i) untouched = untouched && X2[(size_t)j * N + i] == b_of(i, j);
  }
  ok = ok && info3 == zero_col + 1 && untouched;
  zero_col = -1;
  /* unsupported requests are refused, not fatal */
  int scratch = 0;
  const int refused = parsec_dgetrs_incpiv_New(PARSEC_MATRIX_TRANS, &A.super, &L.super, &B.super) == NULL &&
                      parsec_dgesv_incpiv_New(&A.super, &L.super, &B.super, NULL) == NULL && parsec_dgetrf_incpiv_New(&A.super, &B.super, &scratch) == NULL &&
                      parsec_dgetrf_incpiv_New(&B.super, &L.super, &scratch) == NULL;
  /* Entries uniform in [-0.5, 0.5): the condition number does not enter the
   * backward error, which a pivoted LU keeps within N eps times the element
   * growth. N eps = 3e-14 at N = 300 and pairwise pivoting over 5 tile rows
   * grows elements by a small factor, so 1e-12 leaves a factor 30. */
  ok = ok && info2 == 0 && err >= 0.0 && err < 1e-12 && err2 >= 0.0 && err2 < 1e-12 && diff == 0.0 && refused;
  free(X);
  free(X2);
  parsec_data_free(A.mat);
  parsec_data_free(L.mat);
  parsec_data_free(B.mat);
  parsec_tiled_matrix_destroy(&A.super);
  parsec_tiled_matrix_destroy(&L.super);
  parsec_tiled_matrix_destroy(&B.super);
  printf("dgetrf_incpiv capi N %d nb %d NRHS %d info %d %d %d (nopiv %d) backward error %.3e %.3e diff %.3e untouched %d refused %d %s\n", N, nb, NRHS, info, info2,
         info3, info_nopiv, err, err2, diff, untouched, refused, ok ? "ok" : "FAILED");
  parsec_fini(&ctx);
  return ok ? 0 : 1;
}
