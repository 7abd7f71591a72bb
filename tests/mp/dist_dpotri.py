"""Worker for multi-process tests: the distributed inverse from the Cholesky
factor on host tiles (CPU bodies).

A (N x N, nb x nb tiles) lives on a P x Q grid. The ranks fill their lower tiles
with L = chol(S) (NaN above the diagonal), run dpotri_new and check their own
tiles of the lower triangle against the dense inverse of S. The entrywise bound
is the forward error bound of a backward stable inverse, 4 N eps cond(S)
||S^-1||_2 (S = (R + R^T) / 2 + N I has a condition number below 2)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(rank, size, job, N, nb, P, Q):
    import parsec_amd as pa

    pa.mca_set("device_hip_enabled", "0")
    assert pa.comm_init(rank, size, job, -1) == 0
    ctx = pa.init(2)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=P, Q=Q)
    R = np.random.default_rng(13).random((N, N))
    S = (R + R.T) / 2 + N * np.eye(N)
    L = np.linalg.cholesky(S)
    L[np.triu_indices(N, 1)] = np.nan
    X = np.linalg.inv(S)
    bound = 4 * N * np.finfo(np.float64).eps * np.linalg.cond(S) * np.linalg.norm(X, 2)

    for m in range(A.mt):
        for n in range(A.nt):
            if A.rank_of([m, n]) == rank:
                blk = L[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb]
                t = A.tile(m, n)
                t[:, :] = 0.0
                t[:blk.shape[0], :blk.shape[1]] = blk
                A.mark_host_modified(m, n)

    # the factor-and-invert taskpool is refused on several ranks
    refused = size == 1 or pa.dpoinv_new(pa.MATRIX_LOWER, A) is None
    tp = pa.dpotri_new(pa.MATRIX_LOWER, A)
    assert tp is not None
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()
    pa.taskpool_free(tp)

    err, upper_ok = 0.0, True
    for m in range(A.mt):
        for n in range(A.nt):
            if A.rank_of([m, n]) != rank:
                continue
            want = X[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb]
            got = A.tile(m, n)[:want.shape[0], :want.shape[1]]
            if m > n:
                err = max(err, float(np.abs(got - want).max()))
            elif m == n:
                lo = np.tril_indices(want.shape[0])
                err = max(err, float(np.abs(got[lo] - want[lo]).max()))
                upper_ok = upper_ok and bool(np.isnan(got[np.triu_indices(want.shape[0], 1)]).all())
            else:
                upper_ok = upper_ok and bool(np.isnan(got).all())
    ctx.fini()
    pa.comm_fini()
    return err, bound, refused, upper_ok


if __name__ == "__main__":
    r, s = int(sys.argv[1]), int(sys.argv[2])
    err, bound, refused, upper_ok = main(r, s, sys.argv[3], *map(int, sys.argv[4:8]))
    print(f"rank {r} err {err:.3e} bound {bound:.3e} dpoinv refused {refused} upper untouched {upper_ok}", flush=True)
    sys.exit(0 if err <= bound and refused and upper_ok else 1)
