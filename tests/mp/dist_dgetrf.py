"""Worker for multi-process tests: distributed LU without pivoting and its solve
on host tiles (CPU bodies).

A (N x N, nb x nb tiles, column diagonally dominant) lives on a PA x QA grid and
B (N x NRHS, nb x nbr tiles) on a PB x QB grid of the same ranks. The ranks
factor A with dgetrf_nopiv_new, check their own tiles of L\\U against an
unpivoted LU computed with numpy, then solve A X = B and A^T X = B with
dgetrs_nopiv_new and check their own tiles of X."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def lu_nopiv(S):
    A = S.copy()
    n = A.shape[0]
    for j in range(n - 1):
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:])
    return A


def main(rank, size, job, N, nb, NRHS, nbr, PA, QA, PB, QB):
    import parsec_amd as pa

    pa.mca_set("device_hip_enabled", "0")
    assert pa.comm_init(rank, size, job, -1) == 0
    ctx = pa.init(2)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=PA, Q=QA)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nbr, N, NRHS, P=PB, Q=QB)
    rng = np.random.default_rng(12)
    R = rng.standard_normal((N, N))
    S = R + np.diag(np.abs(R).sum(axis=0) + 1.0)
    B0 = rng.standard_normal((N, NRHS))

    def fill(M, D, mb, kb):
        for m in range(M.mt):
            for n in range(M.nt):
                if M.rank_of([m, n]) == rank:
                    blk = D[m * mb:(m + 1) * mb, n * kb:(n + 1) * kb]
                    t = M.tile(m, n)
                    t[:, :] = 0.0
                    t[:blk.shape[0], :blk.shape[1]] = blk
                    M.mark_host_modified(m, n)

    def max_err(M, D, mb, kb):
        err = 0.0
        for m in range(M.mt):
            for n in range(M.nt):
                if M.rank_of([m, n]) == rank:
                    blk = D[m * mb:(m + 1) * mb, n * kb:(n + 1) * kb]
                    err = max(err, float(np.abs(M.tile(m, n)[:blk.shape[0], :blk.shape[1]] - blk).max()))
        return err

    def run(tp):
        ctx.add_taskpool(tp)
        ctx.start()
        ctx.wait()

    fill(A, S, nb, nb)
    r = pa.dgetrf_nopiv_new(A)
    assert r is not None
    tp, info = r
    run(tp)
    assert pa.read_int(info) == 0
    err = max_err(A, lu_nopiv(S), nb, nb)
    # the factor-and-solve taskpool is refused on several ranks
    refused = size == 1 or pa.dgesv_nopiv_new(A, B) is None
    for trans in (pa.MATRIX_NOTRANS, pa.MATRIX_TRANS):
        fill(B, B0, nb, nbr)
        tps = pa.dgetrs_nopiv_new(trans, A, B)
        assert tps is not None
        run(tps)
        pa.taskpool_free(tps)
        X = np.linalg.solve(S.T if trans == pa.MATRIX_TRANS else S, B0)
        err = max(err, max_err(B, X, nb, nbr))
    ctx.fini()
    pa.comm_fini()
    return err, refused


if __name__ == "__main__":
    r, s = int(sys.argv[1]), int(sys.argv[2])
    err, refused = main(r, s, sys.argv[3], *map(int, sys.argv[4:12]))
    print(f"rank {r} err {err:.3e} dgesv refused {refused}", flush=True)
    sys.exit(0 if err < 1e-10 and refused else 1)
