"""Worker for multi-process tests: distributed tile LU with incremental pivoting
and its solve on host tiles (CPU bodies).

A (N x N, nb x nb tiles, standard normal: it needs pivoting) and its companion
L live on a PA x QA grid and B (N x NRHS, nb x nbr tiles) on a PB x QB grid of
the same ranks. The ranks factor A with dgetrf_incpiv_new, solve A X = B with
dgetrs_incpiv_new and check their own tiles of X against numpy.linalg.solve."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main(rank, size, job, N, nb, NRHS, nbr, PA, QA, PB, QB):
    import parsec_amd as pa

    pa.mca_set("device_hip_enabled", "0")
    assert pa.comm_init(rank, size, job, -1) == 0
    ctx = pa.init(2)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=PA, Q=QA)
    L = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=PA, Q=QA)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nbr, N, NRHS, P=PB, Q=QB)
    rng = np.random.default_rng(12)
    S = rng.standard_normal((N, N))
    B0 = rng.standard_normal((N, NRHS))

    def fill(M, D, mb, kb):
        for m in range(M.mt):
            for n in range(M.nt):
                if M.rank_of([m, n]) == rank:
                    t = M.tile(m, n)
                    if D is None:
                        t[:, :] = np.nan  # L's contents on entry do not matter
                    else:
                        blk = D[m * mb:(m + 1) * mb, n * kb:(n + 1) * kb]
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
    fill(L, None, nb, nb)
    fill(B, B0, nb, nbr)
    r = pa.dgetrf_incpiv_new(A, L)
    assert r is not None
    tp, info = r
    run(tp)
    assert pa.read_int(info) == 0
    # the factor-and-solve taskpool is refused on several ranks
    refused = size == 1 or pa.dgesv_incpiv_new(A, L, B) is None
    # a companion on another grid is refused
    if size > 1:
        Lbad = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=QA * PA, Q=1) if QA > 1 else pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=1, Q=PA)
        refused = refused and pa.dgetrf_incpiv_new(A, Lbad) is None
    tps = pa.dgetrs_incpiv_new(pa.MATRIX_NOTRANS, A, L, B)
    assert tps is not None
    run(tps)
    pa.taskpool_free(tps)
    err = max_err(B, np.linalg.solve(S, B0), nb, nbr)
    ctx.fini()
    pa.comm_fini()
    return err, refused


if __name__ == "__main__":
    r, s = int(sys.argv[1]), int(sys.argv[2])
    err, refused = main(r, s, sys.argv[3], *map(int, sys.argv[4:12]))
    print(f"rank {r} err {err:.3e} dgesv refused {refused}", flush=True)
    sys.exit(0 if err < 1e-9 and refused else 1)
