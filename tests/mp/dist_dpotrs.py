"""Worker for multi-process tests: distributed DPOTRS on host tiles (CPU bodies).

A (the Cholesky factor, N x N, nb x nb tiles) lives on a PA x QA grid and B
(N x NRHS, nb x nbr tiles) on a PB x QB grid of the same ranks: the tiles of L
reach the tasks, which run where their B tile lives, through the reader tasks
of dtrsm_left.jdf."""
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
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nbr, N, NRHS, P=PB, Q=QB)
    rng = np.random.default_rng(11)
    R = rng.standard_normal((N, N))
    S = R @ R.T + N * np.eye(N)
    L = np.linalg.cholesky(S)
    B0 = rng.standard_normal((N, NRHS))
    for m in range(A.mt):
        for n in range(m + 1):
            if A.rank_of([m, n]) == rank:
                t = L[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb].copy()
                if m == n:
                    t[np.triu_indices_from(t, 1)] = np.nan  # the strict upper triangle of L is never used
                A.tile(m, n)[:, :] = t
                A.mark_host_modified(m, n)
    mine = 0
    for m in range(B.mt):
        for n in range(B.nt):
            if B.rank_of([m, n]) == rank:
                B.tile(m, n)[:, :] = B0[m * nb:(m + 1) * nb, n * nbr:(n + 1) * nbr]
                B.mark_host_modified(m, n)
                mine += 1
    tp = pa.dpotrs_new(pa.MATRIX_LOWER, A, B)
    assert tp is not None
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()
    X = np.linalg.solve(L.T, np.linalg.solve(L, B0))
    err = 0.0
    for m in range(B.mt):
        for n in range(B.nt):
            if B.rank_of([m, n]) == rank:
                err = max(err, float(np.abs(B.tile(m, n) - X[m * nb:(m + 1) * nb, n * nbr:(n + 1) * nbr]).max()))
    pa.taskpool_free(tp)
    ctx.fini()
    pa.comm_fini()
    return err, mine


if __name__ == "__main__":
    r, s = int(sys.argv[1]), int(sys.argv[2])
    err, mine = main(r, s, sys.argv[3], *map(int, sys.argv[4:12]))
    print(f"rank {r} tiles {mine} err {err:.3e}", flush=True)
    # a rank may own no tile of B (1 x 3 grid, two tile columns): it still serves its tiles of L
    sys.exit(0 if err < 1e-10 else 1)
