"""Worker for multi-process tests: distributed least squares on host tiles (CPU
bodies), dgeqrf then dgeqrs, and dgels in one taskpool.

A and T (M x N, nb x nb tiles) live on a PA x QA grid and B (M x NRHS, nb x nbr
tiles) on a PB x QB grid of the same ranks: V and T reach the tasks, which run
where their B tile lives, through the reader tasks of dormqr.jdf, the tiles of R
through those of dtrsm_left.jdf. Every rank writes its tiles of the two results
(dgeqrs<rank>.npy, dgels<rank>.npy, zeros elsewhere) into outdir; the test adds
them up and checks the residuals. The same matrices as the test: seed 13.
argv: rank size job M N nb NRHS nbr PA QA PB QB outdir"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def _fill(C, rank, S, mb, nb):
    for m in range(C.mt):
        for n in range(C.nt):
            if C.rank_of([m, n]) == rank:
                blk = S[m * mb:(m + 1) * mb, n * nb:(n + 1) * nb]
                t = C.tile(m, n)
                t[:, :] = 0.0
                t[:blk.shape[0], :blk.shape[1]] = blk
                C.mark_host_modified(m, n)


def _run(ctx, tp):
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()


def main(rank, size, job, M, N, nb, NRHS, nbr, PA, QA, PB, QB, outdir):
    import parsec_amd as pa

    pa.mca_set("device_hip_enabled", "0")
    assert pa.comm_init(rank, size, job, -1) == 0
    ctx = pa.init(2)
    rng = np.random.default_rng(13)
    S = rng.standard_normal((M, N))
    B0 = rng.standard_normal((M, NRHS))

    def save(name, B):
        """This rank's tiles of B (zeros elsewhere): the test adds the ranks up."""
        out = np.zeros((M, NRHS))
        for m in range(B.mt):
            for n in range(B.nt):
                if B.rank_of([m, n]) == rank:
                    r, c = min(nb, M - m * nb), min(nbr, NRHS - n * nbr)
                    out[m * nb:m * nb + r, n * nbr:n * nbr + c] = B.tile(m, n)[:r, :c]
        np.save(os.path.join(outdir, f"{name}{rank}.npy"), out)

    # factor, then solve from the stored factor
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, M, N, P=PA, Q=QA)
    T = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, M, N, P=PA, Q=QA)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nbr, M, NRHS, P=PB, Q=QB)
    _fill(A, rank, S, nb, nb)
    _fill(B, rank, B0, nb, nbr)
    _run(ctx, pa.dgeqrf_jdf_new(A, T))
    tp = pa.dgeqrs_new(A, T, B)
    assert tp is not None
    _run(ctx, tp)
    pa.taskpool_free(tp)
    save("dgeqrs", B)

    # factor and solve in one taskpool
    A2 = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, M, N, P=PA, Q=QA)
    T2 = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, M, N, P=PA, Q=QA)
    B2 = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nbr, M, NRHS, P=PB, Q=QB)
    _fill(A2, rank, S, nb, nb)
    _fill(B2, rank, B0, nb, nbr)
    tp = pa.dgels_new(A2, T2, B2)
    assert tp is not None
    _run(ctx, tp)
    pa.taskpool_free(tp)
    save("dgels", B2)

    ctx.fini()
    pa.comm_fini()


if __name__ == "__main__":
    r, s = int(sys.argv[1]), int(sys.argv[2])
    main(r, s, sys.argv[3], *map(int, sys.argv[4:13]), sys.argv[13])
    print(f"rank {r} done", flush=True)
