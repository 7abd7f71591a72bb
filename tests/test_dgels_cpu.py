"""DORMQR, DGEQRS and DGELS with the CPU bodies: Q checked from the stored factor
(the first check of the V and T that DGEQRF hands out), least-squares solutions
against numpy, argument checks, several ranks with A and B on different process
grids, and the C API program.

Thresholds: 1e-13 for the orthogonality checks (the one of test_dgeqrf.py on the
CPU), 1e-14 backward / 1e-11 forward for the solutions (those of the DPOTRS
tests; numpy's own QR solve at these shapes gives 1e-17..1e-18 and 2e-15..6e-15
with cond(A) about 8 for Gaussian tall matrices). The residual norms read from
rows N.. of B are Q^T applied to B, so they get the orthogonality threshold,
relative to the largest column norm of B; a square system has no such rows."""
import os
import subprocess

import numpy as np
import pytest

from test_distributed_cpu import run_ranks

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "mp", "dist_dgels.py")

# (M, N, nb, NRHS, nbr): tall with whole tiles; tall with edge tiles in every
# dimension (N not a multiple of nb: the last R block shares its tile row of B
# with residual rows); square
SHAPES = [(96, 64, 16, 24, 8), (70, 50, 16, 13, 8), (64, 64, 16, 16, 16)]
SOURCES = ["jdf", "ir"]


@pytest.fixture
def ctx(pa):
    """A context whose tasks run the CPU bodies, also on a machine with a GPU."""
    pa.mca_set("device_hip_enabled", "0")
    c = pa.init(3)
    try:
        yield c
    finally:
        c.fini()
        pa.mca_unset("device_hip_enabled")


def fill(M, S, mb, nb):
    for m in range(M.mt):
        for n in range(M.nt):
            blk = S[m * mb:(m + 1) * mb, n * nb:(n + 1) * nb]
            t = M.tile(m, n)
            t[:, :] = 0.0
            t[:blk.shape[0], :blk.shape[1]] = blk


def gather(M, rows, cols, mb, nb):
    out = np.zeros((rows, cols))
    for m in range(M.mt):
        for n in range(M.nt):
            r, c = min(mb, rows - m * mb), min(nb, cols - n * nb)
            out[m * mb:m * mb + r, n * nb:n * nb + c] = M.tile(m, n)[:r, :c]
    return out


def run(ctx, tp):
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()


def problem(M, N, NRHS, seed=7):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((M, N)), rng.standard_normal((M, NRHS))


def factor(pa, ctx, S, nb, source):
    """(A, T) holding the tile QR factor of S from the named taskpool."""
    M, N = S.shape
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
    T = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
    fill(A, S, nb, nb)
    run(ctx, pa.dgeqrf_jdf_new(A, T) if source == "jdf" else pa.dgeqrf_new(A, T, 32))
    return A, T


def apply_q(pa, ctx, trans, A, T, X, nb, nbr):
    """op(Q) X through dormqr_new on a fresh collection."""
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, X.shape[0], X.shape[1])
    fill(B, X, nb, nbr)
    tp = pa.dormqr_new(pa.MATRIX_LEFT, pa.MATRIX_TRANS if trans else pa.MATRIX_NOTRANS, A, T, B)
    assert tp is not None
    run(ctx, tp)
    pa.taskpool_free(tp)
    return gather(B, X.shape[0], X.shape[1], nb, nbr)


def check_q(S, R, QtS, B0, QtB, QQtB, tol):
    """The three properties of the Q stored in (A, T); prints the figures."""
    M, N = S.shape
    top = np.zeros((M, N))
    top[:min(M, N)] = np.triu(R)[:min(M, N)]
    e_r = np.linalg.norm(QtS - top) / np.linalg.norm(S)
    e_rt = np.linalg.norm(QQtB - B0) / np.linalg.norm(B0)
    e_n = np.abs(np.linalg.norm(QtB, axis=0) / np.linalg.norm(B0, axis=0) - 1.0).max()
    print(f"Q^T A - [R; 0]: {e_r:.3e}, Q Q^T B - B: {e_rt:.3e}, column norms: {e_n:.3e}")
    assert e_r < tol
    assert e_rt < tol
    assert e_n < tol


def check_solution(S, B0, Bout, N, tol_q, forward):
    """Least-squares checks on the B that dgeqrs / dgels returned; prints the figures."""
    X = Bout[:N]
    nS, nB = np.linalg.norm(S), np.linalg.norm(B0)
    bwd = np.linalg.norm(S.T @ (S @ X - B0)) / (nS * nS * np.linalg.norm(X) + nS * nB)
    print(f"normal equations residual {bwd:.3e}")
    assert bwd < 1e-14
    if forward:
        Xref = np.linalg.lstsq(S, B0, rcond=None)[0]
        fwd = np.linalg.norm(X - Xref) / np.linalg.norm(Xref)
        print(f"forward error {fwd:.3e}")
        assert fwd < 1e-11
    if S.shape[0] == N:
        return  # square: no residual rows
    # rows N.. hold the residual components: Q^T (B - A X) = [0; them]
    res = np.linalg.norm(S @ X - B0, axis=0)
    got = np.linalg.norm(Bout[N:], axis=0)
    e_res = np.abs(got - res).max() / np.linalg.norm(B0, axis=0).max()
    print(f"residual norms {e_res:.3e}")
    assert e_res < tol_q


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("M,N,nb,NRHS,nbr", SHAPES)
def test_dormqr_q_from_stored_factor(pa, ctx, M, N, nb, NRHS, nbr, source):
    S, B0 = problem(M, N, NRHS)
    A, T = factor(pa, ctx, S, nb, source)
    R = gather(A, M, N, nb, nb)
    QtS = apply_q(pa, ctx, 1, A, T, S, nb, nbr)
    QtB = apply_q(pa, ctx, 1, A, T, B0, nb, nbr)
    QQtB = apply_q(pa, ctx, 0, A, T, QtB, nb, nbr)
    check_q(S, R, QtS, B0, QtB, QQtB, 1e-13)


def test_dormqr_wide_factor(pa, ctx):
    """M < N: min(MT, NT) panels; Q is M x M."""
    M, N, nb, NRHS, nbr = 48, 80, 16, 13, 8
    S, B0 = problem(M, N, NRHS)
    A, T = factor(pa, ctx, S, nb, "jdf")
    R = gather(A, M, N, nb, nb)
    QtS = apply_q(pa, ctx, 1, A, T, S, nb, nbr)
    QtB = apply_q(pa, ctx, 1, A, T, B0, nb, nbr)
    QQtB = apply_q(pa, ctx, 0, A, T, QtB, nb, nbr)
    check_q(S, R, QtS, B0, QtB, QQtB, 1e-13)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("M,N,nb,NRHS,nbr", SHAPES)
def test_dgeqrs_cpu(pa, ctx, M, N, nb, NRHS, nbr, source):
    S, B0 = problem(M, N, NRHS)
    A, T = factor(pa, ctx, S, nb, source)
    QtB = apply_q(pa, ctx, 1, A, T, B0, nb, nbr)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, M, NRHS)
    fill(B, B0, nb, nbr)
    tp = pa.dgeqrs_new(A, T, B)
    assert tp is not None
    run(ctx, tp)
    pa.taskpool_free(tp)
    Bout = gather(B, M, NRHS, nb, nbr)
    check_solution(S, B0, Bout, N, 1e-13, forward=M > N)
    # the solve with R leaves every row >= N as Q^T B left it, also those that
    # share the last tile row with X
    assert np.array_equal(Bout[N:], QtB[N:])


@pytest.mark.parametrize("M,N,nb,NRHS,nbr", SHAPES)
def test_dgels_cpu(pa, ctx, M, N, nb, NRHS, nbr):
    S, B0 = problem(M, N, NRHS, seed=9)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
    T = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, M, NRHS)
    fill(A, S, nb, nb)
    fill(B, B0, nb, nbr)
    tp = pa.dgels_new(A, T, B)
    assert tp is not None
    run(ctx, tp)
    pa.taskpool_free(tp)
    check_solution(S, B0, gather(B, M, NRHS, nb, nbr), N, 1e-13, forward=M > N)


def test_unsupported_requests_return_none(pa, ctx):
    M, N, nb, NRHS, nbr = 64, 32, 16, 16, 8
    S, B0 = problem(M, N, NRHS)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
    T = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, M, NRHS)
    fill(A, S, nb, nb)
    fill(B, B0, nb, nbr)
    # the good request is accepted (and released unused)
    tp = pa.dormqr_new(pa.MATRIX_LEFT, pa.MATRIX_TRANS, A, T, B)
    assert tp is not None
    pa.taskpool_free(tp)
    assert pa.dormqr_new(pa.MATRIX_RIGHT, pa.MATRIX_TRANS, A, T, B) is None
    assert pa.dormqr_new(pa.MATRIX_LEFT, pa.MATRIX_CONJTRANS, A, T, B) is None
    assert pa.dormqr_new(pa.MATRIX_LEFT, 7, A, T, B) is None
    bad = {
        "M < N": (pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, M), pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, M),
                  pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)),
        "non-square tiles": (pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, 8, M, N), pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, 8, M, N), B),
        "B.mb != A.mb": (A, T, pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, 8, nbr, M, NRHS)),
        "B.m != A.m": (A, T, pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, M + nb, NRHS)),
        "T tile size": (A, pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, 32, 32, M, N), B),
        "T tile grid": (A, pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N + nb), B),
    }
    for why, (a, t, b) in bad.items():
        assert pa.dgeqrs_new(a, t, b) is None, why
        assert pa.dgels_new(a, t, b) is None, why
        if why != "M < N":
            assert pa.dormqr_new(pa.MATRIX_LEFT, pa.MATRIX_NOTRANS, a, t, b) is None, why
    # the upper solve stays internal
    Asq = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, M)
    assert pa.dtrsm_new(pa.MATRIX_LEFT, pa.MATRIX_UPPER, pa.MATRIX_NOTRANS, pa.MATRIX_NONUNIT, 1.0, Asq, B) is None
    assert np.array_equal(gather(B, M, NRHS, nb, nbr), B0)  # B untouched by the refusals


@pytest.mark.parametrize("nranks,PA,QA,PB,QB", [
    (2, 2, 1, 1, 2),  # A by rows, B by columns: every V and T tile crosses ranks
    (4, 2, 2, 4, 1),
])
def test_dgels_multirank(pa, tmp_path, nranks, PA, QA, PB, QB):
    """dgeqrf then dgeqrs, and dgels in one taskpool, on several ranks; the
    ranks' tiles of B are added up here and get the one-rank checks."""
    M, N, nb, NRHS, nbr = 112, 80, 16, 24, 8
    outs = run_ranks(nranks, M, N, nb, NRHS, nbr, PA, QA, PB, QB, str(tmp_path), worker=WORKER)
    for rc, out in outs:
        assert rc == 0, out
    rng = np.random.default_rng(13)  # the worker's matrices
    S = rng.standard_normal((M, N))
    B0 = rng.standard_normal((M, NRHS))
    for name in ("dgeqrs", "dgels"):
        Bout = sum(np.load(tmp_path / f"{name}{r}.npy") for r in range(nranks))
        check_solution(S, B0, Bout, N, 1e-13, forward=True)


def test_dgels_capi(pa, tmp_path):
    """C program on the public header: factor and solve, check the
    normal-equations residual, and a refused request."""
    exe = tmp_path / "dgels_capi"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{ROOT}/include", os.path.join(HERE, "capi", "dgels_capi.c"), "-o", str(exe),
           f"-L{ROOT}/parsec_amd/lib", "-lparsec_amd", f"-Wl,-rpath,{ROOT}/parsec_amd/lib", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, PARSEC_MCA_device_hip_enabled="0")
    r = subprocess.run([str(exe), "200", "120", "32", "40"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
