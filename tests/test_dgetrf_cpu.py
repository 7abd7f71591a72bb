"""LU without pivoting (DGETRF_NOPIV, DGETRS_NOPIV, DGESV_NOPIV) with the CPU
bodies: one rank against numpy, several ranks with A and B on different process
grids, argument checks and the C API program.

The test matrix is R (standard normal, seeded) + diag(column sums of |R| + 1):
column diagonally dominant, so partial pivoting never swaps and an unpivoted LU
is the algorithm LAPACK would run. Tolerance: the backward error of a reference
unpivoted LU computed here with numpy in the textbook order; ours may be at
most 4 times that (other summation order). Solves are held to 4 times the
residual of numpy.linalg.solve."""
import os
import subprocess

import numpy as np
import pytest

from test_distributed_cpu import run_ranks

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "mp", "dist_dgetrf.py")

# (N, nb, NRHS, nbr): whole tiles, and a ragged last tile in both dimensions
SHAPES = [(384, 64, 96, 32), (300, 64, 70, 32)]


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


def _fill(M, S, mb, nb):
    for m in range(M.mt):
        for n in range(M.nt):
            blk = S[m * mb:(m + 1) * mb, n * nb:(n + 1) * nb]
            t = M.tile(m, n)
            t[:, :] = 0.0
            t[:blk.shape[0], :blk.shape[1]] = blk


def _gather(M, rows, cols, mb, nb):
    out = np.zeros((rows, cols))
    for m in range(M.mt):
        for n in range(M.nt):
            r, c = min(mb, rows - m * mb), min(nb, cols - n * nb)
            out[m * mb:m * mb + r, n * nb:n * nb + c] = M.tile(m, n)[:r, :c]
    return out


def _lu_nopiv(S):
    A = S.copy()
    for j in range(A.shape[0] - 1):
        A[j + 1:, j] /= A[j, j]
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j, j + 1:])
    return A


def _lu_backward(F, S):
    L = np.tril(F, -1) + np.eye(F.shape[0])
    return np.linalg.norm(L @ np.triu(F) - S) / np.linalg.norm(S)


_problems = {}


def _problem(N, NRHS, seed=6):
    """(S, its reference factor, the reference's backward error, B0), computed once per shape."""
    if (N, NRHS) not in _problems:
        rng = np.random.default_rng(seed)
        R = rng.standard_normal((N, N))
        S = R + np.diag(np.abs(R).sum(axis=0) + 1.0)
        F = _lu_nopiv(S)
        _problems[(N, NRHS)] = (S, F, _lu_backward(F, S), rng.standard_normal((N, NRHS)))
    return _problems[(N, NRHS)]


def _run(ctx, tp):
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()


def _residual(S, X, B0):
    return np.linalg.norm(S @ X - B0) / (np.linalg.norm(S) * np.linalg.norm(X) + np.linalg.norm(B0))


@pytest.mark.parametrize("N,nb,NRHS,nbr", SHAPES)
def test_dgetrf_nopiv_cpu(pa, ctx, N, nb, NRHS, nbr):
    S, F, ref_bwd, _ = _problem(N, NRHS)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, S, nb, nb)
    tp, info = pa.dgetrf_nopiv_new(A)
    _run(ctx, tp)
    assert pa.read_int(info) == 0
    G = _gather(A, N, N, nb, nb)
    bwd = _lu_backward(G, S)
    print(f"N={N} nb={nb}: backward error {bwd:.3e}, reference {ref_bwd:.3e}, ratio {bwd / ref_bwd:.2f}")
    assert bwd <= 4 * ref_bwd
    # entrywise: both are backward stable factors of the same well-conditioned
    # matrix; |F| <= ~N, so 1e-10 is ~1e3 ulps of the largest entry
    assert np.abs(G - F).max() < 1e-10


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("N,nb,NRHS,nbr", SHAPES)
def test_dgetrs_nopiv_cpu(pa, ctx, N, nb, NRHS, nbr, trans):
    S, F, _, B0 = _problem(N, NRHS)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)
    _fill(A, F, nb, nb)
    _fill(B, B0, nb, nbr)
    tp = pa.dgetrs_nopiv_new(pa.MATRIX_TRANS if trans else pa.MATRIX_NOTRANS, A, B)
    assert tp is not None
    _run(ctx, tp)
    pa.taskpool_free(tp)
    X = _gather(B, N, NRHS, nb, nbr)
    op = S.T if trans else S
    ref = _residual(op, np.linalg.solve(op, B0), B0)
    res = _residual(op, X, B0)
    print(f"N={N} trans={trans}: residual {res:.3e}, numpy {ref:.3e}, ratio {res / ref:.2f}")
    assert res <= 4 * ref


@pytest.mark.parametrize("N,nb,NRHS,nbr", SHAPES)
def test_dgesv_nopiv_cpu(pa, ctx, N, nb, NRHS, nbr):
    S, F, _, B0 = _problem(N, NRHS)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)
    _fill(A, S, nb, nb)
    _fill(B, B0, nb, nbr)
    tp, info = pa.dgesv_nopiv_new(A, B)
    _run(ctx, tp)
    assert pa.read_int(info) == 0
    pa.taskpool_free(tp)
    X = _gather(B, N, NRHS, nb, nbr)
    ref = _residual(S, np.linalg.solve(S, B0), B0)
    res = _residual(S, X, B0)
    print(f"N={N}: residual {res:.3e}, numpy {ref:.3e}, ratio {res / ref:.2f}")
    assert res <= 4 * ref


def _zero_pivot_matrix(N, at, seed=7):
    """A = L U from small integers (exact in fp64) with U[at, at] = 0. L and U
    are bidiagonal with entries +-1, so the inverses of their diagonal blocks
    hold only 0 and +-1 and a blocked factorization stays exact too."""
    rng = np.random.default_rng(seed)
    L = np.eye(N) + np.diag(rng.choice([-1.0, 1.0], N - 1), -1)
    U = np.diag(rng.choice([-1.0, 1.0], N)) + np.diag(rng.choice([-1.0, 1.0], N - 1), 1)
    U[at, at] = 0.0
    return L @ U


def test_dgesv_nopiv_zero_pivot_leaves_b_untouched(pa, ctx):
    """A zero pivot (info = its 1-based global index) must not run the solve on
    inf / nan: the run terminates and B is bit-identical to its input."""
    N, nb, NRHS, nbr = 192, 64, 96, 32
    S = _zero_pivot_matrix(N, 70)
    B0 = np.random.default_rng(8).standard_normal((N, NRHS))
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)
    _fill(A, S, nb, nb)
    _fill(B, B0, nb, nbr)
    tp, info = pa.dgesv_nopiv_new(A, B)
    _run(ctx, tp)
    assert pa.read_int(info) == 71
    pa.taskpool_free(tp)
    assert np.array_equal(_gather(B, N, NRHS, nb, nbr), B0)


def test_unsupported_requests_return_none(pa, ctx):
    N, nb, NRHS, nbr = 128, 64, 64, 32
    S, F, _, B0 = _problem(N, NRHS)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)
    _fill(A, F, nb, nb)
    _fill(B, B0, nb, nbr)
    # non-square A, non-square tiles
    Arect = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N + nb, N)
    Atile = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, 32, N, N)
    Brect = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N + nb, NRHS)
    for bad in (Arect, Atile):
        assert pa.dgetrf_nopiv_new(bad) is None
        assert pa.dgetrs_nopiv_new(pa.MATRIX_NOTRANS, bad, Brect if bad is Arect else B) is None
        assert pa.dgesv_nopiv_new(bad, Brect if bad is Arect else B) is None
    # B's tile rows must match A's tile size, and its rows A's order
    Bbad = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, 32, nbr, N, NRHS)
    for bad in (Bbad, Brect):
        assert pa.dgetrs_nopiv_new(pa.MATRIX_NOTRANS, A, bad) is None
        assert pa.dgesv_nopiv_new(A, bad) is None
    # a bad trans
    assert pa.dgetrs_nopiv_new(7, A, B) is None
    assert pa.dgetrs_nopiv_new(pa.MATRIX_CONJTRANS, A, B) is None
    # the new solve modes are not exposed through dtrsm_new
    assert pa.dtrsm_new(pa.MATRIX_LEFT, pa.MATRIX_LOWER, pa.MATRIX_NOTRANS, pa.MATRIX_UNIT, 1.0, A, B) is None
    assert np.array_equal(_gather(B, N, NRHS, nb, nbr), B0)  # B untouched by the refusals
    assert np.array_equal(_gather(A, N, N, nb, nb), F)


@pytest.mark.parametrize("nranks,PA,QA,PB,QB", [
    (2, 2, 1, 1, 2),  # A by rows, B by columns: every tile of the factor crosses ranks
    (4, 2, 2, 1, 4),
])
def test_dgetrf_multirank(pa, nranks, PA, QA, PB, QB):
    """Factor, solve and transposed solve on several ranks (the worker also checks
    that dgesv_nopiv_new is refused there)."""
    outs = run_ranks(nranks, 300, 64, 100, 32, PA, QA, PB, QB, worker=WORKER)
    for rc, out in outs:
        assert rc == 0, out


def test_dgetrf_capi(pa, tmp_path):
    """C program on the public header: factor, solve both ways, check the residuals."""
    exe = tmp_path / "dgetrf_capi"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{ROOT}/include", os.path.join(HERE, "capi", "dgetrf_capi.c"), "-o", str(exe),
           f"-L{ROOT}/parsec_amd/lib", "-lparsec_amd", f"-Wl,-rpath,{ROOT}/parsec_amd/lib", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, PARSEC_MCA_device_hip_enabled="0")
    r = subprocess.run([str(exe), "300", "64", "96"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
