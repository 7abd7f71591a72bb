"""The inverse with the Cholesky factor (DTRTRI, DLAUUM, DPOTRI, DPOINV) with the
CPU bodies: one rank against numpy, several ranks on different process grids,
argument checks and the C API program.

The matrix is S = (R + R^T) / 2 + N I with R uniform in [0, 1) (seeded), its
factor L = chol(S). Strictly upper tiles and the upper triangles of the diagonal
tiles hold NaN wherever the operation works on a triangle: they must come back
bit-identical. Tolerances: an inverse may have at most 4 times the residual of
numpy's own (np.linalg.inv of the triangle / of S); DLAUUM is a product, so its
bound is the derived one, ||result - exact||_F <= N eps || |L^T| |L| ||_F."""
import os
import subprocess

import numpy as np
import pytest

from test_distributed_cpu import run_ranks

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "mp", "dist_dpotri.py")
EPS = np.finfo(np.float64).eps

# (N, nb): whole tiles, and a ragged last tile
SHAPES = [(384, 64), (300, 64)]


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


def _fill(M, S, nb):
    for m in range(M.mt):
        for n in range(M.nt):
            blk = S[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb]
            t = M.tile(m, n)
            t[:, :] = 0.0
            t[:blk.shape[0], :blk.shape[1]] = blk


def _gather(M, N, nb):
    out = np.zeros((N, N))
    for m in range(M.mt):
        for n in range(M.nt):
            r, c = min(nb, N - m * nb), min(nb, N - n * nb)
            out[m * nb:m * nb + r, n * nb:n * nb + c] = M.tile(m, n)[:r, :c]
    return out


_problems = {}


def _problem(N, seed=5):
    """(S, L, L with NaN above the diagonal), computed once per order."""
    if N not in _problems:
        R = np.random.default_rng(seed).random((N, N))
        S = (R + R.T) / 2 + N * np.eye(N)
        L = np.linalg.cholesky(S)
        Ln = L.copy()
        Ln[np.triu_indices(N, 1)] = np.nan
        _problems[N] = (S, L, Ln)
    return _problems[N]


def _run(ctx, tp):
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()


def _upper_untouched(G):
    iu = np.triu_indices(G.shape[0], 1)
    return np.isnan(G[iu]).all()


def _tri_residual(X, L):
    return np.linalg.norm(X @ L - np.eye(L.shape[0])) / (np.linalg.norm(X) * np.linalg.norm(L))


def _inv_residual(S, X):
    return np.linalg.norm(S @ X - np.eye(S.shape[0])) / (np.linalg.norm(S) * np.linalg.norm(X))


def _sym(G):
    T = np.tril(G)
    return T + np.tril(T, -1).T


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dtrtri_cpu(pa, ctx, N, nb):
    S, L, Ln = _problem(N)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, Ln, nb)
    tp, info = pa.dtrtri_new(pa.MATRIX_LOWER, pa.MATRIX_NONUNIT, A)
    _run(ctx, tp)
    assert pa.read_int(info) == 0
    G = _gather(A, N, nb)
    assert _upper_untouched(G)
    X = np.tril(G)
    assert np.isfinite(X).all()
    res, ref = _tri_residual(X, L), _tri_residual(np.linalg.inv(L), L)
    print(f"dtrtri N={N} nb={nb}: residual {res:.3e}, numpy {ref:.3e}, ratio {res / ref:.2f}")
    assert res <= 4 * ref


def test_dtrtri_zero_diagonal_cpu(pa, ctx):
    """A diagonal entry that is exactly zero is reported by its 1-based global index."""
    N, nb = 192, 64
    _, L, _ = _problem(N)
    L0 = L.copy()
    L0[70, 70] = 0.0
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, L0, nb)
    with np.errstate(all="ignore"):
        tp, info = pa.dtrtri_new(pa.MATRIX_LOWER, pa.MATRIX_NONUNIT, A)
        _run(ctx, tp)
    assert pa.read_int(info) == 71


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dlauum_cpu(pa, ctx, N, nb):
    S, L, Ln = _problem(N)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, Ln, nb)
    tp = pa.dlauum_new(pa.MATRIX_LOWER, A)
    assert tp is not None
    _run(ctx, tp)
    G = _gather(A, N, nb)
    assert _upper_untouched(G)
    err = np.linalg.norm(np.tril(G) - np.tril(L.T @ L))
    bound = N * EPS * np.linalg.norm(np.abs(L.T) @ np.abs(L))
    print(f"dlauum N={N} nb={nb}: error {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dpotri_cpu(pa, ctx, N, nb):
    S, L, Ln = _problem(N)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, Ln, nb)
    tp = pa.dpotri_new(pa.MATRIX_LOWER, A)
    assert tp is not None
    _run(ctx, tp)
    pa.taskpool_free(tp)
    G = _gather(A, N, nb)
    assert _upper_untouched(G)
    res, ref = _inv_residual(S, _sym(G)), _inv_residual(S, np.linalg.inv(S))
    print(f"dpotri N={N} nb={nb}: residual {res:.3e}, numpy {ref:.3e}, ratio {res / ref:.2f}")
    assert res <= 4 * ref


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dpoinv_cpu(pa, ctx, N, nb):
    S, _, _ = _problem(N)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, S, nb)
    tp, info = pa.dpoinv_new(pa.MATRIX_LOWER, A)
    _run(ctx, tp)
    assert pa.read_int(info) == 0
    pa.taskpool_free(tp)
    G = _gather(A, N, nb)
    assert np.array_equal(np.triu(G, 1), np.triu(S, 1))  # the upper half is the caller's
    res, ref = _inv_residual(S, _sym(G)), _inv_residual(S, np.linalg.inv(S))
    print(f"dpoinv N={N} nb={nb}: residual {res:.3e}, numpy {ref:.3e}, ratio {res / ref:.2f}")
    assert res <= 4 * ref


def test_dpoinv_not_positive_definite_cpu(pa, ctx):
    """info is what the factorization alone reports, the run terminates, and A
    is bit-identical to what the factorization alone leaves."""
    N, nb = 256, 64
    S, _, _ = _problem(N)
    Sbad = S.copy()
    Sbad[70, 70] = -1.0
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, Sbad, nb)
    tp, info = pa.dpotrf_jdf_new(A)
    _run(ctx, tp)
    want_info, want = pa.read_int(info), _gather(A, N, nb)
    assert want_info != 0
    _fill(A, Sbad, nb)
    tp, info = pa.dpoinv_new(pa.MATRIX_LOWER, A)
    _run(ctx, tp)
    assert pa.read_int(info) == want_info
    pa.taskpool_free(tp)
    assert np.array_equal(_gather(A, N, nb), want, equal_nan=True)


def test_unsupported_requests_return_none(pa, ctx):
    N, nb = 128, 64
    _, L, _ = _problem(N)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    _fill(A, L, nb)
    Arect = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N + nb, N)
    Atile = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, 32, N, N)
    # upper, unit diagonal
    assert pa.dtrtri_new(pa.MATRIX_UPPER, pa.MATRIX_NONUNIT, A) is None
    assert pa.dtrtri_new(pa.MATRIX_LOWER, pa.MATRIX_UNIT, A) is None
    assert pa.dlauum_new(pa.MATRIX_UPPER, A) is None
    assert pa.dpotri_new(pa.MATRIX_UPPER, A) is None
    assert pa.dpoinv_new(pa.MATRIX_UPPER, A) is None
    # non-square A, non-square tiles (mb != nb)
    for bad in (Arect, Atile):
        assert pa.dtrtri_new(pa.MATRIX_LOWER, pa.MATRIX_NONUNIT, bad) is None
        assert pa.dlauum_new(pa.MATRIX_LOWER, bad) is None
        assert pa.dpotri_new(pa.MATRIX_LOWER, bad) is None
        assert pa.dpoinv_new(pa.MATRIX_LOWER, bad) is None
    assert np.array_equal(_gather(A, N, nb), L)  # A untouched by the refusals


@pytest.mark.parametrize("nranks,P,Q", [(1, 1, 1), (2, 2, 1), (4, 2, 2), (3, 1, 3)])
def test_dpotri_multirank(pa, nranks, P, Q):
    """dpotri_new on a P x Q grid: every rank checks its own tiles against the
    dense inverse (the worker also checks that dpoinv_new is refused on more
    than one rank)."""
    outs = run_ranks(nranks, 300, 64, P, Q, worker=WORKER)
    for rc, out in outs:
        assert rc == 0, out


def test_dpotri_capi(pa, tmp_path):
    """C program on the public header: invert the triangle, form L^T L, invert
    from the factor and from the matrix, check the residuals."""
    exe = tmp_path / "dpotri_capi"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{ROOT}/include", os.path.join(HERE, "capi", "dpotri_capi.c"), "-o", str(exe),
           f"-L{ROOT}/parsec_amd/lib", "-lparsec_amd", f"-Wl,-rpath,{ROOT}/parsec_amd/lib", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, PARSEC_MCA_device_hip_enabled="0")
    r = subprocess.run([str(exe), "300", "64"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
