"""Tile LU with incremental pivoting (DGETRF_INCPIV, DGETRS_INCPIV, DGESV_INCPIV)
with the CPU bodies: one rank against the torch model of tests/lu_incpiv_model.py,
several ranks with A / L and B on different process grids, the storage format,
the zero-pivot rule, argument checks and the C API program.

Matrices are standard normal (seeded), plain and with a zeroed diagonal: they
need pivoting, and dgetrf_nopiv_new stops at index 1 on the second kind.
Tolerances: see lu_incpiv_model.py."""
import os
import subprocess

import numpy as np
import pytest

import lu_incpiv_model as lu
from test_distributed_cpu import run_ranks

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WORKER = os.path.join(HERE, "mp", "dist_dgetrf_incpiv.py")

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


def _run(ctx, tp):
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()


def _matrices(pa, N, nb, NRHS, nbr, S, B0):
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    L = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)
    lu.fill(A, S, nb, nb)
    lu.fill_garbage(L)
    lu.fill(B, B0, nb, nbr)
    return A, L, B


@pytest.mark.parametrize("zero_diag", [False, True])
@pytest.mark.parametrize("N,nb,NRHS,nbr", SHAPES)
def test_dgetrf_dgetrs_incpiv_cpu(pa, ctx, N, nb, NRHS, nbr, zero_diag):
    S, B0, res_model, res_torch = lu.problem(N, nb, NRHS, zero_diag=zero_diag)
    A, L, B = _matrices(pa, N, nb, NRHS, nbr, S, B0)
    if zero_diag:
        # the matrix the unpivoted factorization cannot take
        An = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
        lu.fill(An, S, nb, nb)
        tpn, infon = pa.dgetrf_nopiv_new(An)
        _run(ctx, tpn)
        assert pa.read_int(infon) == 1
    tp, info = pa.dgetrf_incpiv_new(A, L)
    _run(ctx, tp)
    assert pa.read_int(info) == 0
    lu.check_factor_format(A, L, N, nb)
    tps = pa.dgetrs_incpiv_new(pa.MATRIX_NOTRANS, A, L, B)
    assert tps is not None
    _run(ctx, tps)
    pa.taskpool_free(tps)
    lu.check_solution(S, lu.gather(B, N, NRHS, nb, nbr), B0, res_model, res_torch, f"N={N} nb={nb} zero_diag={zero_diag} factor+solve")


@pytest.mark.parametrize("zero_diag", [False, True])
@pytest.mark.parametrize("N,nb,NRHS,nbr", SHAPES)
def test_dgesv_incpiv_cpu(pa, ctx, N, nb, NRHS, nbr, zero_diag):
    S, B0, res_model, res_torch = lu.problem(N, nb, NRHS, zero_diag=zero_diag)
    A, L, B = _matrices(pa, N, nb, NRHS, nbr, S, B0)
    tp, info = pa.dgesv_incpiv_new(A, L, B)
    _run(ctx, tp)
    assert pa.read_int(info) == 0
    pa.taskpool_free(tp)
    lu.check_factor_format(A, L, N, nb)
    lu.check_solution(S, lu.gather(B, N, NRHS, nb, nbr), B0, res_model, res_torch, f"N={N} nb={nb} zero_diag={zero_diag} dgesv")


# c = 70: found by a last-row TSTRF; c = 299: by the last GETRF; c = 0: by the first chain
@pytest.mark.parametrize("c", [70, 299, 0])
def test_zero_column_reports_info_and_leaves_b(pa, ctx, c):
    N, nb, NRHS, nbr = 300, 64, 70, 32
    S, B0, _, _ = lu.problem(N, nb, NRHS)
    S = S.copy()
    S[:, c] = 0.0
    A, L, B = _matrices(pa, N, nb, NRHS, nbr, S, B0)
    tp, info = pa.dgesv_incpiv_new(A, L, B)
    _run(ctx, tp)
    assert pa.read_int(info) == c + 1
    pa.taskpool_free(tp)
    lu.check_factor_format(A, L, N, nb)  # no inf / nan anywhere in A or in what L stores
    assert np.array_equal(lu.gather(B, N, NRHS, nb, nbr), B0)


def test_unsupported_requests_return_none(pa, ctx):
    N, nb, NRHS, nbr = 128, 64, 64, 32
    S, B0, _, _ = lu.problem(N, nb, NRHS)
    A, L, B = _matrices(pa, N, nb, NRHS, nbr, S, B0)
    lu.fill_garbage(L, 7.0)
    L0 = lu.gather(L, N, N, nb, nb)

    def refused(a, l, b):
        assert pa.dgetrs_incpiv_new(pa.MATRIX_NOTRANS, a, l, b) is None
        assert pa.dgesv_incpiv_new(a, l, b) is None

    # non-square A, non-square tiles
    Arect = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N + nb, N)
    Brect = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N + nb, NRHS)
    Atile = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, 32, N, N)
    assert pa.dgetrf_incpiv_new(Arect, Arect) is None
    assert pa.dgetrf_incpiv_new(Atile, Atile) is None
    refused(Arect, Arect, Brect)
    refused(Atile, Atile, B)
    # L with another tile size, another grid
    for bad in (pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, 32, 32, N, N), pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N + nb, N + nb),
                pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, 32, N, N)):
        assert pa.dgetrf_incpiv_new(A, bad) is None
        refused(A, bad, B)
    # B's tile rows must match A's tile size, and its rows A's order
    for bad in (pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, 32, nbr, N, NRHS), Brect):
        refused(A, L, bad)
    # NoTrans only
    assert pa.dgetrs_incpiv_new(pa.MATRIX_TRANS, A, L, B) is None
    assert pa.dgetrs_incpiv_new(7, A, L, B) is None
    # tiles beyond the kernels' limit
    big = 1088
    Abig = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, big, big, big, big)
    Lbig = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, big, big, big, big)
    Bbig = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, big, nbr, big, nbr)
    assert pa.dgetrf_incpiv_new(Abig, Lbig) is None
    refused(Abig, Lbig, Bbig)
    assert np.array_equal(lu.gather(A, N, N, nb, nb), S)
    assert np.array_equal(lu.gather(L, N, N, nb, nb), L0)
    assert np.array_equal(lu.gather(B, N, NRHS, nb, nbr), B0)


@pytest.mark.parametrize("nranks,PA,QA,PB,QB", [
    (2, 2, 1, 1, 2),  # A and L by rows, B by columns: every tile of the factor crosses ranks
    (4, 2, 2, 1, 4),
])
def test_dgetrf_incpiv_multirank(pa, nranks, PA, QA, PB, QB):
    """Factor and solve on several ranks (the worker also checks that
    dgesv_incpiv_new is refused there)."""
    outs = run_ranks(nranks, 300, 64, 100, 32, PA, QA, PB, QB, worker=WORKER)
    for rc, out in outs:
        assert rc == 0, out


def test_dgetrf_incpiv_capi(pa, tmp_path):
    """C program on the public header: factor, solve, factor-and-solve, the zero-column rule."""
    exe = tmp_path / "dgetrf_incpiv_capi"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", f"-I{ROOT}/include", os.path.join(HERE, "capi", "dgetrf_incpiv_capi.c"), "-o", str(exe),
           f"-L{ROOT}/parsec_amd/lib", "-lparsec_amd", f"-Wl,-rpath,{ROOT}/parsec_amd/lib", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, PARSEC_MCA_device_hip_enabled="0")
    r = subprocess.run([str(exe), "300", "64", "96"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
