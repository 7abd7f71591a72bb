"""The upper left-side tile solve, the clean-V extraction and the op = N block
reflector apply on the GPU against fp64 references (absolute tolerance 1e-10 as
in the other kernel tests), and DORMQR / DGEQRS / DGELS on HBM-resident tiles:
Q checked from the stored factor at the 1e-12 of test_dgeqrf.py's GPU cases,
solutions at the 1e-14 backward / 1e-11 forward of the DPOTRS tests."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_dgels_cpu import check_q, check_solution  # noqa: E402
from test_dpotrs_gpu import _dense_of, _factor, _fill_store, _gpu_matrix, _gpu_tasks, _rhs, _run  # noqa: E402
from test_kernels_gpu import _cm, _house_qr_ref, _np  # noqa: E402


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _upper_factor(n, dev, seed):
    """Column-major U = L^T (L the Cholesky factor of test_dpotrs_gpu._factor) with
    NaN below the diagonal, where a QR diagonal tile holds V, and the clean U."""
    _, L = _factor(n, dev, seed)
    U = L.t().contiguous()
    Unan = U.clone()
    Unan[torch.tril(torch.ones(n, n, dtype=torch.bool, device=dev), diagonal=-1)] = float("nan")
    return Unan.t().contiguous().t(), U


def _ref_upper(U, B0, alpha, trans):
    return alpha * torch.linalg.solve_triangular(U.t() if trans else U, B0, upper=not trans)


# (n, nrhs, ldb, alpha): one block / one strip; ragged in both dimensions with
# padding rows; many strips; the largest LDS footprint
SHAPES = [(64, 16, 64, 1.0), (200, 50, 216, -0.5), (512, 512, 512, 1.0), (1024, 48, 1024, 1.0)]


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs,ldb,alpha", SHAPES)
def test_kernel_dtrsm_left_upper(pa, dev, n, nrhs, ldb, alpha, trans):
    Uc, U = _upper_factor(n, dev, n + nrhs)
    buf = _rhs(n, nrhs, ldb, dev, n)
    B0 = buf[:, :n].t().clone()
    ref = _ref_upper(U, B0, alpha, trans)
    rc = pa.kernel_dtrsm_left(Uc.data_ptr(), buf.data_ptr(), n, nrhs, n, ldb, alpha, trans, _stream(), upper=1)
    assert rc == 0
    torch.cuda.synchronize()
    err = (buf[:, :n].t() - ref).abs().max().item()
    print(f"upper n={n} nrhs={nrhs} trans={trans} alpha={alpha}: max abs err {err:.3e}")
    assert err < 1e-10
    if ldb > n:
        assert (buf[:, n:] == -7.25).all()  # padding rows untouched


def test_kernel_dtrsm_left_grouped_mixed_triangles(pa, dev):
    """One grouped launch of mixed shapes, triangles and transposes. The last two
    descriptors solve with the lower and with the upper triangle of ONE pointer:
    their diagonal-block inverses must not be shared."""
    cases = [(64, 16, 0, 1.0, 1), (200, 50, 1, 1.0, 0), (320, 33, 0, 2.0, 1), (1024, 48, 1, 1.0, 1), (130, 100, 1, -1.0, 0)]
    keep, bufs, refs, descs = [], [], [], []
    for i, (n, nrhs, trans, alpha, upper) in enumerate(cases):
        buf = _rhs(n, nrhs, n, dev, 70 + i)
        if upper:
            Mc, U = _upper_factor(n, dev, 70 + i)
            refs.append(_ref_upper(U, buf.t().clone(), alpha, trans))
        else:
            Mc, L = _factor(n, dev, 70 + i)
            refs.append(alpha * torch.linalg.solve_triangular(L.t() if trans else L, buf.t().clone(), upper=bool(trans)))
        keep.append(Mc)
        bufs.append(buf)
        descs.append((Mc.data_ptr(), buf.data_ptr(), n, nrhs, n, n, alpha, trans, upper))
    # both triangles of one matrix: lower L1, strictly upper from another factor
    n = 192
    _, L1 = _factor(n, dev, 91)
    _, U2 = _upper_factor(n, dev, 92)
    Mixed = torch.tril(L1) + torch.triu(U2, diagonal=1)
    Up = torch.triu(Mixed)
    Mc = Mixed.t().contiguous().t()
    keep.append(Mc)
    for upper, trans in ((0, 0), (1, 0)):
        buf = _rhs(n, 40, n, dev, 93 + upper)
        B0 = buf.t().clone()
        refs.append(_ref_upper(Up, B0, 1.0, trans) if upper else torch.linalg.solve_triangular(L1, B0, upper=False))
        bufs.append(buf)
        descs.append((Mc.data_ptr(), buf.data_ptr(), n, 40, n, n, 1.0, trans, upper))
    assert pa.kernel_dtrsm_left_batch(descs, _stream()) == 0
    torch.cuda.synchronize()
    for buf, ref in zip(bufs, refs):
        assert (buf.t() - ref).abs().max().item() < 1e-10


@pytest.mark.parametrize("m,n", [(256, 256), (232, 232), (300, 200)])
def test_kernel_qr_extract_v(pa, dev, m, n):
    A = np.random.default_rng(0).standard_normal((m, n))
    k = min(m, n)
    Ad = _cm(A, dev)
    Td = torch.zeros((k, k), dtype=torch.float64, device=dev)
    Vd = torch.full((k, m), float("nan"), dtype=torch.float64, device=dev)
    s = _stream()
    assert pa.kernel_qr_panel(Ad.data_ptr(), m, 0, 0, Td.data_ptr(), k, 0, m, 0, n, s) == 0
    assert pa.kernel_qr_extract_v(Ad.data_ptr(), m, m, n, Vd.data_ptr(), s) == 0
    torch.cuda.synchronize()
    R_ref, V_ref, T_ref = _house_qr_ref(A)
    assert np.allclose(_np(Vd), V_ref, atol=1e-10)
    assert np.allclose(np.triu(_np(Ad))[:k], R_ref, atol=1e-10)  # the tile keeps R


@pytest.mark.parametrize("m2,n", [(100, 64), (512, 200)])
def test_kernel_qr_apply_notrans(pa, dev, m2, n):
    """X := Q X = X - V T V^T X, as UNMQR (V unit lower, m2 x n) and as TSMQR (V = [I; V2])."""
    rng = np.random.default_rng(2)
    s = _stream()
    nc = 96
    # UNMQR
    A = rng.standard_normal((m2, n))
    Ad = _cm(A, dev)
    Td = torch.zeros((n, n), dtype=torch.float64, device=dev)
    Vd = torch.zeros((n, m2), dtype=torch.float64, device=dev)
    assert pa.kernel_qr_panel(Ad.data_ptr(), m2, 0, 0, Td.data_ptr(), n, Vd.data_ptr(), m2, 0, n, s) == 0
    X = rng.standard_normal((m2, nc))
    Xd = _cm(X, dev)
    ws = torch.empty(2 * n * nc, dtype=torch.float64, device=dev)
    assert pa.kernel_qr_apply(Vd.data_ptr(), m2, Td.data_ptr(), n, 0, 0, Xd.data_ptr(), m2, m2, n, nc, ws.data_ptr(), s, 1) == 0
    torch.cuda.synchronize()
    _, V_ref, T_ref = _house_qr_ref(A)
    assert np.allclose(_np(Xd), X - V_ref @ (T_ref @ (V_ref.T @ X)), atol=1e-10)
    # TSMQR
    R = np.triu(rng.standard_normal((n, n)))
    A2 = rng.standard_normal((m2, n))
    Rd, A2d = _cm(R, dev), _cm(A2, dev)
    assert pa.kernel_qr_panel(Rd.data_ptr(), n, A2d.data_ptr(), m2, Td.data_ptr(), n, 0, 0, m2, n, s) == 0
    B1, B2 = rng.standard_normal((n, nc)), rng.standard_normal((m2, nc))
    B1d, B2d = _cm(B1, dev), _cm(B2, dev)
    assert pa.kernel_qr_apply(A2d.data_ptr(), m2, Td.data_ptr(), n, B1d.data_ptr(), n, B2d.data_ptr(), m2, m2, n, nc, ws.data_ptr(), s, 1) == 0
    torch.cuda.synchronize()
    _, V_ref, T_ref = _house_qr_ref(np.vstack([R, A2]))
    X = np.vstack([B1, B2])
    assert np.allclose(np.vstack([_np(B1d), _np(B2d)]), X - V_ref @ (T_ref @ (V_ref.T @ X)), atol=1e-10)


# ------------------------------------------------------------------ taskpools
# (M, N, nb, NRHS, nbr): square; the last two have N not a multiple of nb with M > N
TP_SHAPES = [(1024, 1024, 256, 512, 256), (1280, 768, 256, 200, 128), (1000, 600, 256, 100, 128)]


def _problem(M, N, NRHS, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    S = torch.randn((M, N), dtype=torch.float64, device=dev, generator=g)
    B0 = torch.randn((M, NRHS), dtype=torch.float64, device=dev, generator=g)
    return S, B0


def _apply_q(pa, ctx, gpu, trans, A, T, X, nb, nbr):
    B, sb = _gpu_matrix(pa, gpu, X.shape[0], X.shape[1], nb, nbr)
    _fill_store(sb, X, nb, nbr)
    torch.cuda.synchronize()
    tp = pa.dormqr_new(pa.MATRIX_LEFT, pa.MATRIX_TRANS if trans else pa.MATRIX_NOTRANS, A, T, B)
    assert tp is not None
    _run(ctx, tp)
    pa.taskpool_free(tp)
    return _dense_of(sb, X.shape[0], X.shape[1], nb, nbr)


@pytest.mark.parametrize("source", ["jdf", "ir"])
@pytest.mark.parametrize("M,N,nb,NRHS,nbr", TP_SHAPES)
def test_dormqr_dgeqrs_hbm_resident(pa, dev, M, N, nb, NRHS, nbr, source):
    """Factor on the GPU, then check the stored Q (Q^T A = [R; 0], Q Q^T B = B,
    column norms) and solve with dgeqrs."""
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        S, B0 = _problem(M, N, NRHS, dev, 5)
        A, sa = _gpu_matrix(pa, gpu, M, N, nb, nb)
        T, st = _gpu_matrix(pa, gpu, M, N, nb, nb)
        _fill_store(sa, S, nb, nb)
        torch.cuda.synchronize()
        _run(ctx, pa.dgeqrf_jdf_new(A, T) if source == "jdf" else pa.dgeqrf_new(A, T, 32))
        R = _dense_of(sa, M, N, nb, nb)
        QtS = _apply_q(pa, ctx, gpu, 1, A, T, S, nb, nbr)
        QtB = _apply_q(pa, ctx, gpu, 1, A, T, B0, nb, nbr)
        QQtB = _apply_q(pa, ctx, gpu, 0, A, T, QtB, nb, nbr)
        check_q(S.cpu().numpy(), R.cpu().numpy(), QtS.cpu().numpy(), B0.cpu().numpy(), QtB.cpu().numpy(), QQtB.cpu().numpy(), 1e-12)
        B, sb = _gpu_matrix(pa, gpu, M, NRHS, nb, nbr)
        _fill_store(sb, B0, nb, nbr)
        torch.cuda.synchronize()
        tp = pa.dgeqrs_new(A, T, B)
        assert tp is not None
        _run(ctx, tp)
        pa.taskpool_free(tp)
        Bout = _dense_of(sb, M, NRHS, nb, nbr)
        check_solution(S.cpu().numpy(), B0.cpu().numpy(), Bout.cpu().numpy(), N, 1e-12, forward=M > N)
        # rows >= N, also those sharing the last tile row with X, are what Q^T B left
        assert torch.equal(Bout[N:], QtB[N:])
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


@pytest.mark.parametrize("M,N,nb,NRHS,nbr", TP_SHAPES)
def test_dgels_hbm_resident(pa, dev, M, N, nb, NRHS, nbr):
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        S, B0 = _problem(M, N, NRHS, dev, 6)
        A, sa = _gpu_matrix(pa, gpu, M, N, nb, nb)
        T, st = _gpu_matrix(pa, gpu, M, N, nb, nb)
        B, sb = _gpu_matrix(pa, gpu, M, NRHS, nb, nbr)
        _fill_store(sa, S, nb, nb)
        _fill_store(sb, B0, nb, nbr)
        torch.cuda.synchronize()
        tp = pa.dgels_new(A, T, B)
        assert tp is not None
        _run(ctx, tp)
        pa.taskpool_free(tp)
        Bout = _dense_of(sb, M, NRHS, nb, nbr)
        check_solution(S.cpu().numpy(), B0.cpu().numpy(), Bout.cpu().numpy(), N, 1e-12, forward=M > N)
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


def test_dgels_host_resident_staged(pa, dev):
    """Tiles on the host: staged into the HBM tile cache and written back; the
    result is read from B.tile(m, n)."""
    from test_dgels_cpu import fill, gather

    M, N, nb, NRHS, nbr = 640, 384, 128, 256, 128
    ctx = pa.init(3)
    try:
        rng = np.random.default_rng(8)
        S, B0 = rng.standard_normal((M, N)), rng.standard_normal((M, NRHS))
        A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
        T = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N)
        B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, M, NRHS)
        fill(A, S, nb, nb)
        fill(B, B0, nb, nbr)
        tp = pa.dgels_new(A, T, B)
        assert tp is not None
        _run(ctx, tp)
        pa.taskpool_free(tp)
        check_solution(S, B0, gather(B, M, NRHS, nb, nbr), N, 1e-12, forward=True)
        gpus = [d for d in pa.devices() if d["type"] == pa.DEV_HIP]
        assert gpus[0]["executed_tasks"] > 0 and gpus[0]["bytes_in"] > 0
    finally:
        ctx.fini()
