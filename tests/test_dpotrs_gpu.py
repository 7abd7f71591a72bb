"""Left-side tile solve kernel, the tiled triangular solve taskpools and
DPOTRS / DPOSV on the GPU, against fp64 torch references."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _factor(n, dev, seed):
    """Column-major Cholesky factor of R R^T + n I with NaN above the diagonal
    (the kernel must never use L's strict upper triangle), and the clean L."""
    g = torch.Generator(device=dev).manual_seed(seed)
    R = torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)
    L = torch.linalg.cholesky(R @ R.t() + n * torch.eye(n, dtype=torch.float64, device=dev))
    Lnan = L.clone()
    Lnan[torch.triu(torch.ones(n, n, dtype=torch.bool, device=dev), diagonal=1)] = float("nan")
    return Lnan.t().contiguous().t(), L


def _rhs(n, nrhs, ldb, dev, seed, sentinel=-7.25):
    """Column-major n x nrhs right-hand side inside an ldb x nrhs buffer whose
    padding rows hold a sentinel."""
    g = torch.Generator(device=dev).manual_seed(seed + 1000)
    buf = torch.full((nrhs, ldb), sentinel, dtype=torch.float64, device=dev)
    buf[:, :n] = torch.randn((nrhs, n), dtype=torch.float64, device=dev, generator=g)
    return buf


def _ref(L, B0, alpha, trans):
    return alpha * torch.linalg.solve_triangular(L.t() if trans else L, B0, upper=bool(trans))


# (n, nrhs, ldb, alpha): one block / one strip; n not a multiple of 64 and nrhs
# not a multiple of 16 (with ldb > n and alpha != 1); many strips; the largest
# LDS footprint
SHAPES = [(64, 16, 64, 1.0), (200, 50, 216, -0.5), (512, 512, 512, 1.0), (1024, 48, 1024, 1.0)]


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("n,nrhs,ldb,alpha", SHAPES)
def test_kernel_dtrsm_left(pa, dev, n, nrhs, ldb, alpha, trans):
    Lc, L = _factor(n, dev, n + nrhs)
    buf = _rhs(n, nrhs, ldb, dev, n)
    B0 = buf[:, :n].t().clone()
    ref = _ref(L, B0, alpha, trans)
    rc = pa.kernel_dtrsm_left(Lc.data_ptr(), buf.data_ptr(), n, nrhs, n, ldb, alpha, trans, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    err = (buf[:, :n].t() - ref).abs().max().item()
    print(f"n={n} nrhs={nrhs} trans={trans} alpha={alpha}: max abs err {err:.3e}")
    assert err < 1e-10
    if ldb > n:
        assert (buf[:, n:] == -7.25).all()  # padding rows untouched


def test_kernel_dtrsm_left_grouped(pa, dev):
    """One grouped launch of 5 descriptors of mixed shapes and transposes; two of
    them share an L (its diagonal-block inverses are computed once)."""
    cases = [(64, 16, 0, 1.0), (200, 50, 1, 1.0), (320, 33, 0, 2.0), (1024, 48, 1, 1.0), (130, 100, 1, -1.0)]
    Ls, bufs, refs, descs = [], [], [], []
    for i, (n, nrhs, trans, alpha) in enumerate(cases):
        Lc, L = _factor(n, dev, 50 + i)
        buf = _rhs(n, nrhs, n, dev, 50 + i)
        refs.append(_ref(L, buf.t().clone(), alpha, trans))
        Ls.append(Lc)
        bufs.append(buf)
        descs.append((Lc.data_ptr(), buf.data_ptr(), n, nrhs, n, n, alpha, trans))
    # a sixth descriptor on the first L, other direction
    buf6 = _rhs(64, 20, 64, dev, 99)
    refs.append(_ref(torch.tril(torch.nan_to_num(Ls[0])), buf6.t().clone(), 1.0, 1))
    bufs.append(buf6)
    descs.append((Ls[0].data_ptr(), buf6.data_ptr(), 64, 20, 64, 64, 1.0, 1))
    assert pa.kernel_dtrsm_left_batch(descs, _stream()) == 0
    torch.cuda.synchronize()
    for buf, ref in zip(bufs, refs):
        assert (buf.t() - ref).abs().max().item() < 1e-10


# ------------------------------------------------------------------ taskpools
def _gpu_matrix(pa, gpu, M, N, mb, nb):
    """An M x N collection of mb x nb tiles resident in HBM: (collection, store);
    tile (m, n) is store[n, m], column-major, edge tiles zero padded."""
    MT, NT = -(-M // mb), -(-N // nb)
    store = torch.zeros((NT, MT, nb, mb), dtype=torch.float64, device="cuda")
    return pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, mb, nb, M, N, device=gpu, ptr=store.data_ptr()), store


def _fill_store(store, dense, mb, nb):
    NT, MT = store.shape[0], store.shape[1]
    M, N = dense.shape
    pad = torch.zeros((MT * mb, NT * nb), dtype=dense.dtype, device=dense.device)
    pad[:M, :N] = dense
    store.copy_(pad.reshape(MT, mb, NT, nb).permute(2, 0, 3, 1))


def _dense_of(store, M, N, mb, nb):
    NT, MT = store.shape[0], store.shape[1]
    return store.permute(1, 3, 0, 2).reshape(MT * mb, NT * nb)[:M, :N].clone()


def _spd(N, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    R = torch.rand((N, N), dtype=torch.float64, device=dev, generator=g)
    return (R + R.t()) / 2 + N * torch.eye(N, dtype=torch.float64, device=dev)


def _run(ctx, tp):
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()


def _gpu_tasks(pa):
    gpus = [d for d in pa.devices() if d["type"] == pa.DEV_HIP]
    return gpus[0]["executed_tasks"] if gpus else 0


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("N,nb,NRHS,nbr", [(1024, 256, 512, 256), (900, 256, 200, 128)])
def test_dtrsm_hbm_resident(pa, dev, N, nb, NRHS, nbr, trans):
    """LLN and LLT sweeps on HBM-resident tiles against solve_triangular; the
    second shape has edge tiles in both dimensions. L's strict upper triangle
    (inside the diagonal tiles) holds NaN."""
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        B, sb = _gpu_matrix(pa, gpu, N, NRHS, nb, nbr)
        L = torch.linalg.cholesky(_spd(N, dev, 1))
        Ln = L.clone()
        Ln[torch.triu(torch.ones(N, N, dtype=torch.bool, device=dev), diagonal=1)] = float("nan")
        g = torch.Generator(device=dev).manual_seed(2)
        B0 = torch.randn((N, NRHS), dtype=torch.float64, device=dev, generator=g)
        _fill_store(sa, Ln, nb, nb)
        _fill_store(sb, B0, nb, nbr)
        torch.cuda.synchronize()
        alpha = 0.75
        tp = pa.dtrsm_new(pa.MATRIX_LEFT, pa.MATRIX_LOWER, pa.MATRIX_TRANS if trans else pa.MATRIX_NOTRANS, pa.MATRIX_NONUNIT, alpha, A, B)
        assert tp is not None
        _run(ctx, tp)
        ref = alpha * torch.linalg.solve_triangular(L.t() if trans else L, B0, upper=bool(trans))
        X = _dense_of(sb, N, NRHS, nb, nbr)
        err = (X - ref).abs().max().item()
        print(f"dtrsm N={N} nb={nb} NRHS={NRHS} nbr={nbr} trans={trans}: max abs err {err:.3e}")
        assert err < 1e-10
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


def _check_solution(S, X, B0):
    bwd = (torch.linalg.norm(S @ X - B0) / (torch.linalg.norm(S) * torch.linalg.norm(X) + torch.linalg.norm(B0))).item()
    Xref = torch.cholesky_solve(B0, torch.linalg.cholesky(S))
    fwd = (torch.linalg.norm(X - Xref) / torch.linalg.norm(Xref)).item()
    print(f"backward error {bwd:.3e}, forward error {fwd:.3e}")
    assert bwd < 1e-14
    assert fwd < 1e-11


def test_dpotrs_after_dpotrf(pa, dev):
    N, nb, NRHS = 1024, 256, 256
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        B, sb = _gpu_matrix(pa, gpu, N, NRHS, nb, nb)
        S = _spd(N, dev)
        g = torch.Generator(device=dev).manual_seed(3)
        B0 = torch.randn((N, NRHS), dtype=torch.float64, device=dev, generator=g)
        _fill_store(sa, S, nb, nb)
        _fill_store(sb, B0, nb, nb)
        torch.cuda.synchronize()
        tp, info = pa.dpotrf_jdf_new(A)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        tps = pa.dpotrs_new(pa.MATRIX_LOWER, A, B)
        assert tps is not None
        _run(ctx, tps)
        pa.taskpool_free(tps)
        _check_solution(S, _dense_of(sb, N, NRHS, nb, nb), B0)
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


def test_dposv(pa, dev):
    """Factor and solve in one composed taskpool; then the same with an
    indefinite matrix: info != 0, the run terminates, B is bit-identical."""
    N, nb, NRHS = 1024, 256, 256
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        B, sb = _gpu_matrix(pa, gpu, N, NRHS, nb, nb)
        S = _spd(N, dev)
        g = torch.Generator(device=dev).manual_seed(3)
        B0 = torch.randn((N, NRHS), dtype=torch.float64, device=dev, generator=g)
        _fill_store(sa, S, nb, nb)
        _fill_store(sb, B0, nb, nb)
        torch.cuda.synchronize()
        tp, info = pa.dposv_new(pa.MATRIX_LOWER, A, B)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        pa.taskpool_free(tp)
        _check_solution(S, _dense_of(sb, N, NRHS, nb, nb), B0)
        assert _gpu_tasks(pa) > 0
        # indefinite
        Sbad = S.clone()
        Sbad[300, 300] = -1.0
        _fill_store(sa, Sbad, nb, nb)
        _fill_store(sb, B0, nb, nb)
        torch.cuda.synchronize()
        before = sb.clone()
        tp, info = pa.dposv_new(pa.MATRIX_LOWER, A, B)
        _run(ctx, tp)
        assert pa.read_int(info) != 0
        pa.taskpool_free(tp)
        torch.cuda.synchronize()
        assert torch.equal(sb, before)
    finally:
        ctx.fini()


def test_dpotrs_host_resident_staged(pa, dev):
    """Tiles on the host: staged into the HBM tile cache and written back; the
    result is read from B.tile(m, n)."""
    import numpy as np

    N, nb, NRHS, nbr = 512, 128, 256, 128
    ctx = pa.init(3)
    try:
        A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
        B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)
        S = _spd(N, "cpu", 4).numpy()
        L = np.linalg.cholesky(S)
        B0 = np.random.default_rng(4).standard_normal((N, NRHS))
        for m in range(A.mt):
            for n in range(m + 1):
                A.tile(m, n)[:, :] = L[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb]
        for m in range(B.mt):
            for n in range(B.nt):
                B.tile(m, n)[:, :] = B0[m * nb:(m + 1) * nb, n * nbr:(n + 1) * nbr]
        tp = pa.dpotrs_new(pa.MATRIX_LOWER, A, B)
        _run(ctx, tp)
        pa.taskpool_free(tp)
        X = np.zeros((N, NRHS))
        for m in range(B.mt):
            for n in range(B.nt):
                X[m * nb:(m + 1) * nb, n * nbr:(n + 1) * nbr] = B.tile(m, n)
        Xref = np.linalg.solve(S, B0)
        assert np.linalg.norm(S @ X - B0) / (np.linalg.norm(S) * np.linalg.norm(X) + np.linalg.norm(B0)) < 1e-14
        assert np.linalg.norm(X - Xref) / np.linalg.norm(Xref) < 1e-11
        gpus = [d for d in pa.devices() if d["type"] == pa.DEV_HIP]
        assert gpus[0]["executed_tasks"] > 0 and gpus[0]["bytes_in"] > 0
    finally:
        ctx.fini()
