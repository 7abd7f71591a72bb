"""Tile LU with incremental pivoting on the GPU: the pivoted tile / stacked-pair
factorization kernels, the grouped row interchange kernel, and the
DGETRF_INCPIV / DGETRS_INCPIV / DGESV_INCPIV taskpools.

The yardstick is the torch model of tests/lu_incpiv_model.py (never the code
under test) and torch.linalg.lu_factor_ex on the same tile or pair. Tolerances
(see that module): a factor's backward error ||P S - L U||_F / ||S||_F is held
to 4 times torch's on the same S, a solve's residual to 4 times the model's, and
the model's is itself within 8 times torch.linalg.solve's."""
import numpy as np
import pytest

import lu_incpiv_model as lu

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SENT = -7.25


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _tile(dev, M, ld, fill=SENT):
    """Column-major device buffer (cols x ld) holding M (rows x cols), the rest `fill`."""
    rows, cols = M.shape
    buf = torch.full((cols, ld), fill, dtype=torch.float64, device=dev)
    buf[:, :rows] = M.t().to(dev)
    return buf


def _check_pair(S, top, bot, L, n, h):
    """Backward error, |l| <= 1, pivots in range; returns the pivots."""
    piv = L[:n, n - 1].copy()
    j = np.arange(n)
    assert (piv == np.round(piv)).all() and (piv >= j + 1).all() and (piv <= n + h).all(), piv
    Lstrict = np.tril(L[:n, :n], -1)
    assert np.abs(Lstrict).max(initial=0.0) <= 1.0
    if bot is not None:
        assert np.abs(bot).max(initial=0.0) <= 1.0
    ours = lu.pair_backward_error(S, top, bot, Lstrict, piv.astype(np.int64))
    ref = lu.torch_backward_error(S)
    print(f"n={n} h={h}: backward error ours {ours:.3e}, torch {ref:.3e}, ratio {ours / ref if ref else 0:.2f}")
    assert ours <= 4 * ref
    return piv


# ------------------------------------------------------------ tile GETRF kernel
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [1, 17, 64, 65, 130, 256, 300])
def test_kernel_dgetrf_piv(pa, dev, n, pad):
    lda = n + pad
    S = lu.normal(n, n, 100 + n)
    A = _tile(dev, S, lda)
    L = torch.full((n, lda), float("nan"), dtype=torch.float64, device=dev)  # its contents on entry do not matter
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    assert pa.kernel_dgetrf_piv(A.data_ptr(), n, lda, L.data_ptr(), lda, info.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert info.item() == 0
    F = A[:, :n].t().cpu().numpy()
    Lh = L.t().cpu().numpy()  # lda x n
    assert np.isfinite(F).all()
    # L holds a copy of the strictly lower part, the pivots in its last column, and nothing else new
    assert np.array_equal(np.tril(Lh[:n, :n], -1), np.tril(F, -1))
    untouched = np.ones_like(Lh, dtype=bool)
    untouched[:n, :n] = np.triu(np.ones((n, n), dtype=bool))
    untouched[:n, n - 1] = False
    assert np.isnan(Lh[untouched]).all()
    assert np.abs(np.tril(F, -1)).max(initial=0.0) <= 1.0
    _check_pair(S, F, None, Lh, n, 0)
    if pad:
        assert (A[:, n:] == SENT).all()  # rows n .. lda-1 untouched


@pytest.mark.parametrize("c", [0, 70, 129])
def test_kernel_dgetrf_piv_zero_column(pa, dev, c):
    n = 130
    S = lu.normal(n, n, 7)
    S[:, c] = 0.0
    A = _tile(dev, S, n)
    L = torch.zeros((n, n), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    assert pa.kernel_dgetrf_piv(A.data_ptr(), n, n, L.data_ptr(), n, info.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert info.item() == c + 1
    F = A.t().cpu().numpy()
    assert np.isfinite(F).all() and F[c, c] == 0.0
    _check_pair(S, F, None, L.t().cpu().numpy(), n, 0)
    # a word that already holds a smaller index is left alone, a larger one is lowered
    for start, want in ((1, 1), (200, c + 1)):
        A = _tile(dev, S, n)
        info.fill_(start)
        assert pa.kernel_dgetrf_piv(A.data_ptr(), n, n, L.data_ptr(), n, info.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert info.item() == min(start, want)


# ------------------------------------------------------------ stacked pair (TSTRF)
def _pair(kind, n, h, seed):
    U = torch.triu(lu.normal(n, n, seed))
    A2 = lu.normal(h, n, seed + 1)
    if kind == "top":  # no interchange at all
        U = torch.triu(U, 1) + torch.diag(torch.full((n,), 1e3, dtype=torch.float64))
    elif kind == "bottom":  # every pivot comes from the bottom tile
        U = torch.triu(U, 1) + torch.diag(torch.full((n,), 1e-3, dtype=torch.float64))
    return U, A2


@pytest.mark.parametrize("kind", ["random", "top", "bottom"])
@pytest.mark.parametrize("n,h", [(64, 64), (64, 17), (65, 65), (130, 130), (256, 100), (256, 256), (300, 300)])
def test_kernel_dtstrf(pa, dev, n, h, kind):
    U0, A20 = _pair(kind, n, h, 200 + n + h)
    ldu, lda2, ldl = n + 3, h + 2, n + 1
    low = torch.tril(torch.full((n, n), 3.5, dtype=torch.float64), -1)  # what a GETRF left below the diagonal
    U = _tile(dev, U0 + low, ldu)
    A2 = _tile(dev, A20, lda2)
    L = torch.full((n, ldl), float("nan"), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    assert pa.kernel_dtstrf(U.data_ptr(), ldu, A2.data_ptr(), lda2, h, n, L.data_ptr(), ldl, info.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert info.item() == 0
    Uo = U[:, :n].t().cpu().numpy()
    A2o = A2[:, :h].t().cpu().numpy()
    Lh = L.t().cpu().numpy()
    assert np.array_equal(np.tril(Uo, -1), low.numpy())  # the strict lower triangle of the top tile is bit-identical
    assert (U[:, n:] == SENT).all() and (A2[:, h:] == SENT).all()
    assert np.isnan(Lh[n:, :]).all()
    assert np.isfinite(Uo).all() and np.isfinite(A2o).all()
    piv = _check_pair(torch.cat([U0, A20]).numpy(), Uo, A2o, Lh, n, h)
    if kind == "top":
        assert np.array_equal(piv, np.arange(1, n + 1)) and not np.tril(Lh[:n, :n], -1).any()
    if kind == "bottom":
        # with fewer bottom rows than columns the bottom tile cannot supply every pivot
        assert (piv > n).all() if h >= n else (piv > n).sum() >= h


@pytest.mark.parametrize("n,h", [(512, 512), (1024, 1024), (1024, 700)])
def test_kernel_dtstrf_rows_per_thread(pa, dev, n, h):
    """The strip kernel holds 1, 2, 3 or 5 rows per thread; the shapes above reach
    the last two (more than 512 and more than 768 stacked rows per strip), and
    1024 is the largest tile the kernels take."""
    U0, A20 = _pair("random", n, h, 300 + n + h)
    U, A2 = _tile(dev, U0, n), _tile(dev, A20, h)
    L = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    assert pa.kernel_dtstrf(U.data_ptr(), n, A2.data_ptr(), h, h, n, L.data_ptr(), n, info.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert info.item() == 0
    Uo, A2o = U.t().cpu().numpy(), A2.t().cpu().numpy()
    assert np.isfinite(Uo).all() and np.isfinite(A2o).all()
    _check_pair(torch.cat([U0, A20]).numpy(), Uo, A2o, L.t().cpu().numpy(), n, h)


def test_kernel_dgetrf_piv_largest_tile(pa, dev):
    n = 1024
    S = lu.normal(n, n, 77)
    A = _tile(dev, S, n)
    L = torch.full((n, n), float("nan"), dtype=torch.float64, device=dev)
    assert pa.kernel_dgetrf_piv(A.data_ptr(), n, n, L.data_ptr(), n, 0, _stream()) == 0
    torch.cuda.synchronize()
    F = A.t().cpu().numpy()
    assert np.isfinite(F).all() and np.abs(np.tril(F, -1)).max() <= 1.0
    _check_pair(S, F, None, L.t().cpu().numpy(), n, 0)


@pytest.mark.parametrize("c", [0, 70, 129])
def test_kernel_dtstrf_zero_column(pa, dev, c):
    n, h = 130, 100
    U0, A20 = _pair("random", n, h, 9)
    U0[:, c] = 0.0
    A20[:, c] = 0.0
    U, A2 = _tile(dev, U0, n), _tile(dev, A20, h)
    L = torch.zeros((n, n), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    assert pa.kernel_dtstrf(U.data_ptr(), n, A2.data_ptr(), h, h, n, L.data_ptr(), n, info.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert info.item() == c + 1
    Uo, A2o = U.t().cpu().numpy(), A2.t().cpu().numpy()
    assert np.isfinite(Uo).all() and np.isfinite(A2o).all() and Uo[c, c] == 0.0
    _check_pair(torch.cat([U0, A20]).numpy(), np.triu(Uo), A2o, L.t().cpu().numpy(), n, h)


# ------------------------------------------------------------ row interchanges
def _laswp_ref(top, bot, piv):
    top, bot = top.copy(), None if bot is None else bot.copy()
    mt, h = top.shape[0], 0 if bot is None else bot.shape[0]
    for j, v in enumerate(piv):
        if j >= mt or not (1 <= v <= mt + h):
            continue
        r = int(v) - 1
        if r == j:
            continue
        o = top if r < mt else bot
        ro = r if r < mt else r - mt
        tmp = top[j].copy()
        top[j] = o[ro]
        o[ro] = tmp
    return top, bot


@pytest.mark.parametrize("case", ["repeated", "top_only", "out_of_range", "no_bottom"])
def test_kernel_dlaswp_pair(pa, dev, case):
    mt, h, ncols = 70, 50, 150  # three column strips of 64, the last one ragged
    rng = np.random.default_rng(3)
    piv = rng.integers(1, mt + h + 1, size=mt).astype(np.float64)
    if case == "repeated":
        piv[:3] = 3.0  # (3, 3, 3) is no gather by an index map
        piv[10:20] = float(mt + 5)
    elif case == "top_only":
        piv = rng.integers(1, mt + 1, size=mt).astype(np.float64)
    elif case == "out_of_range":
        piv[::4] = [0.0, -3.0, mt + h + 1.0, 1e300, float("nan"), float("inf")] * 3
    elif case == "no_bottom":
        h = 0
        piv[::2] = mt + 7.0  # beyond the single tile: ignored
        piv[1::2] = rng.integers(1, mt + 1, size=mt // 2)
    top0 = rng.standard_normal((mt, ncols))
    bot0 = rng.standard_normal((h, ncols)) if h else None
    ldt, ldb = mt + 3, h + 2
    top = _tile(dev, torch.from_numpy(top0), ldt)
    bot = _tile(dev, torch.from_numpy(bot0), ldb) if h else None
    pd = torch.from_numpy(piv).to(dev)
    assert pa.kernel_dlaswp_pair(top.data_ptr(), ldt, mt, bot.data_ptr() if h else 0, ldb, h, ncols, pd.data_ptr(), mt, _stream()) == 0
    torch.cuda.synchronize()
    rt, rb = _laswp_ref(top0, bot0, piv)
    assert np.array_equal(top[:, :mt].t().cpu().numpy(), rt)
    assert (top[:, mt:] == SENT).all()
    if h:
        assert np.array_equal(bot[:, :h].t().cpu().numpy(), rb)
        assert (bot[:, h:] == SENT).all()


# ------------------------------------------------------------------ taskpools
def _gpu_matrix(pa, gpu, M, N, mb, nb, fill=0.0):
    """An M x N collection of mb x nb tiles resident in HBM: (collection, store);
    tile (m, n) is store[n, m], column-major, edge tiles zero padded."""
    MT, NT = -(-M // mb), -(-N // nb)
    store = torch.full((NT, MT, nb, mb), fill, dtype=torch.float64, device="cuda")
    return pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, mb, nb, M, N, device=gpu, ptr=store.data_ptr()), store


def _fill_store(store, dense, mb, nb):
    NT, MT = store.shape[0], store.shape[1]
    M, N = dense.shape
    pad = torch.zeros((MT * mb, NT * nb), dtype=dense.dtype, device=store.device)
    pad[:M, :N] = dense.to(store.device)
    store.copy_(pad.reshape(MT, mb, NT, nb).permute(2, 0, 3, 1))


def _dense_of(store, M, N, mb, nb):
    NT, MT = store.shape[0], store.shape[1]
    return store.permute(1, 3, 0, 2).reshape(MT * mb, NT * nb)[:M, :N].clone()


def _run(ctx, tp):
    ctx.add_taskpool(tp)
    ctx.start()
    ctx.wait()


def _gpu_tasks(pa):
    gpus = [d for d in pa.devices() if d["type"] == pa.DEV_HIP]
    return gpus[0]["executed_tasks"] if gpus else 0


NRHS, NBR = 200, 128  # B's tile width differs from nb


@pytest.mark.parametrize("N,nb", [(1024, 256), (900, 256), (384, 128)])
def test_dgetrf_dgetrs_incpiv_hbm_resident(pa, dev, N, nb):
    S, B0, res_model, res_torch = lu.problem(N, nb, NRHS)
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        L, sl = _gpu_matrix(pa, gpu, N, N, nb, nb, fill=float("nan"))
        B, sb = _gpu_matrix(pa, gpu, N, NRHS, nb, NBR)
        _fill_store(sa, torch.from_numpy(S), nb, nb)
        _fill_store(sb, torch.from_numpy(B0), nb, NBR)
        torch.cuda.synchronize()
        tp, info = pa.dgetrf_incpiv_new(A, L)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        F = _dense_of(sa, N, N, nb, nb).cpu().numpy()
        assert np.isfinite(F).all()
        assert np.abs(np.tril(F, -1)).max() <= 1.0  # every multiplier stored in A
        tps = pa.dgetrs_incpiv_new(pa.MATRIX_NOTRANS, A, L, B)
        assert tps is not None
        _run(ctx, tps)
        pa.taskpool_free(tps)
        X = _dense_of(sb, N, NRHS, nb, NBR).cpu().numpy()
        lu.check_solution(S, X, B0, res_model, res_torch, f"dgetrf+dgetrs_incpiv N={N} nb={nb}")
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


@pytest.mark.parametrize("N,nb", [(1024, 256), (900, 256), (384, 128)])
def test_dgesv_incpiv(pa, dev, N, nb):
    """Factor and solve in one composed taskpool; at N = 1024 then the same with
    a column of zeros: info names it, the run terminates, B is bit-identical."""
    S, B0, res_model, res_torch = lu.problem(N, nb, NRHS)
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        L, sl = _gpu_matrix(pa, gpu, N, N, nb, nb, fill=float("nan"))
        B, sb = _gpu_matrix(pa, gpu, N, NRHS, nb, NBR)
        _fill_store(sa, torch.from_numpy(S), nb, nb)
        _fill_store(sb, torch.from_numpy(B0), nb, NBR)
        torch.cuda.synchronize()
        tp, info = pa.dgesv_incpiv_new(A, L, B)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        pa.taskpool_free(tp)
        X = _dense_of(sb, N, NRHS, nb, NBR).cpu().numpy()
        lu.check_solution(S, X, B0, res_model, res_torch, f"dgesv_incpiv N={N} nb={nb}")
        assert _gpu_tasks(pa) > 0
        if N != 1024:
            return
        Z = S.copy()
        Z[:, 300] = 0.0
        _fill_store(sa, torch.from_numpy(Z), nb, nb)
        _fill_store(sb, torch.from_numpy(B0), nb, NBR)
        torch.cuda.synchronize()
        before = sb.clone()
        tp, info = pa.dgesv_incpiv_new(A, L, B)
        _run(ctx, tp)
        assert pa.read_int(info) == 301
        pa.taskpool_free(tp)
        torch.cuda.synchronize()
        assert torch.equal(sb, before)
        assert torch.isfinite(sa).all()
    finally:
        ctx.fini()


def test_dgesv_incpiv_host_resident_staged(pa, dev):
    """Tiles on the host: staged into the HBM tile cache and written back; the
    result is read from B.tile(m, n)."""
    N, nb, nrhs, nbr = 512, 128, 256, 64
    S, B0, res_model, res_torch = lu.problem(N, nb, nrhs)
    ctx = pa.init(3)
    try:
        A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
        L = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
        B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, nrhs)
        lu.fill(A, S, nb, nb)
        lu.fill_garbage(L)
        lu.fill(B, B0, nb, nbr)
        tp, info = pa.dgesv_incpiv_new(A, L, B)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        pa.taskpool_free(tp)
        lu.check_factor_format(A, L, N, nb)
        lu.check_solution(S, lu.gather(B, N, nrhs, nb, nbr), B0, res_model, res_torch, "dgesv_incpiv host-resident")
        gpus = [d for d in pa.devices() if d["type"] == pa.DEV_HIP]
        assert gpus[0]["executed_tasks"] > 0 and gpus[0]["bytes_in"] > 0
    finally:
        ctx.fini()
