"""LU without pivoting on the GPU: the tile GETRF kernel, the unit-diagonal and
right-side modes of the left-side tile solve, and the DGETRF_NOPIV /
DGETRS_NOPIV / DGESV_NOPIV taskpools, against fp64 torch references.

Test matrix: R (standard normal, seeded) + diag(column sums of |R| + 1), column
diagonally dominant. Partial pivoting never swaps on it, so torch.linalg.lu_factor
on the CPU runs the same algorithm; every test asserts that torch's pivots are
the identity before it compares.

Tolerances. Factor: the backward error ||L U - A||_F / ||A||_F of torch's CPU
factor of the same matrix; ours may be at most 4 times that (explicit 64 x 64
block inverses and MFMA summation order). Taskpool solves: 4 times the residual
of torch.linalg.solve. Tile solves (kernel_dtrsm_left): the test triangles have
a unit-size diagonal and off-diagonal column sums below 1, so their 64-blocks
have condition numbers of a few units; substitution leaves a normwise residual of
at most n eps, the multiplication by the block inverses adds that condition
number: 4 n eps is asserted. Block inverses: |X - T^-1| <= n eps cond(T) |T^-1|
for substitution, twice that (numpy's own error) is asserted."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _colmajor(M):
    """A fresh column-major copy of M (never a view of it, also for a single column)."""
    return M.t().clone(memory_format=torch.contiguous_format)


def _dominant(n, seed):
    g = torch.Generator().manual_seed(seed)
    R = torch.randn((n, n), dtype=torch.float64, generator=g)
    return R + torch.diag(R.abs().sum(dim=0) + 1.0)


_refs = {}


def _reference(n, seed):
    """(A, torch's CPU L\\U, its backward error), computed once per (n, seed)."""
    if (n, seed) not in _refs:
        A = _dominant(n, seed)
        LU, piv = torch.linalg.lu_factor(A)
        assert torch.equal(piv, torch.arange(1, n + 1, dtype=piv.dtype)), "the reference pivoted"
        _refs[(n, seed)] = (A, LU, _lu_backward(LU, A))
    return _refs[(n, seed)]


def _lu_backward(F, A):
    n = F.shape[0]
    L = torch.tril(F, -1) + torch.eye(n, dtype=F.dtype, device=F.device)
    return (torch.linalg.norm(L @ torch.triu(F) - A) / torch.linalg.norm(A)).item()


def _zero_pivot_matrix(n, at, seed=7):
    """A = L U from small integers (exact in fp64) with U[at, at] = 0. L and U
    are bidiagonal with entries +-1, so the inverses of their diagonal blocks
    hold only 0 and +-1 and the blocked factorization stays exact."""
    rng = np.random.default_rng(seed)
    L = np.eye(n) + np.diag(rng.choice([-1.0, 1.0], n - 1), -1)
    U = np.diag(rng.choice([-1.0, 1.0], n)) + np.diag(rng.choice([-1.0, 1.0], n - 1), 1)
    U[at, at] = 0.0
    return torch.from_numpy(L @ U)


# ------------------------------------------------------------ tile GETRF kernel
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n", [1, 17, 64, 65, 130, 256, 300])
def test_kernel_dgetrf_nopiv(pa, dev, n, pad):
    lda = n + pad
    A, LUref, ref_bwd = _reference(n, 100 + n)
    buf = torch.full((n, lda), -7.25, dtype=torch.float64, device=dev)  # column-major lda x n
    buf[:, :n] = A.t().to(dev)
    nblk = (n + 63) // 64
    invL = torch.full((nblk, 64, 64), float("nan"), dtype=torch.float64, device=dev)
    invU = torch.full((nblk, 64, 64), float("nan"), dtype=torch.float64, device=dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = pa.kernel_dgetrf_nopiv(buf.data_ptr(), n, lda, info.data_ptr(), invL.data_ptr(), invU.data_ptr(), _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert info.item() == 0
    F = buf[:, :n].t().cpu()
    bwd = _lu_backward(F, A)
    diff = (F - LUref).abs().max().item()
    print(f"n={n} lda={lda}: backward error {bwd:.3e}, torch {ref_bwd:.3e}, ratio {bwd / ref_bwd if ref_bwd else 0:.2f}, max |ours - torch| {diff:.3e}")
    assert bwd <= 4 * ref_bwd
    if pad:
        assert (buf[:, n:] == -7.25).all()  # rows n .. lda-1 untouched
    # the diagonal-block inverses: column-major 64 x 64 blocks, identity-padded
    Fn = F.numpy()
    for b in range(nblk):
        c0, w = 64 * b, min(64, n - 64 * b)
        D = Fn[c0:c0 + w, c0:c0 + w]
        TL, TU = np.eye(64), np.eye(64)
        TL[:w, :w] = np.tril(D, -1) + np.eye(w)
        TU[:w, :w] = np.triu(D)
        for name, T, X in (("invL", TL, invL[b].t().cpu().numpy()), ("invU", TU, invU[b].t().cpu().numpy())):
            ref = np.linalg.inv(T)
            rel = np.linalg.norm(X - ref) / np.linalg.norm(ref)
            assert rel <= 2 * 64 * EPS * np.linalg.cond(T), (name, b, rel)
            assert np.array_equal(X[w:, :], np.eye(64)[w:, :]) and np.array_equal(X[:, w:], np.eye(64)[:, w:]), (name, b, "padding")
        assert np.array_equal(np.triu(invL[b].t().cpu().numpy()), np.eye(64))  # unit lower
        assert np.array_equal(np.tril(invU[b].t().cpu().numpy(), -1), np.zeros((64, 64)))


def test_kernel_dgetrf_nopiv_without_inverse_buffers(pa, dev):
    """invL / invU are optional: the launcher then keeps them in its workspace."""
    n = 130
    A, LUref, ref_bwd = _reference(n, 100 + n)
    buf = A.t().contiguous().to(dev)
    assert pa.kernel_dgetrf_nopiv(buf.data_ptr(), n, n) == 0
    torch.cuda.synchronize()
    assert _lu_backward(buf.t().cpu(), A) <= 4 * ref_bwd


def test_kernel_dgetrf_nopiv_zero_pivot(pa, dev):
    n = 130
    A = _zero_pivot_matrix(n, 70)
    buf = A.t().contiguous().to(dev)
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = pa.kernel_dgetrf_nopiv(buf.data_ptr(), n, n, info.data_ptr(), 0, 0, _stream())
    assert rc == 0
    torch.cuda.synchronize()  # the call returns normally; the factor holds inf / nan
    assert info.item() == 71
    # a word that already holds a smaller index is left alone, a larger one is lowered
    for start, want in ((5, 5), (100, 71)):
        buf = A.t().contiguous().to(dev)
        info.fill_(start)
        assert pa.kernel_dgetrf_nopiv(buf.data_ptr(), n, n, info.data_ptr(), 0, 0, _stream()) == 0
        torch.cuda.synchronize()
        assert info.item() == want


# ------------------------------------- unit diagonal / right side tile solves
def _triangle(n, dev, seed, upper, unit):
    """(tile, T): T is the n x n triangle (unit diagonal when `unit`), the tile is
    column-major with NaN in the other triangle and, when `unit`, on the diagonal."""
    g = torch.Generator().manual_seed(seed)
    R = torch.randn((n, n), dtype=torch.float64, generator=g) / n
    T = torch.triu(R, 1) if upper else torch.tril(R, -1)
    d = torch.ones(n, dtype=torch.float64) if unit else 1.0 + torch.rand(n, dtype=torch.float64, generator=g)
    T = T + torch.diag(d)
    tile = T.clone()
    other = torch.tril(torch.ones(n, n, dtype=torch.bool), -1) if upper else torch.triu(torch.ones(n, n, dtype=torch.bool), 1)
    tile[other] = float("nan")
    if unit:
        tile[torch.eye(n, dtype=torch.bool)] = float("nan")
    return tile.t().contiguous().to(dev), T.to(dev)  # row-major of the transpose = column-major


def _residual_left(T, X, B0, alpha, trans):
    op = T.t() if trans else T
    return (torch.linalg.norm(op @ X - alpha * B0) / (torch.linalg.norm(op) * torch.linalg.norm(X) + abs(alpha) * torch.linalg.norm(B0))).item()


@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("upper", [0, 1])
def test_kernel_dtrsm_left_unit(pa, dev, upper, trans):
    for n in (16, 64, 100, 192):
        tile, T = _triangle(n, dev, 10 * n + upper, upper, True)
        for nrhs in (1, 16, 37):
            g = torch.Generator().manual_seed(n + nrhs)
            B0 = torch.randn((n, nrhs), dtype=torch.float64, generator=g).to(dev)
            buf = _colmajor(B0)  # column-major n x nrhs
            alpha = -0.5
            rc = pa.kernel_dtrsm_left(tile.data_ptr(), buf.data_ptr(), n, nrhs, n, n, alpha, trans, _stream(), upper=upper, unit=1)
            assert rc == 0
            torch.cuda.synchronize()
            X = buf.t()
            assert torch.isfinite(X).all()  # neither the diagonal nor the other triangle was used
            res = _residual_left(T, X, B0, alpha, trans)
            assert res <= 4 * n * EPS, (n, nrhs, res)


@pytest.mark.parametrize("unit", [0, 1])
@pytest.mark.parametrize("trans", [0, 1])
@pytest.mark.parametrize("upper", [0, 1])
def test_kernel_dtrsm_left_right_side(pa, dev, upper, trans, unit):
    """X op(T) = alpha B with B rows x n inside an ldb x n buffer (ldb > rows):
    the rows beyond stay untouched."""
    for n in (16, 64, 100, 192):
        tile, T = _triangle(n, dev, 20 * n + upper, upper, bool(unit))
        op = T.t() if trans else T
        for rows in (1, 16, 37, 130):
            ldb = rows + 5
            g = torch.Generator().manual_seed(n + rows)
            B0 = torch.randn((rows, n), dtype=torch.float64, generator=g).to(dev)
            buf = torch.full((n, ldb), -7.25, dtype=torch.float64, device=dev)  # column-major ldb x n
            buf[:, :rows] = B0.t()
            alpha = 2.0
            rc = pa.kernel_dtrsm_left(tile.data_ptr(), buf.data_ptr(), n, rows, n, ldb, alpha, trans, _stream(), upper=upper, unit=unit, right=1)
            assert rc == 0
            torch.cuda.synchronize()
            X = buf[:, :rows].t()
            assert torch.isfinite(X).all()
            res = (torch.linalg.norm(X @ op - alpha * B0) / (torch.linalg.norm(op) * torch.linalg.norm(X) + alpha * torch.linalg.norm(B0))).item()
            assert res <= 4 * n * EPS, (n, rows, res)
            assert (buf[:, rows:] == -7.25).all()


def test_kernel_dtrsm_left_grouped_modes(pa, dev):
    """One grouped launch over ONE tile pointer that holds L\\U: plain lower,
    unit lower, plain upper, unit upper, and right-side descriptors. The sharing
    key of the diagonal-block inverses (pointer, triangle, unit) keeps them apart."""
    n = 130
    g = torch.Generator().manual_seed(77)
    R = torch.randn((n, n), dtype=torch.float64, generator=g) / n
    M = (R + torch.diag(1.0 + torch.rand(n, dtype=torch.float64, generator=g))).to(dev)
    tile = _colmajor(M)
    eye = torch.eye(n, dtype=torch.float64, device=dev)
    tri = {(0, 0): torch.tril(M), (0, 1): torch.tril(M, -1) + eye, (1, 0): torch.triu(M), (1, 1): torch.triu(M, 1) + eye}
    # (upper, unit, right, trans, nrhs)
    modes = [(0, 0, 0, 0, 20), (0, 1, 0, 0, 20), (1, 0, 0, 0, 33), (1, 1, 0, 1, 16), (1, 0, 1, 0, 40), (0, 1, 1, 1, 7), (0, 0, 1, 0, 16), (1, 1, 1, 0, 50)]
    descs, bufs, checks = [], [], []
    for i, (upper, unit, right, trans, nrhs) in enumerate(modes):
        gi = torch.Generator().manual_seed(200 + i)
        if right:
            B0 = torch.randn((nrhs, n), dtype=torch.float64, generator=gi).to(dev)
            buf = _colmajor(B0)  # column-major nrhs x n
            ldb = nrhs
        else:
            B0 = torch.randn((n, nrhs), dtype=torch.float64, generator=gi).to(dev)
            buf = _colmajor(B0)  # column-major n x nrhs
            ldb = n
        bufs.append(buf)
        checks.append((tri[(upper, unit)], B0, right, trans))
        descs.append((tile.data_ptr(), buf.data_ptr(), n, nrhs, n, ldb, 1.0, trans, upper, unit, right))
    assert pa.kernel_dtrsm_left_batch(descs, _stream()) == 0
    torch.cuda.synchronize()
    for buf, (T, B0, right, trans) in zip(bufs, checks):
        op = T.t() if trans else T
        X = buf.t()
        R_ = X @ op - B0 if right else op @ X - B0
        res = (torch.linalg.norm(R_) / (torch.linalg.norm(op) * torch.linalg.norm(X) + torch.linalg.norm(B0))).item()
        assert res <= 4 * n * EPS, res


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


def _solve_residual(op, X, B0):
    return (torch.linalg.norm(op @ X - B0) / (torch.linalg.norm(op) * torch.linalg.norm(X) + torch.linalg.norm(B0))).item()


@pytest.mark.parametrize("N,nb", [(1024, 256), (900, 256), (384, 128)])
def test_dgetrf_nopiv_hbm_resident(pa, dev, N, nb):
    A0, LUref, ref_bwd = _reference(N, 300 + N)
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        _fill_store(sa, A0, nb, nb)
        torch.cuda.synchronize()
        tp, info = pa.dgetrf_nopiv_new(A)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        F = _dense_of(sa, N, N, nb, nb).cpu()
        bwd = _lu_backward(F, A0)
        diff = (F - LUref).abs().max().item()
        print(f"dgetrf_nopiv N={N} nb={nb}: backward error {bwd:.3e}, torch {ref_bwd:.3e}, ratio {bwd / ref_bwd:.2f}, max |ours - torch| {diff:.3e}")
        assert bwd <= 4 * ref_bwd
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


@pytest.mark.parametrize("trans", [0, 1])
def test_dgetrs_nopiv(pa, dev, trans):
    """Both transposes on torch's factor; B's tile width differs from nb and N has a ragged last tile."""
    N, nb, NRHS, nbr = 900, 256, 200, 128
    A0, LUref, _ = _reference(N, 300 + N)
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        B, sb = _gpu_matrix(pa, gpu, N, NRHS, nb, nbr)
        g = torch.Generator().manual_seed(5)
        B0 = torch.randn((N, NRHS), dtype=torch.float64, generator=g)
        _fill_store(sa, LUref, nb, nb)
        _fill_store(sb, B0, nb, nbr)
        torch.cuda.synchronize()
        tp = pa.dgetrs_nopiv_new(pa.MATRIX_TRANS if trans else pa.MATRIX_NOTRANS, A, B)
        assert tp is not None
        _run(ctx, tp)
        pa.taskpool_free(tp)
        op = A0.t() if trans else A0
        X = _dense_of(sb, N, NRHS, nb, nbr).cpu()
        ref = _solve_residual(op, torch.linalg.solve(op, B0), B0)
        res = _solve_residual(op, X, B0)
        print(f"dgetrs_nopiv trans={trans}: residual {res:.3e}, torch.linalg.solve {ref:.3e}, ratio {res / ref:.2f}")
        assert res <= 4 * ref
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


def test_dgesv_nopiv(pa, dev):
    """Factor and solve in one composed taskpool; then the same with an exact
    zero pivot: info names it, the run terminates, B is bit-identical."""
    N, nb, NRHS, nbr = 1024, 256, 256, 128
    A0, _, _ = _reference(N, 300 + N)
    ctx = pa.init(3)
    try:
        gpu = pa.first_gpu_device_index()
        A, sa = _gpu_matrix(pa, gpu, N, N, nb, nb)
        B, sb = _gpu_matrix(pa, gpu, N, NRHS, nb, nbr)
        g = torch.Generator().manual_seed(6)
        B0 = torch.randn((N, NRHS), dtype=torch.float64, generator=g)
        _fill_store(sa, A0, nb, nb)
        _fill_store(sb, B0, nb, nbr)
        torch.cuda.synchronize()
        tp, info = pa.dgesv_nopiv_new(A, B)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        pa.taskpool_free(tp)
        X = _dense_of(sb, N, NRHS, nb, nbr).cpu()
        ref = _solve_residual(A0, torch.linalg.solve(A0, B0), B0)
        res = _solve_residual(A0, X, B0)
        print(f"dgesv_nopiv: residual {res:.3e}, torch.linalg.solve {ref:.3e}, ratio {res / ref:.2f}")
        assert res <= 4 * ref
        assert _gpu_tasks(pa) > 0
        # an exact zero pivot in the second tile: global index 300 + 1
        _fill_store(sa, _zero_pivot_matrix(N, 300), nb, nb)
        _fill_store(sb, B0, nb, nbr)
        torch.cuda.synchronize()
        before = sb.clone()
        tp, info = pa.dgesv_nopiv_new(A, B)
        _run(ctx, tp)
        assert pa.read_int(info) == 301
        pa.taskpool_free(tp)
        torch.cuda.synchronize()
        assert torch.equal(sb, before)
    finally:
        ctx.fini()


def test_dgesv_nopiv_host_resident_staged(pa, dev):
    """Tiles on the host: staged into the HBM tile cache and written back; the
    result is read from B.tile(m, n)."""
    N, nb, NRHS, nbr = 512, 128, 256, 64
    A0, _, _ = _reference(N, 300 + N)
    ctx = pa.init(3)
    try:
        A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
        B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS)
        S = A0.numpy()
        B0 = np.random.default_rng(4).standard_normal((N, NRHS))
        for m in range(A.mt):
            for n in range(A.nt):
                A.tile(m, n)[:, :] = S[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb]
        for m in range(B.mt):
            for n in range(B.nt):
                B.tile(m, n)[:, :] = B0[m * nb:(m + 1) * nb, n * nbr:(n + 1) * nbr]
        tp, info = pa.dgesv_nopiv_new(A, B)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        pa.taskpool_free(tp)
        X = np.zeros((N, NRHS))
        for m in range(B.mt):
            for n in range(B.nt):
                X[m * nb:(m + 1) * nb, n * nbr:(n + 1) * nbr] = B.tile(m, n)
        Bt = torch.from_numpy(B0)
        ref = _solve_residual(A0, torch.linalg.solve(A0, Bt), Bt)
        res = _solve_residual(A0, torch.from_numpy(X), Bt)
        print(f"dgesv_nopiv host-resident: residual {res:.3e}, torch.linalg.solve {ref:.3e}, ratio {res / ref:.2f}")
        assert res <= 4 * ref
        gpus = [d for d in pa.devices() if d["type"] == pa.DEV_HIP]
        assert gpus[0]["executed_tasks"] > 0 and gpus[0]["bytes_in"] > 0
    finally:
        ctx.fini()
