"""Tile TRTRI / TRMM (L^T B) / LAUUM kernels and the DTRTRI, DLAUUM, DPOTRI and
DPOINV taskpools on the GPU, against fp64 references computed on the CPU.

The triangular operand always has NaN in its strict upper triangle (and, in the
kernel tests, a sentinel in the padding rows lda > n): neither may influence the
result and both must come back bit-identical. Tolerances: an inverse may have at
most 4 times the residual of torch's CPU reference (the project's margin for
kernels built on explicit 64-block inverses, test_dgetrf_gpu.py); TRMM and
LAUUM are products, so their bound is the derived one,
||result - exact||_F <= n eps || |L^T| |B| ||_F."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
SENTINEL = -7.25
NS = [1, 17, 64, 65, 130, 256, 300]
PADS = [0, 3]


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


_tiles = {}


def _tile(n, dev):
    """(L with NaN above, clean L on the GPU, clean L on the CPU, the residual of
    the CPU reference inverse), computed once per n."""
    if n not in _tiles:
        Lnan, L = _factor(n, dev, 100 + n)
        Lc = L.cpu()
        Xref = torch.linalg.solve_triangular(Lc, torch.eye(n, dtype=torch.float64), upper=False)
        _tiles[n] = (Lnan, L, Lc, _tri_residual(Xref, Lc))
    return _tiles[n]


def _padded(M, ld):
    """The column-major image of M (rows x cols) in a cols x ld buffer whose
    padding rows hold the sentinel: buf[c, r] = M[r, c]."""
    rows, cols = M.shape
    buf = torch.full((cols, ld), SENTINEL, dtype=torch.float64, device=M.device)
    buf[:, :rows] = M.t()
    return buf


def _bits(t):
    return t.contiguous().view(torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _tri_residual(X, L):
    n = L.shape[0]
    return (torch.linalg.norm(X @ L - torch.eye(n, dtype=L.dtype, device=L.device)) / (torch.linalg.norm(X) * torch.linalg.norm(L))).item()


def _inv_residual(S, X):
    n = S.shape[0]
    return (torch.linalg.norm(S @ X - torch.eye(n, dtype=S.dtype, device=S.device)) / (torch.linalg.norm(S) * torch.linalg.norm(X))).item()


def _check_triangle_tile(buf, before, n):
    """Lower triangle finite; strict upper triangle and padding rows bit-identical. Returns the clean lower triangle."""
    M = buf[:, :n].t()
    up = torch.triu(torch.ones(n, n, dtype=torch.bool, device=buf.device), diagonal=1)
    assert torch.isfinite(M[~up]).all()
    assert _same_bits(M[up], before[:, :n].t()[up])
    assert _same_bits(buf[:, n:], before[:, n:])
    return torch.tril(torch.nan_to_num(M))


# -------------------------------------------------------------------- kernels
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("n", NS)
def test_kernel_dtrtri(pa, dev, n, pad):
    Lnan, L, Lc, ref = _tile(n, dev)
    lda = n + pad
    # in place
    buf = _padded(Lnan, lda)
    before = buf.clone()
    assert pa.kernel_dtrtri(buf.data_ptr(), n, lda, stream=_stream()) == 0
    torch.cuda.synchronize()
    X = _check_triangle_tile(buf, before, n)
    res = _tri_residual(X.cpu(), Lc)
    print(f"dtrtri tile n={n} pad={pad} in place: residual {res:.3e}, solve_triangular {ref:.3e}, ratio {res / ref if ref else 0:.2f}")
    assert res <= 4 * ref
    # to W: A untouched
    buf = before.clone()
    W = _padded(Lnan, lda + 1)
    Wbefore = W.clone()
    assert pa.kernel_dtrtri(buf.data_ptr(), n, lda, W=W.data_ptr(), ldw=lda + 1, stream=_stream()) == 0
    torch.cuda.synchronize()
    assert _same_bits(buf, before)
    Xw = _check_triangle_tile(W, Wbefore, n)
    res = _tri_residual(Xw.cpu(), Lc)
    print(f"dtrtri tile n={n} pad={pad} to W: residual {res:.3e}, ratio {res / ref if ref else 0:.2f}")
    assert res <= 4 * ref


def test_kernel_dtrtri_zero_diagonal(pa, dev):
    """A zero on the diagonal is reported as info_base + its 1-based index, the
    kernel still finishes; a smaller value already in the word stays."""
    n = 130
    Lnan, _, _, _ = _tile(n, dev)
    L0 = Lnan.clone()
    L0[70, 70] = 0.0
    info = torch.zeros(1, dtype=torch.int32, device=dev)
    buf = _padded(L0, n)
    assert pa.kernel_dtrtri(buf.data_ptr(), n, n, info=info.data_ptr(), info_base=5, stream=_stream()) == 0
    torch.cuda.synchronize()
    assert info.item() == 76
    info.fill_(3)
    buf = _padded(L0, n)
    assert pa.kernel_dtrtri(buf.data_ptr(), n, n, info=info.data_ptr(), info_base=5, stream=_stream()) == 0
    torch.cuda.synchronize()
    assert info.item() == 3


def _rhs(n, nrhs, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn((n, nrhs), dtype=torch.float64, device=dev, generator=g)


def _product_check(got, Lc, Bc, alpha, n, what):
    """||got - alpha L^T B||_F <= n eps || |L^T| |B| ||_F, everything on the CPU in fp64."""
    exact = alpha * (Lc.t() @ Bc)
    err = torch.linalg.norm(got - exact).item()
    bound = n * EPS * torch.linalg.norm(Lc.t().abs() @ Bc.abs()).item()
    print(f"{what}: error {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound


@pytest.mark.parametrize("nrhs", [1, 16, 37])
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("n", NS)
def test_kernel_dtrmm_lt(pa, dev, n, pad, nrhs):
    Lnan, L, Lc, _ = _tile(n, dev)
    ld = n + pad
    alpha = -0.5
    Lbuf = _padded(Lnan, ld)
    Lbefore = Lbuf.clone()
    B0 = _rhs(n, nrhs, dev, 7 * n + nrhs)
    buf = _padded(B0, ld)
    before = buf.clone()
    assert pa.kernel_dtrmm_lt(Lbuf.data_ptr(), buf.data_ptr(), n, nrhs, ld, ld, alpha, _stream()) == 0
    torch.cuda.synchronize()
    assert _same_bits(Lbuf, Lbefore)
    assert _same_bits(buf[:, n:], before[:, n:])
    got = buf[:, :n].t()
    assert torch.isfinite(got).all()
    _product_check(got.cpu(), Lc, B0.cpu(), alpha, n, f"dtrmm tile n={n} pad={pad} nrhs={nrhs}")


def test_kernel_dtrmm_lt_grouped(pa, dev):
    """One grouped launch: descriptors of different n and nrhs over one L pointer
    (the leading n x n triangles of one tile)."""
    Lnan, L, Lc, _ = _tile(300, dev)
    ld = 303
    Lbuf = _padded(Lnan, ld)
    cases = [(300, 37, 1.0), (130, 16, -0.5), (64, 50, 2.0), (17, 1, 1.0), (256, 256, 1.0)]
    bufs, B0s, descs = [], [], []
    for i, (n, nrhs, alpha) in enumerate(cases):
        B0 = _rhs(n, nrhs, dev, 900 + i)
        buf = _padded(B0, n + i)
        B0s.append(B0)
        bufs.append(buf)
        descs.append((Lbuf.data_ptr(), buf.data_ptr(), n, nrhs, ld, n + i, alpha))
    befores = [b.clone() for b in bufs]
    assert pa.kernel_dtrmm_lt_batch(descs, _stream()) == 0
    torch.cuda.synchronize()
    for (n, nrhs, alpha), buf, before, B0 in zip(cases, bufs, befores, B0s):
        assert _same_bits(buf[:, n:], before[:, n:])
        _product_check(buf[:, :n].t().cpu(), Lc[:n, :n], B0.cpu(), alpha, n, f"grouped dtrmm n={n} nrhs={nrhs}")


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("n", NS)
def test_kernel_dlauum(pa, dev, n, pad):
    Lnan, L, Lc, _ = _tile(n, dev)
    lda = n + pad
    buf = _padded(Lnan, lda)
    before = buf.clone()
    assert pa.kernel_dlauum(buf.data_ptr(), n, lda, _stream()) == 0
    torch.cuda.synchronize()
    got = _check_triangle_tile(buf, before, n).cpu()
    exact = torch.tril(Lc.t() @ Lc)
    err = torch.linalg.norm(got - exact).item()
    bound = n * EPS * torch.linalg.norm(Lc.t().abs() @ Lc.abs()).item()
    print(f"dlauum tile n={n} pad={pad}: error {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(err) and err <= bound


# ------------------------------------------------------------------ taskpools
SHAPES = [(1024, 256), (900, 256), (384, 128), (200, 256)]


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


_matrices = {}


def _matrix(N):
    """On the CPU, once per N: S, torch's factor L, L with NaN above the diagonal,
    and the residuals of the CPU references (solve_triangular, cholesky_inverse)."""
    if N not in _matrices:
        S = _spd(N, "cpu", 10 + N)
        L = torch.linalg.cholesky(S)
        Ln = L.clone()
        Ln[torch.triu(torch.ones(N, N, dtype=torch.bool), diagonal=1)] = float("nan")
        tri_ref = _tri_residual(torch.linalg.solve_triangular(L, torch.eye(N, dtype=torch.float64), upper=False), L)
        inv_ref = _inv_residual(S, torch.cholesky_inverse(L))
        _matrices[N] = (S, L, Ln, tri_ref, inv_ref)
    return _matrices[N]


def _lower_result(store, before, N, nb):
    """The lower triangle of the result on the CPU. With `before` (the store as
    it was filled, NaN above the diagonal) everything else of the store --
    strictly upper tiles, upper triangles of diagonal tiles, the padding of edge
    tiles -- must be bit-identical to it."""
    G = _dense_of(store, N, N, nb, nb)
    up = torch.triu(torch.ones(N, N, dtype=torch.bool, device=G.device), diagonal=1)
    if before is not None:
        assert _same_bits(G[up], _dense_of(before, N, N, nb, nb)[up])
        NT = store.shape[0]
        full = torch.ones((NT * nb, NT * nb), dtype=torch.bool, device=G.device)
        full[:N, :N] = False  # the padding of the edge tiles
        pad_mask = full.reshape(NT, nb, NT, nb).permute(2, 0, 3, 1)
        assert _same_bits(store[pad_mask], before[pad_mask])
    low = G[~up]
    assert torch.isfinite(low).all()
    return torch.tril(torch.nan_to_num(G)).cpu()


def _sym(T):
    return T + torch.tril(T, -1).t()


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dtrtri_hbm_resident(pa, dev, N, nb):
    S, L, Ln, tri_ref, _ = _matrix(N)
    ctx = pa.init(3)
    try:
        A, sa = _gpu_matrix(pa, pa.first_gpu_device_index(), N, N, nb, nb)
        _fill_store(sa, Ln.to(dev), nb, nb)
        before = sa.clone()
        torch.cuda.synchronize()
        tp, info = pa.dtrtri_new(pa.MATRIX_LOWER, pa.MATRIX_NONUNIT, A)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        X = _lower_result(sa, before, N, nb)
        res = _tri_residual(X, L)
        print(f"dtrtri N={N} nb={nb}: residual {res:.3e}, solve_triangular {tri_ref:.3e}, ratio {res / tri_ref:.2f}")
        assert res <= 4 * tri_ref
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dlauum_hbm_resident(pa, dev, N, nb):
    S, L, Ln, _, _ = _matrix(N)
    ctx = pa.init(3)
    try:
        A, sa = _gpu_matrix(pa, pa.first_gpu_device_index(), N, N, nb, nb)
        _fill_store(sa, Ln.to(dev), nb, nb)
        before = sa.clone()
        torch.cuda.synchronize()
        tp = pa.dlauum_new(pa.MATRIX_LOWER, A)
        assert tp is not None
        _run(ctx, tp)
        got = _lower_result(sa, before, N, nb)
        err = torch.linalg.norm(got - torch.tril(L.t() @ L)).item()
        bound = N * EPS * torch.linalg.norm(L.t().abs() @ L.abs()).item()
        print(f"dlauum N={N} nb={nb}: error {err:.3e}, bound {bound:.3e}")
        assert np.isfinite(err) and err <= bound
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dpotri_hbm_resident(pa, dev, N, nb):
    S, L, Ln, _, inv_ref = _matrix(N)
    ctx = pa.init(3)
    try:
        A, sa = _gpu_matrix(pa, pa.first_gpu_device_index(), N, N, nb, nb)
        _fill_store(sa, Ln.to(dev), nb, nb)
        before = sa.clone()
        torch.cuda.synchronize()
        tp = pa.dpotri_new(pa.MATRIX_LOWER, A)
        assert tp is not None
        _run(ctx, tp)
        pa.taskpool_free(tp)
        X = _sym(_lower_result(sa, before, N, nb))
        res = _inv_residual(S, X)
        print(f"dpotri N={N} nb={nb}: residual {res:.3e}, cholesky_inverse {inv_ref:.3e}, ratio {res / inv_ref:.2f}")
        assert res <= 4 * inv_ref
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


@pytest.mark.parametrize("N,nb", SHAPES)
def test_dpoinv_hbm_resident(pa, dev, N, nb):
    S, L, _, _, inv_ref = _matrix(N)
    ctx = pa.init(3)
    try:
        A, sa = _gpu_matrix(pa, pa.first_gpu_device_index(), N, N, nb, nb)
        _fill_store(sa, S.to(dev), nb, nb)
        torch.cuda.synchronize()
        tp, info = pa.dpoinv_new(pa.MATRIX_LOWER, A)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        pa.taskpool_free(tp)
        X = _sym(_lower_result(sa, None, N, nb))
        res = _inv_residual(S, X)
        print(f"dpoinv N={N} nb={nb}: residual {res:.3e}, cholesky_inverse {inv_ref:.3e}, ratio {res / inv_ref:.2f}")
        assert res <= 4 * inv_ref
        assert _gpu_tasks(pa) > 0
    finally:
        ctx.fini()


def test_dpoinv_not_positive_definite(pa, dev):
    """One diagonal entry of the second tile is negative: info is what
    dpotrf_jdf_new alone reports, the run terminates, and A is bit-identical to
    what dpotrf_jdf_new alone leaves."""
    N, nb = 1024, 256
    S = _matrix(N)[0].clone()
    S[nb + 44, nb + 44] = -1.0
    ctx = pa.init(3)
    try:
        A, sa = _gpu_matrix(pa, pa.first_gpu_device_index(), N, N, nb, nb)
        _fill_store(sa, S.to(dev), nb, nb)
        torch.cuda.synchronize()
        tp, info = pa.dpotrf_jdf_new(A)
        _run(ctx, tp)
        want_info = pa.read_int(info)
        assert want_info != 0
        torch.cuda.synchronize()
        want = sa.clone()
        _fill_store(sa, S.to(dev), nb, nb)
        torch.cuda.synchronize()
        tp, info = pa.dpoinv_new(pa.MATRIX_LOWER, A)
        _run(ctx, tp)
        assert pa.read_int(info) == want_info
        pa.taskpool_free(tp)
        torch.cuda.synchronize()
        assert _same_bits(sa, want)
    finally:
        ctx.fini()


def test_dpoinv_host_resident_staged(pa, dev):
    """Tiles on the host: staged into the HBM tile cache and written back; the
    result is read from A.tile(m, n)."""
    N, nb = 512, 128
    S, L, _, _, inv_ref = _matrix(N)
    ctx = pa.init(3)
    try:
        A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N)
        Sn = S.numpy()
        for m in range(A.mt):
            for n in range(A.nt):
                A.tile(m, n)[:, :] = Sn[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb]
        tp, info = pa.dpoinv_new(pa.MATRIX_LOWER, A)
        _run(ctx, tp)
        assert pa.read_int(info) == 0
        pa.taskpool_free(tp)
        G = np.zeros((N, N))
        for m in range(A.mt):
            for n in range(A.nt):
                G[m * nb:(m + 1) * nb, n * nb:(n + 1) * nb] = A.tile(m, n)
        X = _sym(torch.tril(torch.from_numpy(G)))
        res = _inv_residual(S, X)
        print(f"dpoinv host-resident: residual {res:.3e}, cholesky_inverse {inv_ref:.3e}, ratio {res / inv_ref:.2f}")
        assert res <= 4 * inv_ref
        gpus = [d for d in pa.devices() if d["type"] == pa.DEV_HIP]
        assert gpus[0]["executed_tasks"] > 0 and gpus[0]["bytes_in"] > 0
    finally:
        ctx.fini()
