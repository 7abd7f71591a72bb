"""The rotated k loop of the grouped DGEMM (pa.kernel_gemm_mainloop(1)) against
fp64 torch references and, bit for bit, against the plain loop (mode 0): every
accumulator takes its MFMAs in the same ascending k order in both loops, so only
the split-K tail (unordered f64 atomic adds) is exempt from bit-equality."""
import contextlib

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


def _cm(rows, cols, dev, gen):
    """rows x cols column-major fp64 matrix (ld = rows)"""
    return torch.randn((cols, rows), dtype=torch.float64, device=dev, generator=gen).t()


@contextlib.contextmanager
def _policy(pa, tile):
    """tile policy (0 auto, 64, 128) for the block; mainloop and policy restored after"""
    prev_tile = pa.kernel_gemm_tile_policy(tile)
    prev_loop = pa.kernel_gemm_mainloop(-1)
    try:
        yield
    finally:
        pa.kernel_gemm_mainloop(prev_loop)
        pa.kernel_gemm_tile_policy(prev_tile)


def _both(pa, outs, launch):
    """Runs launch() with the plain and the rotated loop from the same initial
    outputs; returns the two lists of results (clones)."""
    init = [o.clone() for o in outs]
    res = []
    for mode in (0, 1):
        for o, i in zip(outs, init):
            o.copy_(i)
        pa.kernel_gemm_mainloop(mode)
        assert launch() == 0
        torch.cuda.synchronize()
        assert pa.kernel_gemm_mainloop(-1) == mode
        res.append([o.clone() for o in outs])
    return res


def _err(C, ref):
    # the measure and bound of tests/test_kernels_gpu.py::test_dgemm
    return (C - ref).abs().max().item() / max(1.0, ref.abs().max().item())


TOL = 1e-12


def _gemm_case(pa, dev, m, n, k, transB, alpha, beta, lower=0):
    g = torch.Generator(device=dev).manual_seed(m * 7 + n + k + transB)
    A = _cm(m, k, dev, g)
    Bm = _cm(k, n, dev, g) if not transB else _cm(n, k, dev, g)
    C = _cm(m, n, dev, g)
    Bop = Bm.t() if transB else Bm
    ref = alpha * (A @ Bop) + beta * C
    r0, r1 = _both(pa, [C], lambda: pa.kernel_dgemm(A.data_ptr(), Bm.data_ptr(), C.data_ptr(), m, n, k, m, Bm.stride(1), m, alpha, beta, transB, lower, _stream()))
    for r in (r0, r1):
        assert _err(r[0], ref) < TOL, _err(r[0], ref)
    assert torch.equal(r0[0], r1[0])


def test_setter(pa, dev):
    prev = pa.kernel_gemm_mainloop(-1)
    try:
        assert pa.kernel_gemm_mainloop(1) == prev
        assert pa.kernel_gemm_mainloop(-1) == 1
        assert pa.kernel_gemm_mainloop(0) == 1
        assert pa.kernel_gemm_mainloop(-1) == 0
    finally:
        pa.kernel_gemm_mainloop(prev)


@pytest.mark.parametrize("m,n,k", [(128, 128, 16), (128, 128, 32), (128, 128, 48), (256, 128, 80)])
@pytest.mark.parametrize("transB", [0, 1])
def test_big_tiles(pa, dev, m, n, k, transB):
    """one, two, an odd number of and several k-tiles on 128x128 tiles"""
    with _policy(pa, 128):
        _gemm_case(pa, dev, m, n, k, transB, -1.0, 0.5)


def test_big_tiles_atomic_epilogue(pa, dev):
    """beta 1 and K >= 1024: accumulators from zero, C updated with f64 atomics"""
    with _policy(pa, 128):
        _gemm_case(pa, dev, 128, 256, 1024, 1, -1.0, 1.0)


@pytest.mark.parametrize("alpha", [-1.0, 2.0])
def test_big_tiles_c_preload(pa, dev, alpha):
    """|alpha| = 1: accumulators preloaded with (beta / alpha) C; otherwise C read in the epilogue"""
    with _policy(pa, 128):
        _gemm_case(pa, dev, 128, 128, 64, 1, alpha, 0.5)


@pytest.mark.parametrize("m,n,k", [(64, 64, 16), (64, 64, 48), (128, 192, 80)])
@pytest.mark.parametrize("transB", [0, 1])
def test_small_tiles(pa, dev, m, n, k, transB):
    with _policy(pa, 0):
        _gemm_case(pa, dev, m, n, k, transB, -1.0, 0.5)


@pytest.mark.parametrize("transB", [0, 1])
@pytest.mark.parametrize("tile", [0, 128])
def test_interior_blocks(pa, dev, tile, transB):
    """operands inside larger column-major arrays: lda, ldb, ldc > the block's
    rows, 16-byte aligned offsets (the per-thread offsets and uniform k steps of
    the rotated loop)"""
    m, n, k = 256, 128, 48
    g = torch.Generator(device=dev).manual_seed(77 + transB)
    bigA, bigB, bigC = _cm(300, 70, dev, g), _cm(210, 150, dev, g), _cm(290, 140, dev, g)
    A = bigA[6:6 + m, 4:4 + k]
    Bm = bigB[10:10 + n, 2:2 + k] if transB else bigB[8:8 + k, 3:3 + n]
    C = bigC[12:12 + m, 5:5 + n]
    Bop = Bm.t() if transB else Bm
    ref = -1.0 * (A @ Bop) + 0.5 * C
    big0 = bigC.clone()
    with _policy(pa, tile):
        r0, r1 = _both(pa, [bigC], lambda: pa.kernel_dgemm(A.data_ptr(), Bm.data_ptr(), C.data_ptr(), m, n, k, 300, 210, 290, -1.0, 0.5, transB, 0, _stream()))
    for r in (r0, r1):
        assert _err(r[0][12:12 + m, 5:5 + n], ref) < TOL
        outside = r[0].clone()
        outside[12:12 + m, 5:5 + n] = big0[12:12 + m, 5:5 + n]
        assert torch.equal(outside, big0)  # nothing written around the block
    assert torch.equal(r0[0], r1[0])


@pytest.mark.parametrize("tile", [0, 128])
def test_syrk_lower_only(pa, dev, tile):
    n, k = 256, 48
    g = torch.Generator(device=dev).manual_seed(5)
    A, C = _cm(n, k, dev, g), _cm(n, n, dev, g)
    C0 = C.clone()
    ref = C0 - A @ A.t()
    with _policy(pa, tile):
        r0, r1 = _both(pa, [C], lambda: pa.kernel_dgemm(A.data_ptr(), A.data_ptr(), C.data_ptr(), n, n, k, n, n, n, -1.0, 1.0, 1, 1, _stream()))
    low = torch.tril(torch.ones(n, n, dtype=torch.bool, device=dev))
    for r in (r0, r1):
        assert _err(r[0][low], ref[low]) < TOL
        assert torch.equal(r[0][~low], C0[~low])  # upper triangle untouched
    assert torch.equal(r0[0], r1[0])


@pytest.mark.parametrize("tile", [0, 128])
def test_trsm_through_inverse_triangular_k(pa, dev, tile):
    """Panel solve B := B L^-T as a grouped GEMM with W = L^-1 (construction of
    tests/test_kernels_gpu.py::test_trsm_through_inverse): the descriptors carry
    a truncated K range per column block (op(B) upper triangular)."""
    m = n = 256
    tasks = 2
    g = torch.Generator(device=dev).manual_seed(9)
    R = torch.randn((n, n), dtype=torch.float64, device=dev, generator=g)
    L = torch.linalg.cholesky(R @ R.t() + n * torch.eye(n, dtype=torch.float64, device=dev))
    W = torch.empty((n, n), dtype=torch.float64, device=dev).t()
    W.copy_(torch.linalg.inv(L))
    Bs = [_cm(m, n, dev, g) for _ in range(tasks)]
    refs = [torch.linalg.solve_triangular(L, B.t(), upper=False).t() for B in Bs]  # X L^T = B
    descs = [(B.data_ptr(), W.data_ptr(), m, n, m, n) for B in Bs]
    with _policy(pa, tile):
        r0, r1 = _both(pa, Bs, lambda: pa.kernel_trsm_w_batch(descs, _stream()))
    for r in (r0, r1):
        for X, ref in zip(r, refs):
            assert _err(X, ref) < TOL, _err(X, ref)
    for X0, X1 in zip(r0, r1):
        assert torch.equal(X0, X1)


def test_split_k_tail(pa, dev):
    """9 descriptors of 1024^3 = 576 128-tiles on 512 resident slots: the 64
    tiles of the second round are split along K (BK-multiple chunks through the
    rotated loop) and added into C with f64 atomics. Bound of
    tests/test_headline_gpu.py::test_dgemm_batch_split_k_tail; the add order is
    not fixed, so no bit-equality."""
    g = torch.Generator(device=dev).manual_seed(21)
    n, cnt = 1024, 9
    As = [_cm(n, n, dev, g) for _ in range(cnt)]
    Bs = [_cm(n, n, dev, g) for _ in range(cnt)]
    Cs = [_cm(n, n, dev, g) for _ in range(cnt)]
    refs = [C - A @ B.t() for A, B, C in zip(As, Bs, Cs)]
    descs = [(A.data_ptr(), B.data_ptr(), C.data_ptr(), n, n, n, n, n, n, -1.0, 1.0, 1, 0) for A, B, C in zip(As, Bs, Cs)]
    # one launch of all 9 per loop (the round-filling chunks would cut 8 + 1 and never split)
    prev = pa.kernel_gemm_splitk(1)
    prev_fill = pa.kernel_gemm_chunk_fill(0)
    pa.kernel_gemm_launch_log(True, reset=True)
    try:
        with _policy(pa, 0):
            res = _both(pa, Cs, lambda: pa.kernel_dgemm_batch(descs, _stream()))
        log = pa.kernel_gemm_launch_log()
    finally:
        pa.kernel_gemm_launch_log(False, reset=True)
        pa.kernel_gemm_chunk_fill(prev_fill)
        pa.kernel_gemm_splitk(prev)
    assert len(log) == 2, log  # the plain loop, then the rotated one
    for rec, rotated in zip(log, (False, True)):
        assert (rec["BM"], rec["descs"], rec["ksplit"], rec["rotated"], rec["full"]) == (128, cnt, 4, rotated, True), rec
        assert rec["total_tiles"] == 576 and rec["main_tiles"] < 576, rec
    for r in res:
        for C, ref in zip(r, refs):
            err = ((C - ref).abs().max() / ref.abs().max()).item()
            assert err < 1e-14, err


@pytest.mark.parametrize("tile", [0, 128])
def test_grouped_mixed_k(pa, dev, tile):
    """three descriptors with 1, 3 and 64 k-tiles in one launch (beta != 1: plain
    epilogue): every workgroup runs its own descriptor's k-tile count"""
    g = torch.Generator(device=dev).manual_seed(31)
    shapes = [(128, 128, 16), (256, 128, 48), (128, 256, 1024)]
    As = [_cm(m, k, dev, g) for m, n, k in shapes]
    Bs = [_cm(n, k, dev, g) for m, n, k in shapes]
    Cs = [_cm(m, n, dev, g) for m, n, k in shapes]
    refs = [0.5 * C - A @ B.t() for A, B, C in zip(As, Bs, Cs)]
    descs = [(A.data_ptr(), B.data_ptr(), C.data_ptr(), m, n, k, m, n, m, -1.0, 0.5, 1, 0) for (m, n, k), A, B, C in zip(shapes, As, Bs, Cs)]
    with _policy(pa, tile):
        r0, r1 = _both(pa, Cs, lambda: pa.kernel_dgemm_batch(descs, _stream()))
    for r in (r0, r1):
        for C, ref in zip(r, refs):
            assert _err(C, ref) < TOL, _err(C, ref)
    for C0, C1 in zip(r0, r1):
        assert torch.equal(C0, C1)
