"""Grouped DGEMM (dgemm_batch_kernel / gemm_tile): every test names the dispatch
path it means to run, reads the host's launch record (pa.kernel_gemm_launch_log)
and asserts that path before it looks at a number.

Two oracles:
  exact     operands are integers in [-4, 4] stored as fp64 and alpha, beta come
            from {1, -1, 2, 0.5, -0.25, 0}: every product, partial sum, preload
            scale beta / alpha and result is a dyadic number far below 2^53, so
            any summation order (the f64 atomics of split-K and of the atomic
            epilogue included) gives the same bits as the CPU fp64 matmul. The
            assertion is torch.equal over the whole C buffer: the result and
            everything around it (ldc padding, the upper triangle under
            lower_only, the doubles in front of and behind the matrix).
  rounding  standard normal operands against numpy.longdouble with the
            elementwise bound (k + 16) 2^-53 (|alpha| |op(A)| |op(B)| + |beta| |C0|):
            the gamma bound of k fused multiply-adds in any order, plus slack for
            the alpha / beta scaling, the preload and up to 8 split-K partial adds.
"""
import contextlib
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

MODES = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (transA, transB): NN, NT, TN, TT
MODE_IDS = ["NN", "NT", "TN", "TT"]
TILES = [0, 128]
SENTINEL = 777.0  # fills whatever of a buffer is not the matrix
AB = [(-1.0, 0.5), (2.0, -0.25)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _exact_oracle_is_exact():
    """one 64 x 64 block of an fp64 CPU reference against the int64 matmul"""
    g = torch.Generator().manual_seed(1)
    A = torch.randint(-4, 5, (200, 77), generator=g)
    B = torch.randint(-4, 5, (77, 136), generator=g)
    ref = A.double() @ B.double()
    assert torch.equal(ref[:64, :64], (A[:64] @ B[:, :64]).double())


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Mat:
    """rows x cols column-major matrix with leading dimension ld, `off` doubles
    into a flat buffer that is SENTINEL everywhere else (two more behind it)."""

    def __init__(self, rows, cols, ld=None, off=0, fill="int", gen=None):
        self.rows, self.cols, self.off = rows, cols, off
        self.ld = max(1, rows) if ld is None else ld
        assert self.ld >= rows
        self.size = off + self.ld * max(1, cols) + 2
        self.h = torch.full((self.size,), SENTINEL, dtype=torch.float64)
        v = self.of(self.h)
        if fill == "int":
            v.copy_(torch.randint(-4, 5, (rows, cols), generator=gen).double())
        elif fill == "randn":
            v.copy_(torch.randn((rows, cols), generator=gen, dtype=torch.float64))
        else:
            v.fill_(fill)
        self.d = None

    def of(self, flat):
        """the rows x cols view of a flat buffer laid out like this one"""
        return flat[self.off:self.off + self.ld * self.cols].view(self.cols, self.ld).t()[:self.rows]

    @property
    def v(self):
        return self.of(self.h)

    def to(self, dev):
        self.d = self.h.to(dev)
        return self

    @property
    def ptr(self):
        return self.d.data_ptr() + 8 * self.off

    def get(self):
        return self.d.cpu()


def _operand(rows, cols, trans, ld_extra=0, off=0, fill="int", gen=None):
    """storage of op(X) (rows x cols): X itself, or cols x rows when transposed;
    returns (Mat, op(X) as a CPU view)"""
    if trans:
        M = Mat(cols, rows, cols + ld_extra, off, fill, gen)
        return M, M.v.t()
    M = Mat(rows, cols, rows + ld_extra, off, fill, gen)
    return M, M.v


def _expect_full(bm, m, n, k, *mats):
    """the host's rule for the unchecked launch: whole bm x bm x 16 tiles, even
    leading dimensions and 16-byte aligned operands"""
    return m % bm == 0 and n % bm == 0 and k % 16 == 0 and k > 0 and all(M.ld % 2 == 0 and M.off % 2 == 0 for M in mats)


def _bm(tile, m, n):
    """tile size the policy picks for ONE descriptor (auto: 128 x 128 from 384 tiles on)"""
    if tile == 128:
        return 128
    t128 = ((m + 127) // 128) * ((n + 127) // 128)
    return 128 if (m >= 128 and n >= 128 and t128 >= 384) else 64


@contextlib.contextmanager
def _recording(pa, tile=None, fill=None, splitk=None):
    """policies for the block, launch log on and empty; everything restored after"""
    prev_tile = pa.kernel_gemm_tile_policy(-1 if tile is None else tile)
    prev_fill = pa.kernel_gemm_chunk_fill(-1 if fill is None else fill)
    prev_split = pa.kernel_gemm_splitk(-1 if splitk is None else splitk)
    pa.kernel_gemm_launch_log(True, reset=True)
    try:
        yield
    finally:
        pa.kernel_gemm_launch_log(False, reset=True)
        pa.kernel_gemm_splitk(prev_split)
        pa.kernel_gemm_chunk_fill(prev_fill)
        pa.kernel_gemm_tile_policy(prev_tile)


def _one_launch(pa, **want):
    log = pa.kernel_gemm_launch_log()
    assert len(log) == 1, log
    for key, val in want.items():
        assert log[0][key] == val, (key, val, log[0])
    return log[0]


def _desc(A, B, C, m, n, k, alpha, beta, ta, tb, **extra):
    d = dict(A=A.ptr, B=B.ptr, C=C.ptr, m=m, n=n, k=k, lda=A.ld, ldb=B.ld, ldc=C.ld, alpha=alpha, beta=beta, transA=ta, transB=tb)
    d.update(extra)
    return d


def _expected(C, ref, lower=False):
    """the whole C buffer as it must look: ref inside the matrix (its lower
    triangle under lower_only), the initial contents everywhere else"""
    want = C.h.clone()
    w = C.of(want)
    if lower:
        low = torch.tril(torch.ones(ref.shape, dtype=torch.bool))
        w[low] = ref[low]
    else:
        w.copy_(ref)
    return want


def _run_exact(pa, dev, tile, m, n, k, ta, tb, alpha, beta, ld_extra=0, off=0, c_fill="int", seed=0, **log_want):
    g = torch.Generator().manual_seed(1000 * seed + 7 * m + 3 * n + k + 2 * ta + tb)
    A, opA = _operand(m, k, ta, ld_extra, off, gen=g)
    B, opB = _operand(k, n, tb, ld_extra, off, gen=g)  # stored n x k when transB
    C = Mat(m, n, m + ld_extra, fill=c_fill, gen=g)
    ref = alpha * (opA @ opB)
    if beta != 0.0:
        ref = ref + beta * C.v
    for M in (A, B, C):
        M.to(dev)
    bm = _bm(tile, m, n)
    with _recording(pa, tile=tile):
        assert pa.kernel_dgemm_batch_ex([_desc(A, B, C, m, n, k, alpha, beta, ta, tb)], _stream()) == 0
        torch.cuda.synchronize()
        rec = _one_launch(pa, BM=bm, BN=bm, transA=ta, transB=tb, descs=1, ksplit=1, full=_expect_full(bm, m, n, k, A, B), **log_want)
        assert rec["main_tiles"] == rec["total_tiles"] == rec["grid"] == math.ceil(m / bm) * math.ceil(n / bm)
        assert rec["rotated"] == (rec["full"] and pa.kernel_gemm_mainloop(-1) == 1)
    got = C.get()
    assert torch.equal(got, _expected(C, ref)), (C.of(got) - ref).abs().max().item()
    return rec


# ------------------------------------------------------------ 1. operand modes
SHAPES = [
    # m, n, k, ld_extra, pointer offset (doubles)
    (128, 256, 48, 0, 0),   # FULL under both tilings
    (200, 136, 77, 0, 0),   # ragged in m, n and k
    (130, 66, 18, 1, 0),    # odd lda, ldb, ldc
    (128, 128, 32, 0, 1),   # A, B 8-byte but not 16-byte aligned
    (1, 1, 1, 0, 0),
    (1, 130, 3, 0, 0),
    (67, 1, 2, 0, 0),
]


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + ("+ld" if s[3] else "") + ("+off" if s[4] else ""))
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_operand_modes(pa, dev, mode, tile, shape):
    m, n, k, ld_extra, off = shape
    for i, (alpha, beta) in enumerate(AB):
        rec = _run_exact(pa, dev, tile, m, n, k, mode[0], mode[1], alpha, beta, ld_extra, off, seed=i, epilogue=0)
        assert rec["full"] == (shape == SHAPES[0])


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("mode", MODES[2:], ids=MODE_IDS[2:])
def test_operand_modes_odd_k(pa, dev, mode, tile):
    """K = 17 with even leading dimensions and aligned pointers: only the odd K
    takes the k-contiguous loads of op(A) = A^T off their 16-byte path"""
    for i, (alpha, beta) in enumerate(AB):
        m, n, k = 132, 68, 17
        g = torch.Generator().manual_seed(40 + i)
        A = Mat(k, m, k + 1, gen=g)  # lda = 18 (and ldb of an untransposed B) stay even
        B = Mat(n, k, n, gen=g) if mode[1] else Mat(k, n, k + 1, gen=g)
        C = Mat(m, n, gen=g)
        ref = alpha * (A.v.t() @ (B.v.t() if mode[1] else B.v)) + beta * C.v
        for M in (A, B, C):
            M.to(dev)
        bm = _bm(tile, m, n)
        with _recording(pa, tile=tile):
            assert pa.kernel_dgemm_batch_ex([_desc(A, B, C, m, n, k, alpha, beta, 1, mode[1])], _stream()) == 0
            torch.cuda.synchronize()
            _one_launch(pa, BM=bm, transA=1, transB=mode[1], full=False, epilogue=0, ksplit=1, rotated=False)
        assert torch.equal(C.get(), _expected(C, ref))


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_rounding_bound_ragged(pa, dev, mode, tile):
    """200 x 136 x 77 with normal operands against longdouble, elementwise gamma bound"""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is not an 80-bit (or wider) format here: the rounding oracle needs one"
    m, n, k = 200, 136, 77
    ta, tb = mode
    alpha, beta = -1.0, 0.5
    g = torch.Generator().manual_seed(300 + 2 * ta + tb)
    A, opA = _operand(m, k, ta, fill="randn", gen=g)
    B, opB = _operand(k, n, tb, fill="randn", gen=g)
    C = Mat(m, n, fill="randn", gen=g)
    a, b, c0 = (x.contiguous().numpy().astype(np.longdouble) for x in (opA, opB, C.v))
    ref = alpha * (a @ b) + beta * c0
    bound = np.longdouble(k + 16) * np.longdouble(2.0) ** -53 * (abs(alpha) * (np.abs(a) @ np.abs(b)) + abs(beta) * np.abs(c0))
    for M in (A, B, C):
        M.to(dev)
    bm = _bm(tile, m, n)
    with _recording(pa, tile=tile):
        assert pa.kernel_dgemm_batch_ex([_desc(A, B, C, m, n, k, alpha, beta, ta, tb)], _stream()) == 0
        torch.cuda.synchronize()
        _one_launch(pa, BM=bm, transA=ta, transB=tb, full=False, epilogue=0, ksplit=1)
    got = C.get()
    err = np.abs(C.of(got).contiguous().numpy().astype(np.longdouble) - ref)
    print(f"max err / bound = {float((err / bound).max()):.3f}")
    assert (err <= bound).all(), float((err / bound).max())
    outside = got.clone()
    C.of(outside).copy_(C.v)
    assert torch.equal(outside, C.h)


# ----------------------------------------------------- 2. beta = 0 never reads C
@gpu
@pytest.mark.parametrize("shape", [(128, 256, 48), (200, 136, 77)], ids=["full", "ragged"])
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_beta_zero_ignores_nan_c(pa, dev, mode, tile, shape):
    m, n, k = shape
    for i, alpha in enumerate((-1.0, 2.0)):  # |alpha| = 1 is the C-preload path of the full launches
        _run_exact(pa, dev, tile, m, n, k, mode[0], mode[1], alpha, 0.0, c_fill=float("nan"), seed=10 + i, epilogue=0)


# ------------------------------------------ 3. atomic epilogue in all four modes
@gpu
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_atomic_epilogue_modes(pa, dev, mode):
    """beta 1, K >= 1024, full 128 x 128 tiles: accumulators from zero, alpha * acc
    added into C with f64 atomics"""
    _run_exact(pa, dev, 128, 128, 256, 1024, mode[0], mode[1], -1.0, 1.0, seed=20, epilogue=1)


# ------------------------------------------------- 4. split-K tail, really taken
_SPLIT_CACHE = {}


def _split_case(dev, key, m, n, k):
    """integer op(A) (m x k), op(B) (k x n), C0 and C0 - op(A) op(B), computed once per shape"""
    if key not in _SPLIT_CACHE:
        g = torch.Generator().manual_seed(50 + k)
        opA = torch.randint(-4, 5, (m, k), generator=g).double()
        opB = opA.t() if n is None else torch.randint(-4, 5, (k, n), generator=g).double()
        C0 = torch.randint(-4, 5, (m, opB.shape[1]), generator=g).double()
        _SPLIT_CACHE[key] = (opA, opB, C0, C0 - opA @ opB)
    return _SPLIT_CACHE[key]


def _store(x, trans, dev):
    """op(X) = x as a column-major Mat: x itself, or x^T when the operand is transposed"""
    src = x.t() if trans else x
    M = Mat(src.shape[0], src.shape[1], fill=0.0)
    M.v.copy_(src)
    return M.to(dev)


def _slots(dev):
    return 2 * torch.cuda.get_device_properties(dev).multi_processor_count


@gpu
@pytest.mark.parametrize("k,ksplit,epilogue", [(512, 2, 0), (2048, 8, 1)])
@pytest.mark.parametrize("mode", [(0, 1), (1, 0)], ids=["NT", "TN"])
def test_split_k_tail_taken(pa, dev, mode, k, ksplit, epilogue):
    """ONE descriptor of (slots / 8 + 1) x 8 128-tiles: 8 tiles more than one round
    of resident workgroups, which the auto policy runs as a split-K tail (K / 256
    ways, at most 8) added into C with f64 atomics"""
    slots = _slots(dev)
    mt, nt = slots // 8 + 1, 8
    assert slots < mt * nt <= slots + slots // 8
    m, n = 128 * mt, 128 * nt
    ta, tb = mode
    opA, opB, C0, ref = _split_case(dev, ("rect", k), m, n, k)
    A, B = _store(opA, ta, dev), _store(opB, tb, dev)
    C = Mat(m, n, fill=0.0)
    C.v.copy_(C0)
    C.to(dev)
    with _recording(pa, tile=0, splitk=1):
        assert pa.kernel_dgemm_batch_ex([_desc(A, B, C, m, n, k, -1.0, 1.0, ta, tb)], _stream()) == 0
        torch.cuda.synchronize()
        rec = _one_launch(pa, BM=128, transA=ta, transB=tb, full=True, ksplit=ksplit, epilogue=epilogue, total_tiles=mt * nt, main_tiles=slots)
    assert rec["ksplit"] >= 2 and rec["main_tiles"] < rec["total_tiles"]
    assert rec["grid"] == rec["main_tiles"] + (rec["total_tiles"] - rec["main_tiles"]) * rec["ksplit"]
    assert torch.equal(C.get(), _expected(C, ref))


@gpu
def test_split_k_tail_lower_only(pa, dev):
    """SYRK descriptor of t x t tiles, t^2 just above one round: the tail (which
    holds the last diagonal tile) is split; the upper triangle stays untouched"""
    slots = _slots(dev)
    t = math.isqrt(slots) + 1
    tail = t * t - slots
    assert 0 < tail and 2 * tail <= slots
    n, k = 128 * t, 512
    opA, _, C0, ref = _split_case(dev, ("syrk", k), n, None, k)
    A = _store(opA, 0, dev)
    C = Mat(n, n, fill=0.0)
    C.v.copy_(C0)
    C.to(dev)
    with _recording(pa, tile=0, splitk=1):
        assert pa.kernel_dgemm_batch_ex([_desc(A, A, C, n, n, k, -1.0, 1.0, 0, 1, lower_only=1)], _stream()) == 0
        torch.cuda.synchronize()
        rec = _one_launch(pa, BM=128, full=True, ksplit=2, epilogue=0, total_tiles=t * t, main_tiles=slots)
    assert rec["ksplit"] >= 2 and rec["main_tiles"] < rec["total_tiles"]
    assert torch.equal(C.get(), _expected(C, ref, lower=True))


# --------------------------------------------------- 6. chunking, host code only
def test_chunk_plan(pa):
    plan = pa.kernel_gemm_chunk_plan
    prev = pa.kernel_gemm_chunk_fill(1)
    try:
        assert plan([(1024, 1024)] * 9, 512) == [8, 1]
        assert plan([(512, 512)] * 40, 512) == [32, 8]
        assert plan([(512, 512)] * 31, 512) == [31]  # fewer tiles than one round: a single chunk
        assert plan([(128, 128)], 512) == [1]
        assert plan([], 512) == []
        for shapes in ([(64, 64)] * 45, [(512, 512)] * 100, [(1024, 1024)] * 41, [(128 * (1 + i % 7), 128 * (1 + i % 3)) for i in range(97)]):
            for slots in (1, 16, 512, 608):
                cuts = plan(shapes, slots)
                assert sum(cuts) == len(shapes)
                assert all(1 <= c <= 40 for c in cuts)
        pa.kernel_gemm_chunk_fill(0)
        assert plan([(1024, 1024)] * 9, 512) == [9]  # fixed launches of up to 40 descriptors
        assert plan([(512, 512)] * 45, 512) == [40, 5]
    finally:
        pa.kernel_gemm_chunk_fill(prev)


def test_chunk_fill_setter(pa):
    prev = pa.kernel_gemm_chunk_fill(-1)
    try:
        assert pa.kernel_gemm_chunk_fill(0) == prev
        assert pa.kernel_gemm_chunk_fill(-1) == 0
        assert pa.kernel_gemm_chunk_fill(1) == 0
        assert pa.kernel_gemm_chunk_fill(-1) == 1
    finally:
        pa.kernel_gemm_chunk_fill(prev)


# ------------------------------------------------------------ 7. grouped launches
def _small_group(dev, modes, m=64, n=64, k=16, seed=60):
    g = torch.Generator().manual_seed(seed)
    descs, checks = [], []
    for ta, tb in modes:
        A, opA = _operand(m, k, ta, gen=g)
        B, opB = _operand(k, n, tb, gen=g)
        C = Mat(m, n, gen=g)
        ref = 2.0 * (opA @ opB) - 0.25 * C.v
        for M in (A, B, C):
            M.to(dev)
        descs.append(_desc(A, B, C, m, n, k, 2.0, -0.25, ta, tb))
        checks.append((C, ref, (A, B)))
    return descs, checks


@gpu
def test_grouped_modes_and_chunk_cut(pa, dev):
    """45 descriptors of 64 x 64 x 16 in one call: 42 NN (more than the 40 a launch
    holds: cut 40 + 2) and one each NT, TN, TT in launches of their own"""
    modes = [(0, 0)] * 20 + [(0, 1)] + [(0, 0)] * 12 + [(1, 0), (1, 1)] + [(0, 0)] * 10
    descs, checks = _small_group(dev, modes)
    with _recording(pa, tile=0):
        assert pa.kernel_dgemm_batch_ex(descs, _stream()) == 0
        torch.cuda.synchronize()
        log = pa.kernel_gemm_launch_log()
    assert [(r["transA"], r["transB"], r["descs"]) for r in log] == [(0, 0, 40), (0, 0, 2), (0, 1, 1), (1, 0, 1), (1, 1, 1)]
    for r in log:
        assert (r["BM"], r["full"], r["epilogue"], r["ksplit"]) == (64, True, 0, 1), r
        assert r["total_tiles"] == r["grid"] == r["descs"]
    for C, ref, _ in checks:
        assert torch.equal(C.get(), _expected(C, ref))


@gpu
@pytest.mark.parametrize("tile", TILES)
def test_grouped_empty_descriptors(pa, dev, tile):
    """m = 0 and n = 0 descriptors between non-empty ones own no tile and write nothing"""
    descs, checks = _small_group(dev, [(0, 1)] * 5, m=70, n=66, k=18, seed=61)
    descs[1]["m"] = 0
    descs[3]["n"] = 0
    with _recording(pa, tile=tile):
        assert pa.kernel_dgemm_batch_ex(descs, _stream()) == 0
        torch.cuda.synchronize()
        bm = 128 if tile == 128 else 64
        per = math.ceil(70 / bm) * math.ceil(66 / bm)
        _one_launch(pa, BM=bm, descs=5, total_tiles=3 * per, full=False, epilogue=0, ksplit=1)
    for i, (C, ref, _) in enumerate(checks):
        if i in (1, 3):
            assert torch.equal(C.get(), C.h)
        else:
            assert torch.equal(C.get(), _expected(C, ref))


# ------------------------------------------- 8. structured flags through the ex binding
FLAG_SHAPES = [(256, 192, 256), (200, 136, 200)]


def _flag_case(pa, dev, tile, shape, mode, flag):
    m, n, k = shape
    ta, tb = mode
    g = torch.Generator().manual_seed(70 + 2 * ta + tb + m)
    A, opA = _operand(m, k, ta, gen=g)
    B, opB = _operand(k, n, tb, gen=g)
    extra = {}
    if flag == "a_lower":
        opA.copy_(torch.tril(opA))  # op(A) lower triangular, zeros above (writes through to A's storage)
        extra["a_lower"] = 1
    if flag == "b_upper":
        opB.copy_(torch.triu(opB))
        extra["b_upper"] = 1
    alpha, beta = -1.0, 0.5
    use_cin, use_c2 = flag in ("Cin", "Cin+C2"), flag in ("C2", "Cin+C2")
    C = Mat(m, n, m + 2, fill=float("nan") if use_cin else "int", gen=g)
    Cin = Mat(m, n, m + 4, gen=g)
    C2 = Mat(m, n, m + 6, gen=g)
    ref = alpha * (opA @ opB) + beta * (Cin.v if use_cin else C.v)
    for M in (A, B, C, Cin, C2):
        M.to(dev)
    if use_cin:
        extra.update(Cin=Cin.ptr, ldcin=Cin.ld)
    if use_c2:
        extra.update(C2=C2.ptr, ldc2=C2.ld)
    bm = _bm(tile, m, n)
    with _recording(pa, tile=tile):
        assert pa.kernel_dgemm_batch_ex([_desc(A, B, C, m, n, k, alpha, beta, ta, tb, **extra)], _stream()) == 0
        torch.cuda.synchronize()
        _one_launch(pa, BM=bm, transA=ta, transB=tb, full=_expect_full(bm, m, n, k, A, B), epilogue=0, ksplit=1)
    assert torch.equal(C.get(), _expected(C, ref))
    assert torch.equal(Cin.get(), Cin.h)  # an input
    if use_c2:
        assert torch.equal(C2.get(), _expected(C2, C2.v - ref))  # C2_0 - what was written to C
    else:
        assert torch.equal(C2.get(), C2.h)


@gpu
@pytest.mark.parametrize("flag", ["a_lower", "b_upper", "Cin", "C2", "Cin+C2"])
@pytest.mark.parametrize("shape", FLAG_SHAPES, ids=["256x192x256", "200x136x200"])
@pytest.mark.parametrize("tile", TILES)
def test_structured_flags(pa, dev, tile, shape, flag):
    for mode in MODES:
        _flag_case(pa, dev, tile, shape, mode, flag)


# ------------------------------------------- 9. BLAS semantics of parsec_amd_dgemm
def _blas(pa, ta, tb, m, n, k, alpha, A, B, beta, C):
    return pa.kernel_dgemm_blas(ta, tb, m, n, k, alpha, A.ptr, A.ld, B.ptr, B.ld, beta, C.ptr, C.ld, _stream())


@gpu
@pytest.mark.parametrize("beta", [0.5, 0.0, 1.0])
@pytest.mark.parametrize("shape", [(128, 256), (200, 136)], ids=["tiles", "ragged"])
@pytest.mark.parametrize("tile", TILES)
def test_blas_k_zero_scales_c(pa, dev, tile, shape, beta):
    """K = 0: C := beta C (beta = 0: C := 0 whatever it held); no operand is read"""
    m, n = shape
    g = torch.Generator().manual_seed(80)
    for ta, tb in (("N", "N"), ("T", "N"), ("N", "T"), ("T", "T")):
        A, B = Mat(2, 2, max(m, 2), gen=g).to(dev), Mat(2, 2, max(n, 2), gen=g).to(dev)
        C = Mat(m, n, m + 2, fill=float("nan") if beta == 0.0 else "int", gen=g).to(dev)
        ref = torch.zeros(m, n, dtype=torch.float64) if beta == 0.0 else beta * C.v
        with _recording(pa, tile=tile):
            assert _blas(pa, ta, tb, m, n, 0, -1.0, A, B, beta, C) == 0
            torch.cuda.synchronize()
            _one_launch(pa, descs=1, full=False, epilogue=0, ksplit=1, rotated=False)
        assert torch.equal(C.get(), _expected(C, ref))


@gpu
@pytest.mark.parametrize("beta", [0.5, 0.0, 1.0])
@pytest.mark.parametrize("shape", [(128, 256, 48), (200, 136, 77)], ids=["tiles", "ragged"])
@pytest.mark.parametrize("tile", TILES)
def test_blas_alpha_zero_ignores_operands(pa, dev, tile, shape, beta):
    """alpha = 0: A and B are not referenced, so their NaN and Inf stay out of C"""
    m, n, k = shape
    g = torch.Generator().manual_seed(81)
    for ta, tb in (("N", "N"), ("T", "N"), ("N", "T"), ("T", "T")):
        A, _ = _operand(m, k, ta == "T", gen=g)
        B, _ = _operand(k, n, tb == "T", gen=g)
        A.v[::3, ::2] = float("nan")
        A.v[1::3, 1::2] = float("inf")
        B.v[::2, ::3] = float("-inf")
        B.v[1::2, 1::3] = float("nan")
        C = Mat(m, n, m + 2, fill=float("nan") if beta == 0.0 else "int", gen=g)
        ref = torch.zeros(m, n, dtype=torch.float64) if beta == 0.0 else beta * C.v
        for M in (A, B, C):
            M.to(dev)
        with _recording(pa, tile=tile):
            assert _blas(pa, ta, tb, m, n, k, 0.0, A, B, beta, C) == 0
            torch.cuda.synchronize()
            _one_launch(pa, descs=1, full=False, epilogue=0, ksplit=1, rotated=False)
        assert torch.equal(C.get(), _expected(C, ref))


@gpu
def test_blas_empty_c_launches_nothing(pa, dev):
    g = torch.Generator().manual_seed(82)
    A, B, C = (Mat(64, 64, gen=g).to(dev) for _ in range(3))
    with _recording(pa, tile=0):
        assert _blas(pa, "N", "N", 0, 64, 64, 1.0, A, B, 0.0, C) == 0
        assert _blas(pa, "N", "T", 64, 0, 64, 1.0, A, B, 0.0, C) == 0
        torch.cuda.synchronize()
        assert pa.kernel_gemm_launch_log() == []
    assert torch.equal(C.get(), C.h)


@gpu
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("tb", ["N", "n", "T", "t", "C", "c"])
@pytest.mark.parametrize("ta", ["N", "n", "T", "t", "C", "c"])
def test_blas_modes_ragged(pa, dev, ta, tb, tile):
    """every spelling of the operand letters at 200 x 136 x 77; 't', 'c', 'C' transpose"""
    m, n, k = 200, 136, 77
    tA, tB = int(ta in "TtCc"), int(tb in "TtCc")
    alpha, beta = 2.0, -0.25
    g = torch.Generator().manual_seed(90 + 2 * tA + tB)
    A, opA = _operand(m, k, tA, gen=g)
    B, opB = _operand(k, n, tB, gen=g)
    C = Mat(m, n, m + 1, gen=g)
    ref = alpha * (opA @ opB) + beta * C.v
    for M in (A, B, C):
        M.to(dev)
    bm = _bm(tile, m, n)
    with _recording(pa, tile=tile):
        assert _blas(pa, ta, tb, m, n, k, alpha, A, B, beta, C) == 0
        torch.cuda.synchronize()
        _one_launch(pa, BM=bm, transA=tA, transB=tB, full=False, epilogue=0, ksplit=1)
    assert torch.equal(C.get(), _expected(C, ref))
