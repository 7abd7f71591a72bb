"""Host-only launch plan of the grouped DGEMM (pa.kernel_gemm_launch_plan): the
launches pa.kernel_dgemm_batch_ex would issue for a descriptor list, decided
from the descriptors, the policy settings and an explicit slot count alone. The
cases are the decisions no GPU test asserts: leading dimensions that leave the
pinned k-loop body, yielding and claiming launches, mixed-mode batches and the
halved slots of a padded launch. No allocation, no GPU: the pointers are 0 and
never read."""
import contextlib

import pytest

SLOTS = 512


@contextlib.contextmanager
def _policy(pa, tile=0, fill=1):
    """the settings a plan depends on, pinned for the block and restored after"""
    prev = (pa.kernel_gemm_tile_policy(tile), pa.kernel_gemm_chunk_fill(fill), pa.kernel_gemm_splitk(1), pa.kernel_gemm_mainloop(1),
            pa.kernel_gemm_pipeline(1))
    try:
        yield
    finally:
        pa.kernel_gemm_tile_policy(prev[0])
        pa.kernel_gemm_chunk_fill(prev[1])
        pa.kernel_gemm_splitk(prev[2])
        pa.kernel_gemm_mainloop(prev[3])
        pa.kernel_gemm_pipeline(prev[4])


def _desc(m, n, k, alpha=-1.0, beta=1.0, ta=0, tb=1, lda=None, ldb=None):
    """op(A) m x k, op(B) k x n, tightly stored unless a leading dimension is given"""
    return dict(m=m, n=n, k=k, alpha=alpha, beta=beta, transA=ta, transB=tb, lda=lda or (k if ta else m), ldb=ldb or (n if tb else k), ldc=m)


def _one(pa, descs, **kw):
    plan = pa.kernel_gemm_launch_plan(descs, SLOTS, **kw)
    assert len(plan) == 1, plan
    return plan[0]


def _has(rec, **want):
    for key, val in want.items():
        assert rec[key] == val, (key, val, rec)


def test_tile_shape_and_full_kernel(pa):
    d = _desc(128, 256, 48, alpha=-1.0, beta=0.5)
    with _policy(pa, tile=0):
        _has(_one(pa, [d]), BM=64, BN=64, grid=8, total_tiles=8, main_tiles=8, ksplit=1, full=True, epilogue=0, rotated=True, pipelined=True,
             transA=0, transB=1, descs=1, pad_bytes=0)
    with _policy(pa, tile=128):
        _has(_one(pa, [d]), BM=128, BN=128, grid=2, full=True, epilogue=0, rotated=True, pipelined=True)


def test_ragged_descriptor_takes_the_checked_kernel(pa):
    with _policy(pa):
        _has(_one(pa, [_desc(200, 136, 77)]), full=False, epilogue=0, rotated=False, pipelined=False)


def test_atomic_epilogue_from_k_1024(pa):
    with _policy(pa, tile=128):
        _has(_one(pa, [_desc(128, 256, 1024, alpha=-1.0, beta=1.0)]), full=True, epilogue=1)
        _has(_one(pa, [_desc(128, 256, 1008, alpha=-1.0, beta=1.0)]), full=True, epilogue=0)


def test_split_k_tail(pa):
    """8320 x 1024 = 65 x 8 = 520 tiles of 128 x 128: one round of 512 and a tail of 8"""
    with _policy(pa):
        _has(_one(pa, [_desc(8320, 1024, 512)]), BM=128, total_tiles=520, main_tiles=512, ksplit=2, grid=528, epilogue=0)
        _has(_one(pa, [_desc(8320, 1024, 2048)]), total_tiles=520, main_tiles=512, ksplit=8, grid=576, epilogue=1)
        # partial sums are added into C: beta must be 1
        _has(_one(pa, [_desc(8320, 1024, 512, beta=0.5)]), total_tiles=520, main_tiles=520, ksplit=1, grid=520)


def test_padded_launch_halves_the_slots(pa):
    """256 slots: two rounds and a tail of 8, ksplit = min(256 / 8, 512 / 256, 8)"""
    with _policy(pa):
        _has(_one(pa, [_desc(8320, 1024, 512)], one_per_cu=True), total_tiles=520, main_tiles=512, ksplit=2, grid=528, pad_bytes=8192)
        # the pad belongs to the 128 x 128 kernel alone
        _has(_one(pa, [_desc(128, 256, 48)], one_per_cu=True), BM=64, pad_bytes=0)


def test_pinned_body_needs_32_bit_offsets(pa):
    """NT: a k-tile spans 16 columns of A, 16 * 2^25 * 8 = 2^32 bytes"""
    with _policy(pa, tile=128):
        _has(_one(pa, [_desc(128, 128, 64, lda=2 ** 25)]), full=True, rotated=True, pipelined=False)
        _has(_one(pa, [_desc(128, 128, 64, lda=2 ** 25 - 2)]), full=True, rotated=True, pipelined=True)


def test_yield_and_claim_keep_the_compiler_scheduled_body(pa):
    d = _desc(128, 256, 48)
    with _policy(pa):
        _has(_one(pa, [d], bulk_yield=True), full=True, rotated=True, pipelined=False)
        _has(_one(pa, [d], claim=2), full=True, rotated=True, pipelined=False)
        _has(_one(pa, [d], claim=1), full=True, rotated=True, pipelined=True)  # priority alone claims no CU


def test_mixed_modes_and_the_k0_group(pa):
    descs = [_desc(64, 64, 16, ta=0, tb=0), _desc(64, 64, 16, ta=0, tb=1), _desc(128, 64, 16, ta=0, tb=1), _desc(64, 64, 16, ta=1, tb=0),
             _desc(64, 64, 16, alpha=0.0, ta=1, tb=1), _desc(64, 64, 0, ta=0, tb=1)]
    with _policy(pa):
        plan = pa.kernel_gemm_launch_plan(descs, SLOTS)
    assert [(r["transA"], r["transB"], r["descs"]) for r in plan] == [(0, 0, 1), (0, 1, 2), (1, 0, 1), (0, 0, 2)]
    _has(plan[1], total_tiles=3, grid=3, full=True)
    _has(plan[3], full=False, epilogue=0, rotated=False, pipelined=False, total_tiles=2)


def test_chunk_cut(pa):
    descs = [_desc(512, 512, 512)] * 40
    with _policy(pa, tile=128, fill=1):
        plan = pa.kernel_gemm_launch_plan(descs, SLOTS)
        assert [r["descs"] for r in plan] == [32, 8] == pa.kernel_gemm_chunk_plan([(512, 512)] * 40, SLOTS)
        assert [r["total_tiles"] for r in plan] == [512, 128]
    with _policy(pa, tile=128, fill=0):
        assert [r["descs"] for r in pa.kernel_gemm_launch_plan(descs, SLOTS)] == [40]


def test_plan_rejects_unknown_keys_and_empty_lists(pa):
    assert pa.kernel_gemm_launch_plan([], SLOTS) == []
    with pytest.raises(ValueError):
        pa.kernel_gemm_launch_plan([dict(m=64, n=64, k=16, inplace=1)], SLOTS)
