#!/usr/bin/env python3
"""The other BASELINE.json workloads, one JSON line each (rank 0):

  qr       tiled Householder QR (PTG DGEQRF: GEQRT/UNMQR/TSQRT/TSMQR), matrix and
           T factors resident in HBM, GFLOP/s with 4/3 N^3 (config 4)
  stencil  DTD 3D 7-point Jacobi stencil, halo faces between blocks (and ranks),
           GPU bodies, Gpoint-updates/s and GFLOP/s at 8 flop/point (config 5)
  dtd_gemm DTD tiled DGEMM C += A B on 4 x 4 tiles, CPU bodies in one process
           (config 1, the plumbing check), GFLOP/s
  potrs    solve with the Cholesky factor (DPOTRS = the two lower dtrsm_left.jdf sweeps):
           A factored once outside the timed region, every timed step restores B
           and solves, GFLOP/s with 2 N^2 NRHS; the same process then times
           torch.cholesky_solve on the dense factor (what a user does without it)
  gels     least squares with the tile QR factor, M >= N: DGEQRS (dormqr.jdf then
           dtrsm_left.jdf on a factor computed once outside the timed region) and
           DGELS (DGEQRF + DGEQRS in one taskpool), B (and for DGELS A, T)
           restored every timed step, GFLOP/s with 4 M N NRHS - N^2 NRHS (plus
           2 M N^2 - 2/3 N^3 for DGELS); the same process then times a torch
           yardstick on the dense data: torch.linalg.lstsq if it runs on the
           device, otherwise torch.linalg.qr + solve_triangular
  getrf    LU WITHOUT pivoting on a seeded, column diagonally dominant matrix:
           DGETRF_NOPIV alone (2/3 N^3) and DGESV_NOPIV (+ 2 N^2 NRHS), A (and
           B) restored every timed step, with the backward error
           ||L U - A||_F / ||A||_F; the same process then times
           torch.linalg.lu_factor / lu_solve on the dense data -- torch PIVOTS
           (partial pivoting), so the yardstick does more work than we do
  getrf_incpiv  tile LU with incremental (pairwise) pivoting on a seeded standard
           normal matrix (it needs pivoting): DGETRF_INCPIV and DGESV_INCPIV
           with A, L and B restored every timed step; GFLOP/s credited with
           2/3 N^3 (+ 2 N^2 NRHS), the flops executed (GETRF 2/3, GESSM 1,
           TSTRF 1, SSSSM 3 nb^3 each: about N^3) printed beside it; the same
           process then times torch.linalg.lu_factor / lu_solve, and the solve
           residual ||A X - B||_F / (||A||_F ||X||_F + ||B||_F) is printed for
           ours and torch's
  potri    the inverse with the Cholesky factor of a seeded SPD matrix: DTRTRI
           (N^3 / 3) and DPOTRI (2/3 N^3) on the dense factor torch computed,
           DPOINV (N^3) on the matrix, A restored every timed step; the same
           process then times torch.cholesky_inverse on that factor, and
           ||A X - I||_F / (||A||_F ||X||_F) is printed for ours and torch's.
           --cond C swaps in a matrix of condition number C

Multi-GPU: launch like bench.py (torch.distributed.run, one rank per GPU).

    python benchmarks/bench_workloads.py qr --n 16384 --nb 512
    python benchmarks/bench_workloads.py stencil --n 512 --b 128 --iters 20
    python benchmarks/bench_workloads.py dtd_gemm --n 2048
    python benchmarks/bench_workloads.py potrs --n 16384 --nb 512 --nrhs 16384
    python benchmarks/bench_workloads.py gels --m 32768 --n 8192 --nb 512 --nrhs 512
    python benchmarks/bench_workloads.py getrf --n 16384 --nb 512 --nrhs 512
    python benchmarks/bench_workloads.py getrf_incpiv --n 16384 --nb 512 --nrhs 512
    python benchmarks/bench_workloads.py potri --n 16384 --nb 512
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _dist():
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    return world, rank, local


def _comm(pa, world, rank, local, gpu=True):
    if world > 1:
        job = "_".join([os.environ.get("MASTER_PORT", "0"), os.environ.get("TORCHELASTIC_RUN_ID", "wl"), str(os.getppid())])
        if pa.comm_init(rank, world, job, local if gpu else -1) != 0:
            raise RuntimeError("comm_init failed")


def bench_qr(args):
    import torch
    import torch.distributed as dist

    world, rank, local = _dist()
    if args.share_gpu:  # validation mode: every rank on GPU 0, collectives over gloo
        local = 0
    torch.cuda.set_device(local)
    if world > 1:
        if args.share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    import parsec_amd as pa

    pa.require_native()
    pa.mca_set("device_hip_mask", str(1 << local))
    _comm(pa, world, rank, local)
    ctx = pa.init(args.cores)

    def allreduce(v, op=None):  # on the GPU (RCCL) or, sharing one GPU, on host copies (gloo)
        if world == 1:
            return v
        kw = {} if op is None else {"op": op}
        if args.share_gpu:
            c = v.cpu()
            dist.all_reduce(c, **kw)
            v.copy_(c)
        else:
            dist.all_reduce(v, **kw)
        return v
    gpu = pa.first_gpu_device_index()
    N, nb = args.n, args.nb
    # process grid: --qr-grid 1d = P x 1 row-cyclic (the TS chain of a panel
    # crosses every rank), 2d = the most square P x Q (P >= Q), which halves the
    # ranks a panel chain crosses at 8 GPUs and spreads the trailing update
    if args.qr_grid == "2d":
        P = int(world ** 0.5)
        while world % P:
            P -= 1
        P, Q = max(P, world // P), min(P, world // P)
    else:
        P, Q = world, 1
    NT = (N + nb - 1) // nb
    myrow, mycol = rank // Q, rank % Q
    lm = sum(1 for g in range(NT) if g % P == myrow)
    ln = sum(1 for g in range(NT) if g % Q == mycol)
    storeA = torch.empty((ln, lm, nb, nb), dtype=torch.float64, device="cuda")
    storeT = torch.zeros((ln, lm, nb, nb), dtype=torch.float64, device="cuda")
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=P, Q=Q, device=gpu, ptr=storeA.data_ptr())
    T = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=P, Q=Q, device=gpu, ptr=storeT.data_ptr())
    # auto: one process row -> the flat TS tree from the ptgpp-compiled
    # dgeqrf.jdf (what the hierarchical tree reduces to there); several process
    # rows -> the hierarchical tree (TT merges across the rows)
    hqr = args.qr_tree == "hqr" or (args.qr_tree == "auto" and P > 1)
    use_jdf = not hqr and args.taskpool == "jdf"
    if hqr:  # TT-kernel reflectors of the hierarchical tree
        storeTT = torch.zeros((ln, lm, nb, nb), dtype=torch.float64, device="cuda")
        TT = pa.BlockCyclic(pa.MATRIX_DOUBLE, rank, nb, nb, N, N, P=P, Q=Q, device=gpu, ptr=storeTT.data_ptr())
    g = torch.Generator(device="cuda").manual_seed(1234 + rank)
    storeA.copy_(torch.rand(storeA.shape, dtype=torch.float64, device="cuda", generator=g) - 0.5)
    backup = storeA.clone()

    def step():
        storeA.copy_(backup)
        storeT.zero_()
        torch.cuda.synchronize()
        tp = pa.dgeqrf_hqr_new(A, T, TT, args.qr_domain) if hqr else pa.dgeqrf_jdf_new(A, T) if use_jdf else pa.dgeqrf_new(A, T, args.ib)
        ctx.add_taskpool(tp)
        ctx.start()
        ctx.wait()

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        barrier()
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    dt = (time.perf_counter() - t0) / args.steps
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device="cuda")
        allreduce(tt, dist.ReduceOp.MAX)
        dt = float(tt.item())
    check = None
    if args.check:
        # R of the last timed factorization against the input, outside the timed
        # region. Q orthogonal => A^T A = R^T R; probed with a random x from the
        # local tiles and summed over ranks (4 all-reduces of N-vectors):
        # ||A^T (A x) - R^T (R x)|| / (||A||_F^2 ||x||)
        torch.cuda.synchronize()
        gx = torch.Generator(device="cuda").manual_seed(99)
        x = torch.rand(N, dtype=torch.float64, device="cuda", generator=gx) - 0.5
        At, Rt = backup.view(-1, nb, nb), storeA.view(-1, nb, nb)
        loc = [(m, n, A.local_index(m, n)) for n in range(NT) for m in range(NT)]
        loc = [(m, n, li) for (m, n, li) in loc if li >= 0]

        def allsum(v):
            return allreduce(v)

        def blk(t, m, n):
            return t.t()[:min(nb, N - m * nb), :min(nb, N - n * nb)]

        def sl(i):
            return slice(i * nb, min(N, (i + 1) * nb))

        ax, rx = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
        fro = torch.zeros(1, dtype=torch.float64, device="cuda")
        for m, n, li in loc:
            a = blk(At[li], m, n)
            ax[sl(m)] += a @ x[sl(n)]
            fro += (a * a).sum()
            if m <= n:
                r = blk(Rt[li], m, n)
                rx[sl(m)] += (torch.triu(r) if m == n else r) @ x[sl(n)]
        allsum(ax), allsum(rx), allsum(fro)
        ata, rtr = torch.zeros(N, dtype=torch.float64, device="cuda"), torch.zeros(N, dtype=torch.float64, device="cuda")
        for m, n, li in loc:
            ata[sl(n)] += blk(At[li], m, n).t() @ ax[sl(m)]
            if m <= n:
                r = blk(Rt[li], m, n)
                rtr[sl(n)] += (torch.triu(r) if m == n else r).t() @ rx[sl(m)]
        allsum(ata), allsum(rtr)
        check = float(torch.linalg.norm(ata - rtr) / (fro.item() * torch.linalg.norm(x)))
    ctx.fini()
    if world > 1:
        pa.comm_fini()
    out = {"metric": "GFLOP/s tiled DGEQRF (PTG, HBM-resident)", "value": round(4.0 / 3.0 * N ** 3 / dt / 1e9, 1), "unit": "GFLOP/s",
           "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True,
           "dtype": "fp64", "data": "synthetic uniform(-0.5, 0.5)", "config": {"model": "tiled DGEQRF (" + ((f"hierarchical, TS domains of {args.qr_domain}" if args.qr_domain > 0 else "hierarchical, flat TS per process row") + ", TT binary trees" if hqr else "flat TS tree") + (", ptgpp-compiled dgeqrf.jdf" if use_jdf else ", hand-built C++ DAG") + ")", "N": N, "nb": nb, "ib": 32,
                                                                             "parallelism": f"2D block-cyclic P{P}xQ{Q}" if Q > 1 else f"1D row-cyclic P{P}x1"}}
    if check is not None:
        out["residual_AtAx_vs_RtRx"] = check
    if args.share_gpu:
        out["note"] = "validation mode: all ranks share GPU 0; not a scaling measurement"
    if world > 1:
        dist.destroy_process_group()
    return out, rank


def bench_stencil(args):
    world, rank, local = _dist()
    import torch

    dev = 0 if args.share_gpu else local  # --share-gpu: every rank on GPU 0 (halo-path validation, not scaling)
    torch.cuda.set_device(dev)
    import parsec_amd as pa

    pa.require_native()
    pa.mca_set("device_hip_mask", str(1 << dev))
    _comm(pa, world, rank, dev)
    ctx = pa.init(args.cores)
    # grid resident in HBM (the home device of every block and face buffer)
    G = pa.StencilGrid(rank, world, args.n, args.n, args.n, args.b, args.b, args.b, device=pa.first_gpu_device_index())
    pa.stencil3d_run(ctx, G, 2, 0.4, 0.1, True)  # warmup: tiles to HBM, kernels loaded
    secs, pts, _ = pa.stencil3d_run(ctx, G, args.iters, 0.4, 0.1, True)
    if world > 1:
        secs = pa.comm_allreduce_max_f64(secs) if hasattr(pa, "comm_allreduce_max_f64") else secs
    ctx.fini()
    if world > 1:
        pa.comm_fini()
    gpts = pts / secs / 1e9
    out = {"metric": "Gpoint-updates/s DTD 3D 7-point stencil", "value": round(gpts, 2), "unit": "Gpoints/s", "gflops": round(8 * gpts, 1),
           "n_gpus": world, "steps": args.iters, "ms_per_step": round(secs / args.iters * 1e3, 3), "higher_is_better": True, "dtype": "fp64",
           "data": "synthetic smooth field", "config": {"model": "DTD stencil3d", "grid": [args.n] * 3, "block": args.b, "ranks": world}}
    if args.share_gpu:
        out["note"] = f"validation mode: all {world} ranks share GPU 0 (halo faces cross ranks over IPC); not a scaling measurement"
    return out, rank


def bench_dtd_gemm(args):
    import numpy as np

    import parsec_amd as pa

    pa.mca_set("device_hip_enabled", "0")
    ctx = pa.init(args.cores)
    N, nt = args.n, 4
    nb = N // nt
    mats = [pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N) for _ in range(3)]
    rng = np.random.default_rng(0)
    for M in mats:
        for m in range(nt):
            for n in range(nt):
                M.tile(m, n)[:, :] = rng.standard_normal((nb, nb))
    pa.dtd_dgemm(ctx, 1.0, mats[0], mats[1], 1.0, mats[2], False)  # warmup
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pa.dtd_dgemm(ctx, 1.0, mats[0], mats[1], 1.0, mats[2], False)
    dt = (time.perf_counter() - t0) / args.steps
    ctx.fini()
    out = {"metric": "GFLOP/s DTD tiled DGEMM (CPU bodies, 1 process)", "value": round(2.0 * N ** 3 / dt / 1e9, 2), "unit": "GFLOP/s",
           "n_gpus": 0, "steps": args.steps, "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True, "dtype": "fp64",
           "config": {"model": "DTD dgemm", "N": N, "tiles": "4x4", "cores": args.cores}}
    return out, 0


def bench_potrs(args):
    import torch

    import parsec_amd as pa

    world, rank, local = _dist()
    if world > 1:
        raise RuntimeError("potrs: one GPU (the yardstick is a single-device torch.cholesky_solve)")
    if not torch.cuda.is_available():
        raise RuntimeError("potrs: no GPU")
    N, nb, NRHS = args.n, args.nb, args.nrhs
    nbr = args.nbr or min(nb, NRHS)
    dev = torch.device("cuda", 0)
    ctx = pa.init(args.cores)
    gpu = pa.first_gpu_device_index()
    if gpu < 0:
        raise RuntimeError("no GPU device registered in the runtime")
    NT, NTB = -(-N // nb), -(-NRHS // nbr)

    def run(tp):
        ctx.add_taskpool(tp)
        ctx.start()
        ctx.wait()

    def dense_of(store, rows, cols, mb, cb):  # a dense COPY of a tiled store [n][m][col][row]
        return store.permute(1, 3, 0, 2).reshape(store.shape[1] * mb, store.shape[0] * cb)[:rows, :cols].contiguous()

    # SPD input as in bench.py (random symmetric, diagonally dominant), factored once
    sa = torch.zeros((NT, NT, nb, nb), dtype=torch.float64, device=dev)
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N, device=gpu, ptr=sa.data_ptr())
    gen = torch.Generator(device=dev).manual_seed(12345)
    R = torch.rand((N, N), dtype=torch.float64, device=dev, generator=gen) - 0.5
    S = (R + R.t()) * 0.5 + N * torch.eye(N, dtype=torch.float64, device=dev)
    del R
    pad = torch.zeros((NT * nb, NT * nb), dtype=torch.float64, device=dev)
    pad[:N, :N] = S
    sa.copy_(pad.reshape(NT, nb, NT, nb).permute(2, 0, 3, 1))
    del pad
    torch.cuda.synchronize()
    tp, info = pa.dpotrf_jdf_new(A)
    run(tp)
    if pa.read_int(info) != 0:
        raise RuntimeError("dpotrf reported a non-SPD matrix")
    sb = torch.zeros((NTB, NT, nbr, nb), dtype=torch.float64, device=dev)
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS, device=gpu, ptr=sb.data_ptr())
    B0 = torch.rand((N, NRHS), dtype=torch.float64, device=dev, generator=gen) - 0.5
    pad = torch.zeros((NT * nb, NTB * nbr), dtype=torch.float64, device=dev)
    pad[:N, :NRHS] = B0
    backup = pad.reshape(NT, nb, NTB, nbr).permute(2, 0, 3, 1).contiguous()
    del pad
    torch.cuda.synchronize()

    def step():
        sb.copy_(backup)
        torch.cuda.synchronize()
        tp = pa.dpotrs_new(pa.MATRIX_LOWER, A, B)
        run(tp)
        pa.taskpool_free(tp)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    flops = 2.0 * N * N * NRHS
    X = dense_of(sb, N, NRHS, nb, nbr)
    resid = float(torch.linalg.norm(S @ X - B0) / (torch.linalg.norm(S) * torch.linalg.norm(X) + torch.linalg.norm(B0)))
    if not resid < 1e-13:
        raise RuntimeError(f"DPOTRS backward error {resid:.3e} too large")
    # yardstick: the dense factor gathered from the tiles, torch.cholesky_solve
    # (out of place, so it needs no restore), same warm-up and repeats
    L = torch.tril(dense_of(sa, N, N, nb, nb))
    for _ in range(max(1, args.warmup)):
        Y = torch.cholesky_solve(B0, L)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        Y = torch.cholesky_solve(B0, L)
    torch.cuda.synchronize()
    dty = (time.perf_counter() - t0) / args.steps
    diff = float(torch.linalg.norm(X - Y) / torch.linalg.norm(Y))
    ctx.fini()
    out = {"metric": "GFLOP/s DPOTRS (dtrsm_left.jdf, HBM-resident tiles, B restored every step)", "value": round(flops / dt / 1e9, 1), "unit": "GFLOP/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 3), "higher_is_better": True, "dtype": "fp64",
           "backward_error": resid, "yardstick": "torch.cholesky_solve on the dense factor, same process",
           "yardstick_gflops": round(flops / dty / 1e9, 1), "yardstick_ms": round(dty * 1e3, 3), "ratio_to_yardstick": round(dty / dt, 3),
           "rel_diff_to_yardstick": diff,
           "config": {"model": "DPOTRS", "N": N, "nb": nb, "NRHS": NRHS, "nbr": nbr, "cores": args.cores}}
    return out, 0


def bench_gels(args):
    import torch

    import parsec_amd as pa

    world, rank, local = _dist()
    if world > 1:
        raise RuntimeError("gels: one GPU (the yardstick is a single-device torch solve)")
    if not torch.cuda.is_available():
        raise RuntimeError("gels: no GPU")
    M, N, nb, NRHS = args.m, args.n, args.nb, args.nrhs
    if M < N:
        raise RuntimeError("gels: M >= N")
    nbr = args.nbr or min(nb, NRHS)
    dev = torch.device("cuda", 0)
    ctx = pa.init(args.cores)
    gpu = pa.first_gpu_device_index()
    if gpu < 0:
        raise RuntimeError("no GPU device registered in the runtime")
    MT, NT, NTB = -(-M // nb), -(-N // nb), -(-NRHS // nbr)

    def run(tp):
        ctx.add_taskpool(tp)
        ctx.start()
        ctx.wait()

    def tiled(dense, rows, cols, mt, nt, mb, cb):  # the store image [n][m][col][row] of a dense matrix
        pad = torch.zeros((mt * mb, nt * cb), dtype=torch.float64, device=dev)
        pad[:rows, :cols] = dense
        return pad.reshape(mt, mb, nt, cb).permute(2, 0, 3, 1).contiguous()

    def dense_of(store, rows, cols, mb, cb):  # a dense COPY of a tiled store
        return store.permute(1, 3, 0, 2).reshape(store.shape[1] * mb, store.shape[0] * cb)[:rows, :cols].contiguous()

    gen = torch.Generator(device=dev).manual_seed(12345)
    S = torch.rand((M, N), dtype=torch.float64, device=dev, generator=gen) - 0.5
    B0 = torch.rand((M, NRHS), dtype=torch.float64, device=dev, generator=gen) - 0.5
    backupA = tiled(S, M, N, MT, NT, nb, nb)
    backupB = tiled(B0, M, NRHS, MT, NTB, nb, nbr)
    sa = backupA.clone()
    st = torch.zeros_like(sa)
    sb = backupB.clone()
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N, device=gpu, ptr=sa.data_ptr())
    T = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, M, N, device=gpu, ptr=st.data_ptr())
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, M, NRHS, device=gpu, ptr=sb.data_ptr())
    torch.cuda.synchronize()

    def step_gels():
        sa.copy_(backupA)
        st.zero_()
        sb.copy_(backupB)
        torch.cuda.synchronize()
        tp = pa.dgels_new(A, T, B)
        run(tp)
        pa.taskpool_free(tp)

    def step_geqrs():
        sb.copy_(backupB)
        torch.cuda.synchronize()
        tp = pa.dgeqrs_new(A, T, B)
        run(tp)
        pa.taskpool_free(tp)

    def timed(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    def normal_residual():
        X = dense_of(sb, M, NRHS, nb, nbr)[:N]
        nS, nB = torch.linalg.norm(S), torch.linalg.norm(B0)
        return X, float(torch.linalg.norm(S.t() @ (S @ X - B0)) / (nS * nS * torch.linalg.norm(X) + nS * nB))

    # DGELS first: it leaves the factor in A and T for the DGEQRS steps
    dt_gels = timed(step_gels)
    X, resid_gels = normal_residual()
    dt_geqrs = timed(step_geqrs)
    X, resid = normal_residual()
    if not (resid < 1e-13 and resid_gels < 1e-13):
        raise RuntimeError(f"normal-equations residual too large: dgeqrs {resid:.3e}, dgels {resid_gels:.3e}")
    flops_solve = 4.0 * M * N * NRHS - 2.0 * N * N * NRHS + 1.0 * N * N * NRHS
    flops_qr = 2.0 * M * N * N - 2.0 / 3.0 * N ** 3
    # yardstick on the dense data (factor and solve, what DGELS does): lstsq if
    # the device runs it, otherwise QR + triangular solve
    del sa, st, backupA

    def y_lstsq():
        return torch.linalg.lstsq(S, B0).solution

    def y_qr():
        Q, R = torch.linalg.qr(S)
        return torch.linalg.solve_triangular(R, Q.t() @ B0, upper=True)

    yard, yname = y_lstsq, "torch.linalg.lstsq"
    try:
        Y = yard()
        torch.cuda.synchronize()
        if not bool(torch.isfinite(Y).all()):
            raise RuntimeError("non-finite")
    except Exception as e:  # not available on this device / build
        yard, yname = y_qr, f"torch.linalg.qr + solve_triangular (lstsq did not run: {type(e).__name__})"
    for _ in range(max(1, args.warmup)):
        Y = yard()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        Y = yard()
    torch.cuda.synchronize()
    dty = (time.perf_counter() - t0) / args.steps
    diff = float(torch.linalg.norm(X - Y) / torch.linalg.norm(Y))
    ctx.fini()
    out = {"metric": "GFLOP/s DGEQRS (dormqr.jdf + dtrsm_left.jdf, HBM-resident tiles, B restored every step)", "value": round(flops_solve / dt_geqrs / 1e9, 1),
           "unit": "GFLOP/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt_geqrs * 1e3, 3), "higher_is_better": True,
           "dtype": "fp64", "normal_equations_residual": resid,
           "dgels_gflops": round((flops_qr + flops_solve) / dt_gels / 1e9, 1), "dgels_ms": round(dt_gels * 1e3, 3), "dgels_normal_equations_residual": resid_gels,
           "yardstick": yname + " on the dense data (factor and solve), same process",
           "yardstick_gflops": round((flops_qr + flops_solve) / dty / 1e9, 1), "yardstick_ms": round(dty * 1e3, 3), "dgels_ratio_to_yardstick": round(dty / dt_gels, 3),
           "rel_diff_to_yardstick": diff,
           "config": {"model": "DGELS", "M": M, "N": N, "nb": nb, "NRHS": NRHS, "nbr": nbr, "cores": args.cores}}
    return out, 0


def bench_getrf(args):
    import torch

    import parsec_amd as pa

    world, rank, local = _dist()
    if world > 1:
        raise RuntimeError("getrf: one GPU (the yardstick is a single-device torch.linalg.lu_factor)")
    if not torch.cuda.is_available():
        raise RuntimeError("getrf: no GPU")
    N, nb, NRHS = args.n, args.nb, args.nrhs
    nbr = args.nbr or min(nb, NRHS)
    dev = torch.device("cuda", 0)
    ctx = pa.init(args.cores)
    gpu = pa.first_gpu_device_index()
    if gpu < 0:
        raise RuntimeError("no GPU device registered in the runtime")
    NT, NTB = -(-N // nb), -(-NRHS // nbr)

    def run(tp):
        ctx.add_taskpool(tp)
        ctx.start()
        ctx.wait()

    def tiled(dense, rows, cols, mt, nt, mb, cb):  # the store image [n][m][col][row] of a dense matrix
        pad = torch.zeros((mt * mb, nt * cb), dtype=torch.float64, device=dev)
        pad[:rows, :cols] = dense
        return pad.reshape(mt, mb, nt, cb).permute(2, 0, 3, 1).contiguous()

    def dense_of(store, rows, cols, mb, cb):  # a dense COPY of a tiled store
        return store.permute(1, 3, 0, 2).reshape(store.shape[1] * mb, store.shape[0] * cb)[:rows, :cols].contiguous()

    # R standard normal + diag(column sums of |R| + 1): column diagonally dominant,
    # the class of matrices an unpivoted LU is meant for
    gen = torch.Generator(device=dev).manual_seed(12345)
    S = torch.randn((N, N), dtype=torch.float64, device=dev, generator=gen)
    S += torch.diag(S.abs().sum(dim=0) + 1.0)
    B0 = torch.randn((N, NRHS), dtype=torch.float64, device=dev, generator=gen)
    backupA = tiled(S, N, N, NT, NT, nb, nb)
    backupB = tiled(B0, N, NRHS, NT, NTB, nb, nbr)
    sa = backupA.clone()
    sb = backupB.clone()
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N, device=gpu, ptr=sa.data_ptr())
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS, device=gpu, ptr=sb.data_ptr())
    torch.cuda.synchronize()
    infos = []

    def step_getrf():
        sa.copy_(backupA)
        torch.cuda.synchronize()
        tp, info = pa.dgetrf_nopiv_new(A)
        run(tp)
        infos.append(pa.read_int(info))

    def step_gesv():
        sa.copy_(backupA)
        sb.copy_(backupB)
        torch.cuda.synchronize()
        tp, info = pa.dgesv_nopiv_new(A, B)
        run(tp)
        infos.append(pa.read_int(info))
        pa.taskpool_free(tp)

    def timed(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    dt_getrf = timed(step_getrf)
    F = dense_of(sa, N, N, nb, nb)
    L = torch.tril(F, -1)
    L.diagonal().fill_(1.0)
    nS = torch.linalg.norm(S)
    lu_bwd = float(torch.linalg.norm(L @ torch.triu(F) - S) / nS)
    del L, F
    dt_gesv = timed(step_gesv)
    if any(infos):
        raise RuntimeError(f"a zero pivot was reported: info {infos}")
    X = dense_of(sb, N, NRHS, nb, nbr)
    resid = float(torch.linalg.norm(S @ X - B0) / (nS * torch.linalg.norm(X) + torch.linalg.norm(B0)))
    if not (lu_bwd < 1e-13 and resid < 1e-13):
        raise RuntimeError(f"backward error too large: LU {lu_bwd:.3e}, solve {resid:.3e}")
    flops_lu = 2.0 / 3.0 * N ** 3
    flops_sv = flops_lu + 2.0 * N * N * NRHS
    del sa, backupA
    # yardstick on the dense data: torch's LU, which PIVOTS (out of place, no restore needed)
    for _ in range(max(1, args.warmup)):
        LU, piv = torch.linalg.lu_factor(S)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        LU, piv = torch.linalg.lu_factor(S)
    torch.cuda.synchronize()
    dty_lu = (time.perf_counter() - t0) / args.steps
    for _ in range(max(1, args.warmup)):
        Y = torch.linalg.lu_solve(LU, piv, B0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        Y = torch.linalg.lu_solve(LU, piv, B0)
    torch.cuda.synchronize()
    dty_sv = dty_lu + (time.perf_counter() - t0) / args.steps
    swaps = int((piv != torch.arange(1, N + 1, device=dev, dtype=piv.dtype)).sum())
    Lt = torch.tril(LU, -1)
    Lt.diagonal().fill_(1.0)
    torch_bwd = float(torch.linalg.norm(Lt @ torch.triu(LU) - S) / nS) if swaps == 0 else None
    diff = float(torch.linalg.norm(X - Y) / torch.linalg.norm(Y))
    ctx.fini()
    out = {"metric": "GFLOP/s DGETRF_NOPIV (dgetrf_nopiv.jdf, no pivoting, HBM-resident tiles, A restored every step)", "value": round(flops_lu / dt_getrf / 1e9, 1),
           "unit": "GFLOP/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt_getrf * 1e3, 3), "higher_is_better": True,
           "dtype": "fp64", "flops_getrf": flops_lu, "flops_gesv": flops_sv, "lu_backward_error": lu_bwd,
           "dgesv_gflops": round(flops_sv / dt_gesv / 1e9, 1), "dgesv_ms": round(dt_gesv * 1e3, 3), "dgesv_backward_error": resid,
           "yardstick": "torch.linalg.lu_factor / lu_solve on the dense data, same process; torch PIVOTS (partial pivoting), we do not",
           "yardstick_lu_gflops": round(flops_lu / dty_lu / 1e9, 1), "yardstick_lu_ms": round(dty_lu * 1e3, 3),
           "yardstick_solve_gflops": round(flops_sv / dty_sv / 1e9, 1), "yardstick_solve_ms": round(dty_sv * 1e3, 3),
           "yardstick_row_swaps": swaps, "yardstick_lu_backward_error": torch_bwd,
           "ratio_to_yardstick": round(dty_lu / dt_getrf, 3), "dgesv_ratio_to_yardstick": round(dty_sv / dt_gesv, 3), "rel_diff_to_yardstick": diff,
           "config": {"model": "DGETRF_NOPIV", "N": N, "nb": nb, "NRHS": NRHS, "nbr": nbr, "cores": args.cores}}
    return out, 0


def bench_getrf_incpiv(args):
    import torch

    import parsec_amd as pa

    world, rank, local = _dist()
    if world > 1:
        raise RuntimeError("getrf_incpiv: one GPU (the yardstick is a single-device torch.linalg.lu_factor)")
    if not torch.cuda.is_available():
        raise RuntimeError("getrf_incpiv: no GPU")
    N, nb, NRHS = args.n, args.nb, args.nrhs
    nbr = args.nbr or min(nb, NRHS)
    dev = torch.device("cuda", 0)
    ctx = pa.init(args.cores)
    gpu = pa.first_gpu_device_index()
    if gpu < 0:
        raise RuntimeError("no GPU device registered in the runtime")
    NT, NTB = -(-N // nb), -(-NRHS // nbr)

    def run(tp):
        ctx.add_taskpool(tp)
        ctx.start()
        ctx.wait()

    def tiled(dense, rows, cols, mt, nt, mb, cb):  # the store image [n][m][col][row] of a dense matrix
        pad = torch.zeros((mt * mb, nt * cb), dtype=torch.float64, device=dev)
        pad[:rows, :cols] = dense
        return pad.reshape(mt, mb, nt, cb).permute(2, 0, 3, 1).contiguous()

    def dense_of(store, rows, cols, mb, cb):  # a dense COPY of a tiled store
        return store.permute(1, 3, 0, 2).reshape(store.shape[1] * mb, store.shape[0] * cb)[:rows, :cols].contiguous()

    # standard normal: partial pivoting swaps almost every row, an unpivoted LU is unusable
    gen = torch.Generator(device=dev).manual_seed(12345)
    S = torch.randn((N, N), dtype=torch.float64, device=dev, generator=gen)
    B0 = torch.randn((N, NRHS), dtype=torch.float64, device=dev, generator=gen)
    backupA = tiled(S, N, N, NT, NT, nb, nb)
    backupB = tiled(B0, N, NRHS, NT, NTB, nb, nbr)
    sa = backupA.clone()
    sl = torch.zeros_like(sa)
    sb = backupB.clone()
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N, device=gpu, ptr=sa.data_ptr())
    L = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N, device=gpu, ptr=sl.data_ptr())
    B = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nbr, N, NRHS, device=gpu, ptr=sb.data_ptr())
    torch.cuda.synchronize()
    infos = []

    def step_getrf():
        sa.copy_(backupA)
        sl.zero_()
        torch.cuda.synchronize()
        r = pa.dgetrf_incpiv_new(A, L)
        if r is None:
            raise RuntimeError("dgetrf_incpiv_new refused the request")
        run(r[0])
        infos.append(pa.read_int(r[1]))

    def step_gesv():
        sa.copy_(backupA)
        sl.zero_()
        sb.copy_(backupB)
        torch.cuda.synchronize()
        tp, info = pa.dgesv_incpiv_new(A, L, B)
        run(tp)
        infos.append(pa.read_int(info))
        pa.taskpool_free(tp)

    def timed(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    dt_getrf = timed(step_getrf)
    dt_gesv = timed(step_gesv)
    if any(infos):
        raise RuntimeError(f"a zero on U's diagonal was reported: info {infos}")
    nS = torch.linalg.norm(S)

    def residual(X):
        return float(torch.linalg.norm(S @ X - B0) / (nS * torch.linalg.norm(X) + torch.linalg.norm(B0)))

    X = dense_of(sb, N, NRHS, nb, nbr)
    resid = residual(X)
    max_mult = float(torch.tril(dense_of(sa, N, N, nb, nb), -1).abs().max())
    flops_lu = 2.0 / 3.0 * N ** 3
    flops_sv = flops_lu + 2.0 * N * N * NRHS
    # executed: GETRF 2/3, GESSM 1, TSTRF 1, SSSSM 3 (solve with the full L1 + one K = nb GEMM), in nb^3
    pairs = NT * (NT - 1) / 2.0
    exec_lu = (2.0 / 3.0 * NT + 2.0 * pairs + 3.0 * (NT - 1) * NT * (2 * NT - 1) / 6.0) * float(nb) ** 3
    exec_sv = exec_lu + (NT + 3.0 * pairs) * float(nb) ** 2 * NRHS + float(N) * N * NRHS
    del sa, sl, backupA
    # yardstick on the dense data: torch's LU with partial pivoting (out of place, no restore needed)
    for _ in range(max(1, args.warmup)):
        LU, piv = torch.linalg.lu_factor(S)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        LU, piv = torch.linalg.lu_factor(S)
    torch.cuda.synchronize()
    dty_lu = (time.perf_counter() - t0) / args.steps
    for _ in range(max(1, args.warmup)):
        Y = torch.linalg.lu_solve(LU, piv, B0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        Y = torch.linalg.lu_solve(LU, piv, B0)
    torch.cuda.synchronize()
    dty_sv = dty_lu + (time.perf_counter() - t0) / args.steps
    torch_resid = residual(Y)
    # pairwise pivoting loses accuracy with the number of tile rows (both figures are
    # printed); only a result that is no solution at all is an error
    if not resid < 1e-9:
        raise RuntimeError(f"solve residual too large: ours {resid:.3e}, torch {torch_resid:.3e}")
    ctx.fini()
    out = {"metric": "GFLOP/s DGETRF_INCPIV (dgetrf_incpiv.jdf, pairwise pivoting, credited 2/3 N^3, HBM-resident tiles, A and L restored every step)",
           "value": round(flops_lu / dt_getrf / 1e9, 1), "unit": "GFLOP/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(dt_getrf * 1e3, 3), "higher_is_better": True, "dtype": "fp64", "flops_getrf": flops_lu, "flops_gesv": flops_sv,
           "executed_flops_getrf": exec_lu, "executed_flops_gesv": exec_sv, "executed_gflops": round(exec_lu / dt_getrf / 1e9, 1),
           "dgesv_gflops": round(flops_sv / dt_gesv / 1e9, 1), "dgesv_ms": round(dt_gesv * 1e3, 3), "dgesv_residual": resid, "max_multiplier": max_mult,
           "yardstick": "torch.linalg.lu_factor / lu_solve (partial pivoting) on the dense data, same process",
           "yardstick_lu_gflops": round(flops_lu / dty_lu / 1e9, 1), "yardstick_lu_ms": round(dty_lu * 1e3, 3),
           "yardstick_solve_gflops": round(flops_sv / dty_sv / 1e9, 1), "yardstick_solve_ms": round(dty_sv * 1e3, 3), "yardstick_residual": torch_resid,
           "residual_ratio_to_yardstick": round(resid / torch_resid, 2),
           "ratio_to_yardstick": round(dty_lu / dt_getrf, 3), "dgesv_ratio_to_yardstick": round(dty_sv / dt_gesv, 3),
           "config": {"model": "DGETRF_INCPIV", "N": N, "nb": nb, "NRHS": NRHS, "nbr": nbr, "tile_rows": NT, "cores": args.cores}}
    return out, 0


def bench_potri(args):
    import torch

    import parsec_amd as pa

    world, rank, local = _dist()
    if world > 1:
        raise RuntimeError("potri: one GPU (the yardstick is a single-device torch.cholesky_inverse)")
    if not torch.cuda.is_available():
        raise RuntimeError("potri: no GPU")
    N, nb = args.n, args.nb
    dev = torch.device("cuda", 0)
    ctx = pa.init(args.cores)
    gpu = pa.first_gpu_device_index()
    if gpu < 0:
        raise RuntimeError("no GPU device registered in the runtime")
    NT = -(-N // nb)

    def run(tp):
        ctx.add_taskpool(tp)
        ctx.start()
        ctx.wait()

    def tiled(dense):  # the store image [n][m][col][row] of a dense N x N matrix
        pad = torch.zeros((NT * nb, NT * nb), dtype=torch.float64, device=dev)
        pad[:N, :N] = dense
        return pad.reshape(NT, nb, NT, nb).permute(2, 0, 3, 1).contiguous()

    def lower_of(store):  # a dense COPY of the lower triangle of a tiled store
        return torch.tril(store.permute(1, 3, 0, 2).reshape(NT * nb, NT * nb)[:N, :N])

    gen = torch.Generator(device=dev).manual_seed(12345)
    if args.cond > 1.0:
        # Q diag(logspace(0, -log10(cond))) Q^T: a prescribed condition number
        Q, _ = torch.linalg.qr(torch.randn((N, N), dtype=torch.float64, device=dev, generator=gen))
        d = torch.logspace(0.0, -math.log10(args.cond), N, dtype=torch.float64, device=dev)
        S = (Q * d) @ Q.t()
        S = (S + S.t()) / 2
        del Q
    else:
        # (R + R^T) / 2 + N I, R uniform: the well-conditioned family of the tests
        S = torch.rand((N, N), dtype=torch.float64, device=dev, generator=gen)
        S = (S + S.t()) / 2 + N * torch.eye(N, dtype=torch.float64, device=dev)
    Lf = torch.linalg.cholesky(S)  # the dense factor: our input and torch's
    backupS = tiled(S)
    backupL = tiled(Lf)
    sa = backupL.clone()
    A = pa.BlockCyclic(pa.MATRIX_DOUBLE, 0, nb, nb, N, N, device=gpu, ptr=sa.data_ptr())
    torch.cuda.synchronize()
    infos = []

    def step_trtri():
        sa.copy_(backupL)
        torch.cuda.synchronize()
        tp, info = pa.dtrtri_new(pa.MATRIX_LOWER, pa.MATRIX_NONUNIT, A)
        run(tp)
        infos.append(pa.read_int(info))

    def step_potri():
        sa.copy_(backupL)
        torch.cuda.synchronize()
        tp = pa.dpotri_new(pa.MATRIX_LOWER, A)
        run(tp)
        pa.taskpool_free(tp)

    def step_poinv():
        sa.copy_(backupS)
        torch.cuda.synchronize()
        tp, info = pa.dpoinv_new(pa.MATRIX_LOWER, A)
        run(tp)
        infos.append(pa.read_int(info))
        pa.taskpool_free(tp)

    def timed(step):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps

    eye = torch.eye(N, dtype=torch.float64, device=dev)
    nS, nL = torch.linalg.norm(S), torch.linalg.norm(Lf)

    def tri_residual(X):  # ||X L - I||_F / (||X||_F ||L||_F)
        return float(torch.linalg.norm(X @ Lf - eye) / (torch.linalg.norm(X) * nL))

    def inv_residual(X):  # ||A X - I||_F / (||A||_F ||X||_F)
        return float(torch.linalg.norm(S @ X - eye) / (nS * torch.linalg.norm(X)))

    def sym(T):
        return T + torch.tril(T, -1).t()

    dt_trtri = timed(step_trtri)
    res_trtri = tri_residual(lower_of(sa))
    dt_potri = timed(step_potri)
    res_potri = inv_residual(sym(lower_of(sa)))
    dt_poinv = timed(step_poinv)
    res_poinv = inv_residual(sym(lower_of(sa)))
    if any(infos):
        raise RuntimeError(f"a zero diagonal entry / a failed factorization was reported: info {infos}")
    del sa, backupS, backupL
    # yardsticks on the dense factor, same process (out of place, no restore needed)
    for _ in range(max(1, args.warmup)):
        Y = torch.cholesky_inverse(Lf)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        Y = torch.cholesky_inverse(Lf)
    torch.cuda.synchronize()
    dty_potri = (time.perf_counter() - t0) / args.steps
    res_y_potri = inv_residual(Y)
    del Y
    for _ in range(max(1, args.warmup)):
        Y = torch.linalg.solve_triangular(Lf, eye, upper=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        Y = torch.linalg.solve_triangular(Lf, eye, upper=False)
    torch.cuda.synchronize()
    dty_trtri = (time.perf_counter() - t0) / args.steps
    res_y_trtri = tri_residual(Y)
    ctx.fini()
    f_trtri, f_potri, f_poinv = N ** 3 / 3.0, 2.0 * N ** 3 / 3.0, float(N) ** 3
    print(f"residual ||A X - I||_F / (||A||_F ||X||_F): DPOTRI {res_potri:.3e}, DPOINV {res_poinv:.3e}, torch.cholesky_inverse {res_y_potri:.3e}; "
          f"||X L - I||_F / (||X||_F ||L||_F): DTRTRI {res_trtri:.3e}, torch.linalg.solve_triangular {res_y_trtri:.3e}", flush=True)
    out = {"metric": "GFLOP/s DPOTRI (dtrtri_L.jdf + dlauum_L.jdf on the dense factor, HBM-resident tiles, A restored every step)",
           "value": round(f_potri / dt_potri / 1e9, 1), "unit": "GFLOP/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": round(dt_potri * 1e3, 3), "higher_is_better": True, "dtype": "fp64",
           "flops_dtrtri": f_trtri, "flops_dpotri": f_potri, "flops_dpoinv": f_poinv,
           "dtrtri_gflops": round(f_trtri / dt_trtri / 1e9, 1), "dtrtri_ms": round(dt_trtri * 1e3, 3), "dtrtri_residual": res_trtri,
           "dpotri_residual": res_potri,
           "dpoinv_gflops": round(f_poinv / dt_poinv / 1e9, 1), "dpoinv_ms": round(dt_poinv * 1e3, 3), "dpoinv_residual": res_poinv,
           "yardstick": "torch.cholesky_inverse (and torch.linalg.solve_triangular against I for DTRTRI) on the dense factor, same process",
           "yardstick_potri_gflops": round(f_potri / dty_potri / 1e9, 1), "yardstick_potri_ms": round(dty_potri * 1e3, 3), "yardstick_potri_residual": res_y_potri,
           "yardstick_trtri_ms": round(dty_trtri * 1e3, 3), "yardstick_trtri_residual": res_y_trtri,
           "ratio_to_yardstick": round(dty_potri / dt_potri, 3), "dtrtri_ratio_to_yardstick": round(dty_trtri / dt_trtri, 3),
           "dpotri_residual_ratio": round(res_potri / res_y_potri, 2), "dtrtri_residual_ratio": round(res_trtri / res_y_trtri, 2),
           "config": {"model": "DPOTRI", "N": N, "nb": nb, "cond": args.cond, "cores": args.cores}}
    return out, 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("workload", choices=["qr", "stencil", "dtd_gemm", "potrs", "gels", "getrf", "getrf_incpiv", "potri"])
    ap.add_argument("--n", "--size", dest="n", type=int, default=None, help="matrix order (use --size under torchrun)")
    ap.add_argument("--m", type=int, default=None, help="gels: rows of A (default: n)")
    ap.add_argument("--nb", type=int, default=512)
    ap.add_argument("--ib", type=int, default=32, help="qr: accepted for the reference's command line; both taskpools factor 32-column sub-panels (qr_sub2c) and apply one nb x nb block reflector per tile")
    ap.add_argument("--nrhs", type=int, default=None, help="potrs / gels / getrf: right-hand sides (default: n)")
    ap.add_argument("--nbr", type=int, default=0, help="potrs / gels / getrf: tile width of B (default: min(nb, nrhs))")
    ap.add_argument("--cond", type=float, default=0.0, help="potri: condition number of the matrix, Q diag(logspace) Q^T (default 0: the well-conditioned (R + R^T) / 2 + N I)")
    ap.add_argument("--b", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cores", type=int, default=4)
    ap.add_argument("--qr-grid", choices=["1d", "2d"], default="2d", help="qr: process grid over the ranks")
    ap.add_argument("--share-gpu", action="store_true", help="qr / stencil: validation mode, every rank on GPU 0; not a scaling measurement")
    ap.add_argument("--check", action="store_true", help="qr: verify R (||A^T A x - R^T R x|| / (||A||_F^2 ||x||), all ranks) after the timed steps")
    ap.add_argument("--qr-tree", choices=["auto", "hqr", "flat"], default="auto", help="qr: hierarchical (TS domains + TT trees), flat TS tree, or auto (flat on one process row, hierarchical otherwise)")
    ap.add_argument("--taskpool", choices=["jdf", "ir"], default="jdf", help="qr flat tree: the ptgpp-compiled dgeqrf.jdf (default) or the hand-built C++ DAG (dgeqrf.cpp)")
    ap.add_argument("--qr-domain", type=int, default=0,
                    help="qr: rows per TS domain of the hierarchical tree (0: one flat TS chain per process row, TT binary tree across process rows; 1 GPU measured fastest flat: profiles/r3_qr_tree_ab.jsonl)")
    args = ap.parse_args()
    if args.n is None:
        args.n = {"qr": 16384, "stencil": 512, "dtd_gemm": 2048, "potrs": 16384, "gels": 16384, "getrf": 16384, "getrf_incpiv": 16384, "potri": 16384}[args.workload]
    if args.nrhs is None:
        args.nrhs = args.n
    if args.m is None:
        args.m = args.n
    fn = {"qr": bench_qr, "stencil": bench_stencil, "dtd_gemm": bench_dtd_gemm, "potrs": bench_potrs, "gels": bench_gels, "getrf": bench_getrf, "getrf_incpiv": bench_getrf_incpiv, "potri": bench_potri}[args.workload]
    out, rank = fn(args)
    if rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
