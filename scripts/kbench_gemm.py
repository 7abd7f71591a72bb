"""Grouped fp64 GEMM throughput: the DPOTRF trailing-update shape (C -= A B^T on
nb x nb tiles) and one large square GEMM. PARSEC_GEMM_FULL=0 (read once per
process) times the bounds-checked kernel, PARSEC_GEMM_PAD_TEST=1 the padded
one-workgroup-per-CU launch of a DPOTRF bulk stream. (The kernel variants
PARSEC_GEMM_VARIANT once selected are gone; d5f2999 is the last commit that
has them.)

--ab: the three k loops (plain = pa.kernel_gemm_mainloop 0; rotated with the
compiler-scheduled body = mainloop 1, pa.kernel_gemm_pipeline 0; rotated with the
pinned body = mainloop 1, pipeline 1) timed alternately in this process on the
same operands, ROUNDS rounds each; prints the median and best rate of each loop
and whether their outputs are bit-equal."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import parsec_amd as pa  # noqa: E402

ROUNDS = 5
MODES = ("plain", "rotated", "pinned")
KNOBS = {"plain": (0, 0), "rotated": (1, 0), "pinned": (1, 1)}  # (kernel_gemm_mainloop, kernel_gemm_pipeline)


def select(mode):
    pa.kernel_gemm_mainloop(KNOBS[mode][0])
    pa.kernel_gemm_pipeline(KNOBS[mode][1])


def timeit(fn, reps=10):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps


def ab(label, fn, outs, flops, reps):
    """fn() under the three loops: bit-equality of outs from equal inputs, then alternating timing rounds"""
    init = [o.clone() for o in outs]
    res = []
    for mode in MODES:
        for o, i in zip(outs, init):
            o.copy_(i)
        select(mode)
        fn()
        torch.cuda.synchronize()
        res.append([o.clone() for o in outs])
    equal = all(torch.equal(x, y) for r in res[1:] for x, y in zip(res[0], r))
    del res, init
    rates = {m: [] for m in MODES}
    for _ in range(ROUNDS):
        for mode in MODES:
            select(mode)
            rates[mode].append(flops / timeit(fn, reps) / 1e12)
    med = {m: statistics.median(r) for m, r in rates.items()}
    cols = " | ".join(f"{m} median {med[m]:6.2f} best {max(rates[m]):6.2f} TF ({100.0 * (med[m] / med[MODES[0]] - 1.0):+5.2f} %)" for m in MODES)
    print(f"{label}: {cols} | bit-equal {equal}", flush=True)
    return equal


def main():
    dev = torch.device("cuda", 0)
    s = torch.cuda.current_stream().cuda_stream
    do_ab = "--ab" in sys.argv[1:]
    tag = f"full={os.environ.get('PARSEC_GEMM_FULL', '1')} pad={os.environ.get('PARSEC_GEMM_PAD_TEST', '0')}"
    prev, prev_pipe = pa.kernel_gemm_mainloop(-1), pa.kernel_gemm_pipeline(-1)
    all_equal = True
    for nb, ntask in ((512, 32), (1024, 16), (1024, 40)):
        A = [torch.randn(nb, nb, dtype=torch.float64, device=dev) for _ in range(8)]
        C = [torch.randn(nb, nb, dtype=torch.float64, device=dev) for _ in range(ntask)]
        C0 = [c.clone() for c in C]
        descs = [(A[i % 8].data_ptr(), A[(i + 1) % 8].data_ptr(), C[i].data_ptr(), nb, nb, nb, nb, nb, nb, -1.0, 1.0, 1, 0) for i in range(ntask)]
        pa.kernel_dgemm_batch(descs, s)
        torch.cuda.synchronize()
        err = max(float((C[i] - (C0[i] - A[(i + 1) % 8].t() @ A[i % 8])).abs().max()) for i in range(ntask))  # column-major view
        fl = 2.0 * nb ** 3 * ntask
        if do_ab:
            all_equal &= ab(f"{tag} gemm nb={nb} tasks={ntask} maxerr={err:.2e}", lambda: pa.kernel_dgemm_batch(descs, s), C, fl, 10)
            continue
        dt = timeit(lambda: pa.kernel_dgemm_batch(descs, s))
        print(f"{tag} gemm nb={nb} tasks={ntask}: {fl / dt / 1e12:6.1f} TF ({dt * 1e6:8.1f} us) maxerr={err:.2e}", flush=True)
    n = 8192
    A = torch.randn(n, n, dtype=torch.float64, device=dev)
    B = torch.randn(n, n, dtype=torch.float64, device=dev)
    C = torch.zeros(n, n, dtype=torch.float64, device=dev)
    big = lambda: pa.kernel_dgemm(A.data_ptr(), B.data_ptr(), C.data_ptr(), n, n, n, n, n, n, 1.0, 0.0, 1, 0, s)  # noqa: E731
    if do_ab:
        all_equal &= ab(f"{tag} gemm n={n}", big, [C], 2.0 * n ** 3, 3)
        pa.kernel_gemm_mainloop(prev)
        pa.kernel_gemm_pipeline(prev_pipe)
        print(f"{tag} outputs bit-equal between the loops: {all_equal}", flush=True)
        return 0 if all_equal else 1
    dt = timeit(big, 3)
    print(f"{tag} gemm n={n}: {2 * n ** 3 / dt / 1e12:6.1f} TF", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
