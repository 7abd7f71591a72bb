"""The yardstick of the DGETRF_INCPIV tests: an independent model of tile LU with
incremental (pairwise) pivoting, written with torch on the CPU, and the checks
the CPU and GPU test files share. It is never the code under test.

torch.linalg.lu_factor_ex (which does not raise on a zero pivot) factors the
diagonal tile and each stacked pair [U(k,k); A(m,k)]; the pivots are applied
sequentially; solve_triangular and matmul do the rest. The model carries a
right-hand side through the factorization and finishes with the solve with U.

Tolerances (the project's convention, 4 times the yardstick's own error):
  * a tile or a pair: ||P S - L U||_F / ||S||_F of ours <= 4 x that of
    torch.linalg.lu_factor_ex on the same S;
  * a solve: ||A X - B||_F / (||A||_F ||X||_F + ||B||_F) of ours <= 4 x the
    model's, and as a condition on the inputs the model's is itself <= 8 x
    torch.linalg.solve's (1.6 - 4.0 on standard normal A and B at the shapes used).
"""
import numpy as np
import torch


def normal(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(rows, cols, dtype=torch.float64, generator=g)


def apply_pivots(C, piv):
    """LAPACK row interchanges, in sequence: row j <-> row piv[j] - 1 (piv 1-based)."""
    for j, p in enumerate(piv.tolist()):
        p -= 1
        if p != j:
            C[[j, p], :] = C[[p, j], :]
    return C


def _unit_lower_solve(Lm, C):
    L1 = torch.tril(Lm, -1) + torch.eye(Lm.shape[0], dtype=Lm.dtype)
    return torch.linalg.solve_triangular(L1, C, upper=False, unitriangular=True)


def model_solve(S, B, nb):
    """X of S X = B by tile LU with pairwise pivoting; also the factored A."""
    A, B = S.clone(), B.clone()
    N = A.shape[0]
    NT = (N + nb - 1) // nb
    sl = [slice(k * nb, min(N, (k + 1) * nb)) for k in range(NT)]
    for k in range(NT):
        LU, piv, _ = torch.linalg.lu_factor_ex(A[sl[k], sl[k]])
        A[sl[k], sl[k]] = LU
        right = slice(sl[k].stop, N)
        for C in (A[sl[k], right], B[sl[k], :]):
            C[:] = _unit_lower_solve(LU, apply_pivots(C.clone(), piv))
        for m in range(k + 1, NT):
            top = A[sl[k], sl[k]]
            n1 = top.shape[0]
            LU2, piv2, _ = torch.linalg.lu_factor_ex(torch.cat([torch.triu(top), A[sl[m], sl[k]]]))
            A[sl[k], sl[k]] = torch.tril(top, -1) + torch.triu(LU2[:n1])
            L2 = LU2[n1:].clone()
            A[sl[m], sl[k]] = L2
            for M, cols in ((A, right), (B, slice(None))):
                C = apply_pivots(torch.cat([M[sl[k], cols], M[sl[m], cols]]), piv2[:n1])
                C1 = _unit_lower_solve(LU2[:n1], C[:n1])
                M[sl[k], cols] = C1
                M[sl[m], cols] = C[n1:] - L2 @ C1
    X = torch.linalg.solve_triangular(torch.triu(A), B, upper=True)
    return X, A


def residual(S, X, B):
    S, X, B = (torch.as_tensor(np.ascontiguousarray(t)) if not torch.is_tensor(t) else t for t in (S, X, B))
    return float(torch.linalg.norm(S @ X - B) / (torch.linalg.norm(S) * torch.linalg.norm(X) + torch.linalg.norm(B)))


_problems = {}


def problem(N, nb, NRHS, seed=11, zero_diag=False):
    """(S, B, model residual, torch.linalg.solve residual) as numpy / floats, computed once."""
    key = (N, nb, NRHS, seed, zero_diag)
    if key not in _problems:
        S = normal(N, N, seed)
        if zero_diag:
            S.fill_diagonal_(0.0)
        B = normal(N, NRHS, seed + 1000)
        X, _ = model_solve(S, B, nb)
        res_model = residual(S, X, B)
        res_torch = residual(S, torch.linalg.solve(S, B), B)
        _problems[key] = (S.numpy().copy(), B.numpy().copy(), res_model, res_torch)
    return _problems[key]


def check_solution(S, X, B, res_model, res_torch, what=""):
    res = residual(S, X, B)
    print(f"{what}: residual ours {res:.3e}, model {res_model:.3e}, torch.linalg.solve {res_torch:.3e} "
          f"(ours / model {res / res_model:.2f}, model / torch {res_model / res_torch:.2f})")
    assert res_model <= 8 * res_torch, "the input is outside the range the tolerance was derived for"
    assert res <= 4 * res_model


def pair_backward_error(S, top_out, bot_out, Lstrict, piv):
    """||P S - [L1; L2] U||_F / ||S||_F from the outputs of a tile / pair factorization:
    top_out's upper triangle is U, Lstrict's strict lower triangle L1, bot_out L2 (or None)."""
    S = torch.as_tensor(np.ascontiguousarray(S))
    n = S.shape[1]
    U = torch.triu(torch.as_tensor(np.ascontiguousarray(top_out)))
    L1 = torch.tril(torch.as_tensor(np.ascontiguousarray(Lstrict)), -1) + torch.eye(n, dtype=torch.float64)
    Lfull = L1 if bot_out is None else torch.cat([L1, torch.as_tensor(np.ascontiguousarray(bot_out))])
    PS = apply_pivots(S.clone(), torch.as_tensor(np.asarray(piv, dtype=np.int64)))
    return float(torch.linalg.norm(PS - Lfull @ U) / torch.linalg.norm(S))


def torch_backward_error(S):
    """The same figure for torch.linalg.lu_factor_ex on S (rows >= columns)."""
    S = torch.as_tensor(np.ascontiguousarray(S))
    n = S.shape[1]
    LU, piv, _ = torch.linalg.lu_factor_ex(S)
    Lfull = torch.tril(LU, -1)
    Lfull[:n] += torch.eye(n, dtype=torch.float64)
    PS = apply_pivots(S.clone(), piv)
    return float(torch.linalg.norm(PS - Lfull @ torch.triu(LU[:n])) / torch.linalg.norm(S))


def fill(M, D, mb, nb):
    for m in range(M.mt):
        for n in range(M.nt):
            blk = D[m * mb:(m + 1) * mb, n * nb:(n + 1) * nb]
            t = M.tile(m, n)
            t[:, :] = 0.0
            t[:blk.shape[0], :blk.shape[1]] = blk


def fill_garbage(M, value=np.nan):
    """L's contents on entry must not matter."""
    for m in range(M.mt):
        for n in range(M.nt):
            M.tile(m, n)[:, :] = value


def gather(M, rows, cols, mb, nb):
    out = np.zeros((rows, cols))
    for m in range(M.mt):
        for n in range(M.nt):
            r, c = min(mb, rows - m * mb), min(nb, cols - n * nb)
            out[m * mb:m * mb + r, n * nb:n * nb + c] = M.tile(m, n)[:r, :c]
    return out


def check_factor_format(A, L, N, nb):
    """|l| <= 1 for every stored multiplier, pivots in range, nothing inf / nan."""
    NT = (N + nb - 1) // nb
    rows = [min(nb, N - k * nb) for k in range(NT)]
    for k in range(NT):
        for m in range(k, NT):
            a = np.array(A.tile(m, k))[:rows[m], :rows[k]]
            l = np.array(L.tile(m, k))
            lo = np.tril(l[:rows[k], :rows[k]], -1)
            assert np.isfinite(a).all() and np.isfinite(lo).all(), (m, k)
            assert np.abs(lo).max(initial=0.0) <= 1.0, ("L", m, k)
            mult = np.tril(a, -1) if m == k else a
            assert np.abs(mult).max(initial=0.0) <= 1.0, ("A", m, k)
            piv = l[:rows[k], nb - 1]
            j = np.arange(rows[k])
            hi = rows[k] if m == k else rows[k] + rows[m]
            assert (piv == np.round(piv)).all() and (piv >= j + 1).all() and (piv <= hi).all(), ("piv", m, k, piv)
    for m in range(NT):
        for n in range(m + 1, NT):
            assert np.isfinite(np.array(A.tile(m, n))[:rows[m], :rows[n]]).all(), (m, n)
