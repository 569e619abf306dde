"""Inputs, acceptance and the multi-rank worker of the El::LU tests (CPU over
gloo, GPU host-staged or RCCL); see _dist_workers."""
from __future__ import annotations

import traceback

import numpy as np

from _dist_workers import _bits, init, finish

TINY = np.finfo(np.float64).tiny


def apply_swaps(B, piv):
    """The rows of B after the swap sequence piv (row j <-> row piv[j], in order)."""
    B = np.array(B, copy=True)
    for j, p in enumerate(piv):
        if p != j:
            B[[j, p]] = B[[p, j]]
    return B


def explicit(piv, m):
    """v with (P B)[i] = B[v[i]]."""
    return apply_swaps(np.arange(m), piv)


def split_lu(LU):
    """(L, U) in float64 from the packed factors: L m x k unit lower, U k x n upper."""
    m, n = LU.shape
    k = min(m, n)
    F = LU.astype(np.float64)
    return np.tril(F[:, :k], -1) + np.eye(m, k), np.triu(F[:k, :])


def accept(A, LU, piv):
    """The acceptance every case shares.  A: what went in (in the type); LU: the
    packed factors that came out; piv: the swap sequence.  Returns (None or what
    went wrong, the residual over max(m, n) eps ||A||_F).
      * piv is a valid swap sequence, j <= piv[j] < m;
      * every entry is finite;
      * max |L| <= 1 exactly: each multiplier is a quotient by its column's largest entry;
      * ||P A - L U||_F <= 10 max(m, n) eps ||A||_F in float64, the project's Cholesky
        bound: LAPACK (torch.linalg.lu_factor) stays at or below 0.061 of the bare
        max(m, n) eps ||A||_F on uniform [-1, 1] inputs of these shapes in both
        types, and an indexing error costs O(1) / eps."""
    m, n = A.shape
    k = min(m, n)
    eps = np.finfo(A.dtype).eps
    piv = np.asarray(piv)
    if piv.shape != (k,):
        return f"{piv.shape} pivots for {m} x {n}", np.inf
    if not all(j <= piv[j] < m for j in range(k)):
        return f"not a swap sequence: {piv.tolist()}", np.inf
    if not np.isfinite(LU).all():
        return "not finite", np.inf
    lmax = np.abs(np.tril(LU[:, :k], -1)).max(initial=0.0)
    if lmax > 1:
        return f"max |L| = {lmax!r} > 1", np.inf
    L, U = split_lu(LU)
    A64 = A.astype(np.float64)
    ratio = np.linalg.norm(apply_swaps(A64, piv) - L @ U) / max(max(m, n) * eps * np.linalg.norm(A64), TINY)
    print(f"lu residual {m}x{n} {A.dtype}: {ratio:.3g} of max(m,n) eps ||A||_F")
    return (None if ratio <= 10 else f"residual {ratio:.3g} > 10 max(m,n) eps ||A||_F"), ratio


def random_matrix(m, n, seed, npdt):
    import oracle
    return np.asfortranarray(oracle.hash_matrix(m, n, seed, 0.0, 1.0, npdt))


def forced_perm(m, k, first):
    """A permutation of range(m) that starts with `first` (pivot row of column j =
    first[j], j < len(first)) and continues with the remaining rows, largest first."""
    first = [int(r) for r in first][:k]
    assert len(set(first)) == len(first) and all(0 <= r < m for r in first), first
    rest = [r for r in range(m - 1, -1, -1) if r not in set(first)]
    return np.array(first + rest, dtype=np.int64)


def far_rows(m, k):
    """k distinct pivot rows: m - 1, m - 4, m - 7, ... (wrapping), except that column 2
    keeps row 2 (no swap at that step)."""
    out, seen, x = [], set(), m - 1
    for j in range(k):
        if j == 2 and m > 2:
            want = 2
        else:
            want, x = x, (x - 3) % m
        while want in seen:
            want = (want + 1) % m
        seen.add(want)
        out.append(want)
    return out


def forced_input(m, n, perm, seed, npdt):
    """A with A[perm] = L0 U0: L0 unit lower with strict-lower entries in {-1/2, 0,
    1/2}, U0 integer in [-2, 2] with diagonal in +-{1, 2, 4}.  Every entry is exact
    in f32 and f64 and column j's pivot, row perm[j], is unique by a factor of 2."""
    k = min(m, n)
    rng = np.random.default_rng(seed)
    L0 = np.tril(rng.integers(-1, 2, (m, k)) * 0.5, -1) + np.eye(m, k)
    U0 = np.triu(rng.integers(-2, 3, (k, n)).astype(np.float64), 1)
    U0[np.arange(k), np.arange(k)] = rng.choice([1.0, 2.0, 4.0], k) * rng.choice([-1.0, 1.0], k)
    A = np.zeros((m, n))
    A[perm] = L0 @ U0
    return np.asfortranarray(A.astype(npdt)), L0, U0


def check_forced(A, LU, piv, perm, L0, U0):
    """The shared acceptance, then: the first min(m, n) rows of the returned
    permutation are perm's exactly; U = U0 and L's rows, in the order the returned
    permutation gives, = L0's, both within the acceptance bound."""
    why, _ = accept(A, LU, piv)
    if why:
        return why
    m, n = A.shape
    k = min(m, n)
    v = explicit(piv, m)
    if not np.array_equal(v[:k], perm[:k]):
        return f"pivot rows {v[:k].tolist()} != {perm[:k].tolist()}"
    bound = 10 * max(m, n) * np.finfo(A.dtype).eps * np.linalg.norm(A.astype(np.float64))
    L, U = split_lu(LU)
    inv = np.empty(m, dtype=np.int64)
    inv[perm] = np.arange(m)
    eu, el_ = np.linalg.norm(U - U0), np.linalg.norm(L - L0[inv[v]])
    print(f"forced {m}x{n} {A.dtype}: ||U-U0|| = {eu:.3g}, ||L-L0|| = {el_:.3g}, bound {bound:.3g}")
    if eu > bound:
        return f"||U - U0||_F = {eu:.3g} > {bound:.3g}"
    if el_ > bound:
        return f"||L - L0||_F = {el_:.3g} > {bound:.3g}"
    return None


def nan_rule_reference(A):
    """Partial pivoting in float64 under the documented rule: the largest |value|
    pivots, the first of equals, and a NaN never beats a number; a column with
    nothing but zeros and NaNs left is a zero pivot.  Returns (the original rows
    chosen, U or None, the 0-based column of a zero pivot or None)."""
    W = A.astype(np.float64).copy()
    m, n = W.shape
    k = min(m, n)
    orig = np.arange(m)
    with np.errstate(invalid="ignore"):
        for j in range(k):
            col = np.abs(W[j:, j])
            cand = np.where(np.isnan(col), -1.0, col)
            if not cand.max() > 0:
                return orig[:j], None, j
            p = j + int(np.argmax(cand))
            W[[j, p]], orig[[j, p]] = W[[p, j]], orig[[p, j]]
            W[j + 1:, j] /= W[j, j]
            W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], W[j, j + 1:])
    return orig[:k], np.triu(W[:k]), None


def check_nan_rule(A, LU, piv):
    """A holds NaNs but every column keeps numbers: the rows chosen are the
    reference's exactly (so each pivot is the largest number of its column), U is
    finite and the reference's within the acceptance bound, and no finite
    multiplier exceeds 1."""
    m, n = A.shape
    k = min(m, n)
    rows, U, zero = nan_rule_reference(A)
    assert zero is None
    piv = np.asarray(piv)
    if piv.shape != (k,) or not all(j <= piv[j] < m for j in range(k)):
        return f"not a swap sequence: {piv.tolist()}"
    got = explicit(piv, m)[:k]
    if not np.array_equal(got, rows):
        return f"pivot rows {got.tolist()} != {rows.tolist()}"
    Ug = np.triu(LU[:k].astype(np.float64))
    if not np.isfinite(Ug).all():
        return "U is not finite"
    bound = 10 * max(m, n) * np.finfo(A.dtype).eps * np.linalg.norm(np.nan_to_num(A.astype(np.float64)))
    if np.linalg.norm(Ug - U) > bound:
        return f"||U - U_ref||_F = {np.linalg.norm(Ug - U):.3g} > {bound:.3g}"
    Lg = np.abs(np.tril(LU[:, :k], -1))
    if (Lg[np.isfinite(Lg)] > 1).any():
        return "a finite multiplier exceeds 1"
    return None


def nan_inputs(m, n, seed, npdt, R):
    """(A with NaNs in rows that are lane 0 of a wave / thread 0 of a workgroup of
    the GPU leaf, where a NaN entering the reduction would hide the numbers after
    it; the same A with column 1 all zeros and NaNs)."""
    A = random_matrix(m, n, seed, npdt)
    for (i, j) in ((0, 0), (R, 0), (128, 1), (64, 2)):
        if i < m and j < n:
            A[i, j] = np.nan
    Z = A.copy()
    if n > 1:
        Z[:, 1] = 0
        Z[0, 1] = np.nan
        if R < m:
            Z[R, 1] = np.nan
    return A, Z


def solve_bound(A, Y, npdt):
    """The reference's own threshold (tests/lapack_like/LU.cpp:45-53):
    ||Y - A X||_oo <= 100 eps max(m, n) max(||A||_1, ||Y||_1)."""
    A64, Y64 = A.astype(np.float64), Y.astype(np.float64)
    return 100 * np.finfo(npdt).eps * max(A.shape) * max(np.abs(A64).sum(axis=0).max(), np.abs(Y64).sum(axis=0).max())


def oo_norm(E):
    return np.abs(E).sum(axis=1).max() if E.size else 0.0


def payload_matrix(m, n, seed, npdt):
    """Random entries with -0.0, +0.0, infinities and NaNs of distinct payloads."""
    B = random_matrix(m, n, seed, npdt)
    bits = _bits(B).reshape(-1).copy()
    rng = np.random.default_rng(seed)
    w = B.dtype.itemsize * 8
    sign, quiet = 1 << (w - 1), (0x7ff8 << 48) if w == 64 else (0x7fc0 << 16)
    idx = rng.permutation(bits.size)[: max(4, bits.size // 5)]
    for t, i in enumerate(idx):
        bits[i] = (sign, 0, quiet | (t + 1), quiet | sign | (3 * t + 5))[t % 4]
    return np.asfortranarray(bits.view(npdt).reshape(m, n))


def full_matrix(el, D):
    """Every rank's copy of the whole matrix ([*,*] <- D)."""
    S = D.like(el.STAR, el.STAR)
    S.assign(D)
    return S.get_local()


def lu_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, shapes, nb: int, seed: int):
    """El::LU on [MC,MR] matrices: random inputs through `accept`, forced-pivot
    inputs whose pivot rows are owned by other process rows than their
    destinations, a zero column and a matrix that turns singular during the
    elimination (SingularMatrixError on every rank, naming the column), and a valid
    factorization afterwards; DistPermutation::PermuteRows and its inverse,
    bit-exact against numpy, on [MC,MR] and on another distribution."""
    import oracle
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        r, c = g.height, g.width
        npdt = np.float64 if dtype == el.F64 else np.float32
        el.SetBlocksize(nb)

        def dist(A, U=el.MC, V=el.MR):
            D = el.DistMatrix(g, dtype, U, V, device, height=A.shape[0], width=A.shape[1])
            D.set_local(oracle.local_block(A, U, V, r, c, g.vc_rank))
            return D

        def factor(A):
            D = dist(A)
            P = el.LU(D)
            return full_matrix(el, D), P.swap_dests(), P

        for (m, n) in shapes:
            k = min(m, n)
            A = random_matrix(m, n, seed + m + 3 * n, npdt)
            LU, piv, P = factor(A)
            why, _ = accept(A, LU, piv)
            assert why is None, f"{m}x{n} grid {r}x{c} rank {rank}: {why}"
            assert P.Height() == m

            # pivot rows from the far end, so (m > r) they sit on other process rows
            # than their destinations: the last row first, and column 2 keeps row 2
            perm = forced_perm(m, k, far_rows(m, k))
            Af, L0, U0 = forced_input(m, n, perm, seed + 1, npdt)
            LU, piv, _ = factor(Af)
            why = check_forced(Af, LU, piv, perm, L0, U0)
            assert why is None, f"forced {m}x{n} grid {r}x{c} rank {rank}: {why}"

            # bit-exact row permutation with the pivots just computed
            B0 = payload_matrix(m, 7, seed + 2, npdt)
            want = B0[explicit(piv, m)]
            for (U, V) in ((el.MC, el.MR), (el.VC, el.STAR)):
                B = dist(B0, U, V)
                P2 = el.LU(dist(Af))
                P2.PermuteRows(B)
                got = full_matrix(el, B)
                assert np.array_equal(_bits(got), _bits(want)), f"PermuteRows {m} [{U},{V}] rank {rank}"
                P2.InversePermuteRows(B)
                assert np.array_equal(_bits(full_matrix(el, B)), _bits(B0)), f"InversePermuteRows {m} rank {rank}"

            if m == n:
                for col in (0, min(nb, n - 1), n - 1):
                    Az = A.copy()
                    Az[:, col] = 0
                    try:
                        factor(Az)
                    except el.SingularMatrixError as e:
                        assert str(e).endswith(f"column {col + 1}"), (col, str(e))
                    else:
                        raise AssertionError(f"zero column {col}, rank {rank}: no SingularMatrixError")
                Ad = Af.copy()
                Ad[perm[k - 1]] = Ad[perm[0]]  # two equal rows: the last pivot is exactly zero
                try:
                    factor(Ad)
                except el.SingularMatrixError as e:
                    assert str(e).endswith(f"column {n}"), str(e)
                else:
                    raise AssertionError(f"equal rows, rank {rank}: no SingularMatrixError")
                LU, piv, _ = factor(A)
                assert accept(A, LU, piv)[0] is None
        finish()
    except Exception:
        traceback.print_exc()
        raise


def solve_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, n: int, nrhs: int, nb: int,
                 seed: int):
    """LU + LUSolveAfter NORMAL / TRANSPOSE and LinearSolve within the reference's bound."""
    import oracle
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        r, c = g.height, g.width
        npdt = np.float64 if dtype == el.F64 else np.float32
        el.SetBlocksize(nb)
        check_solves(el, g, device, dtype, n, nrhs, seed,
                     lambda A, U=el.MC, V=el.MR: _dist(el, oracle, g, r, c, dtype, device, A, U, V))
        finish()
    except Exception:
        traceback.print_exc()
        raise


def _dist(el, oracle, g, r, c, dtype, device, A, U, V):
    D = el.DistMatrix(g, dtype, U, V, device, height=A.shape[0], width=A.shape[1])
    D.set_local(oracle.local_block(A, U, V, r, c, g.vc_rank))
    return D


def check_solves(el, g, device, dtype, n, nrhs, seed, dist):
    npdt = np.float64 if dtype == el.F64 else np.float32
    A = random_matrix(n, n, seed, npdt)
    Y = random_matrix(n, nrhs, seed + 1, npdt)
    A64, Y64 = A.astype(np.float64), Y.astype(np.float64)
    D = dist(A)
    P = el.LU(D)
    for orient, op in ((el.NORMAL, A64), (el.TRANSPOSE, A64.T), (el.ADJOINT, A64.T)):
        X = dist(Y)
        el.LUSolveAfter(orient, D, P, X)
        err = oo_norm(Y64 - op @ full_matrix(el, X).astype(np.float64))
        print(f"lu solve_after orient {orient} n={n} {npdt.__name__}: {err:.3g} <= {solve_bound(A, Y, npdt):.3g}")
        assert err <= solve_bound(A, Y, npdt), (orient, err)
    D2, X = dist(A), dist(Y)
    el.LinearSolve(D2, X)
    assert np.array_equal(_bits(full_matrix(el, D2)), _bits(A)), "LinearSolve changed A"
    err = oo_norm(Y64 - A64 @ full_matrix(el, X).astype(np.float64))
    assert err <= solve_bound(A, Y, npdt), err
