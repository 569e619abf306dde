"""Inputs, acceptance and the multi-rank workers of the El::QR tests (CPU over
gloo, GPU host-staged or RCCL); see _dist_workers."""
from __future__ import annotations

import traceback

import numpy as np

from _dist_workers import init, finish

NRHS = 9


def random_matrix(m, n, seed, npdt):
    import oracle
    return np.asfortranarray(oracle.hash_matrix(m, n, seed, 0.0, 1.0, npdt))


def rebuild_q(packed, t, d):
    """Q = H_0 .. H_{k-1} diag(d) in float64 from the packed reflectors (m x m):
    the reflectors applied to the identity from the last to the first."""
    m, n = packed.shape
    k = min(m, n)
    P = packed.astype(np.float64)
    t = np.asarray(t, np.float64).reshape(-1)
    d = np.asarray(d, np.float64).reshape(-1)
    Q = np.eye(m)
    for j in range(k - 1, -1, -1):
        u = np.concatenate(([1.0], P[j + 1:, j]))
        Q[j:, j:] -= t[j] * np.outer(u, u @ Q[j:, j:])
    Q[:, :k] *= d
    return Q


def accept(A, packed, t, d):
    """The acceptance every case shares.  A: what went in (in the type); packed, t,
    d: what came out.  Q is rebuilt in float64 as H_0 .. H_{k-1} diag(d).  Returns
    (None or what went wrong, Q).
      * everything is finite; d in {+-1}; diag(R) >= 0; 1 <= t_j <= 2;
      * |t_j (1 + ||u_j||^2) - 2| <= 10 m eps;
      * ||A - Q R||_F <= 10 max(m, n) eps ||A||_F;
      * ||Q^T Q - I||_F <= 10 max(m, n) eps.
    The last two are the LU acceptance's form: LAPACK's f64 Householder QR
    (numpy.linalg.qr) stays under 0.12 and 0.6 of the bare max(m, n) eps on these
    inputs, and test_qr_cpu asserts that a plain f32 restatement of the unblocked
    algorithm meets the same bounds, so they are reachable in both types."""
    m, n = A.shape
    k = min(m, n)
    eps = np.finfo(A.dtype).eps
    t = np.asarray(t).reshape(-1)
    d = np.asarray(d).reshape(-1)
    if t.shape != (k,) or d.shape != (k,):
        return f"t {t.shape}, d {d.shape} for {m} x {n}", None
    if not (np.isfinite(packed).all() and np.isfinite(t).all() and np.isfinite(d).all()):
        return "not finite", None
    if not (np.abs(d) == 1).all():
        return f"signature not +-1: {d.tolist()}", None
    P = packed.astype(np.float64)
    R = np.triu(P[:k])
    if not (np.diag(R) >= 0).all():
        return f"negative diagonal of R: {np.diag(R).min()!r}", None
    t64 = t.astype(np.float64)
    if not ((t64 >= 1).all() and (t64 <= 2).all()):
        return f"t outside [1, 2]: {t64.min()!r} .. {t64.max()!r}", None
    for j in range(k):
        u2 = float(P[j + 1:, j] @ P[j + 1:, j])
        if abs(t64[j] * (1 + u2) - 2) > 10 * m * eps:
            return f"t_{j} (1 + |u|^2) - 2 = {t64[j] * (1 + u2) - 2:.3g} > 10 m eps", None
    Q = rebuild_q(packed, t, d)
    A64 = A.astype(np.float64)
    # an exact power-of-two rescaling, so that the float64 norms below neither
    # overflow nor underflow on the scaled inputs
    amax = np.abs(A64).max(initial=0.0)
    sc = np.ldexp(1.0, -int(np.frexp(amax)[1])) if amax > 0 else 1.0
    A64, R = A64 * sc, R * sc
    na = np.linalg.norm(A64)
    res = np.linalg.norm(A64 - Q[:, :k] @ R) / (max(m, n) * eps * na) if na > 0 else 0.0
    orth = np.linalg.norm(Q.T @ Q - np.eye(m)) / (max(m, n) * eps)
    print(f"qr {m}x{n} {A.dtype}: residual {res:.3g}, orthogonality {orth:.3g} of max(m,n) eps")
    if not res <= 10:
        return f"residual {res:.3g} > 10 max(m,n) eps ||A||_F", Q
    if not orth <= 10:
        return f"orthogonality {orth:.3g} > 10 max(m,n) eps", Q
    return None, Q


def unblocked_reference(A):
    """The unblocked algorithm restated in plain numpy, every operation in A's type
    (reflector::Col with the scaled norm, then the rank-one update)."""
    T = A.dtype.type
    W = np.array(A, copy=True, order="F")
    m, n = W.shape
    k = min(m, n)
    t, d = np.zeros(k, A.dtype), np.zeros(k, A.dtype)
    for j in range(k):
        x = W[j + 1:, j]
        alpha = W[j, j]
        mx = np.abs(x).max(initial=T(0))
        if mx == 0:
            beta, t[j] = -alpha, T(2)
        else:
            nu = mx * np.sqrt(np.sum((x / mx) ** 2, dtype=A.dtype))
            nrm = np.hypot(alpha, nu)
            beta = nrm if alpha <= 0 else -nrm
            t[j] = (beta - alpha) / beta
            x /= (alpha - beta)
        z = W[j, j + 1:] + x @ W[j + 1:, j + 1:]
        W[j + 1:, j + 1:] -= t[j] * np.outer(x, z)
        d[j] = T(1) if beta >= 0 else T(-1)
        W[j, j + 1:] = d[j] * (W[j, j + 1:] - t[j] * z)
        W[j, j] = beta * d[j]
    return W, t, d


def ls_bound(A, X, B):
    """10 max(m, n) eps (||A||_F ||X||_F + ||B||_F), the factor the solve checks share."""
    m, n = A.shape
    f = lambda M: np.linalg.norm(M.astype(np.float64))
    return 10 * max(m, n) * np.finfo(A.dtype).eps * (f(A) * f(X) + f(B))


def check_least_squares(A, B, X):
    """||A^T (A X - B)||_F <= 10 max(m, n) eps ||A||_F (||A||_F ||X||_F + ||B||_F)"""
    A64, B64, X64 = (M.astype(np.float64) for M in (A, B, X))
    err = np.linalg.norm(A64.T @ (A64 @ X64 - B64))
    bound = np.linalg.norm(A64) * ls_bound(A, X, B)
    print(f"least squares {A.shape} {A.dtype}: {err:.3g} <= {bound:.3g}")
    return None if err <= bound else f"||A^T (A X - B)|| = {err:.3g} > {bound:.3g}"


def check_min_norm(A, B, X, Q):
    """||A^T X - B||_F <= 10 max(m, n) eps (||A||_F ||X||_F + ||B||_F) (the same form
    without the outer ||A||_F, which the normal equations bring), and X in range(A):
    ||X - Q_thin Q_thin^T X||_F <= the same bound."""
    A64, B64, X64 = (M.astype(np.float64) for M in (A, B, X))
    n = A.shape[1]
    bound = ls_bound(A, X, B)
    err = np.linalg.norm(A64.T @ X64 - B64)
    Qt = Q[:, :n]
    out = np.linalg.norm(X64 - Qt @ (Qt.T @ X64))
    print(f"minimum norm {A.shape} {A.dtype}: residual {err:.3g}, out of range {out:.3g} <= {bound:.3g}")
    if not err <= bound:
        return f"||A^T X - B|| = {err:.3g} > {bound:.3g}"
    if not out <= bound:
        return f"||X - Q Q^T X|| = {out:.3g} > {bound:.3g}"
    return None


def scaled_input(m, n, seed, npdt, up):
    """hash_matrix scaled by 2^+-600 (f64) / 2^+-80 (f32): every stored value stays in
    range, a plain sum of squares gives Inf / 0."""
    e = (600 if npdt == np.float64 else 80) * (1 if up else -1)
    return np.asfortranarray(np.ldexp(random_matrix(m, n, seed, npdt), e).astype(npdt))


def full_matrix(el, D):
    """Every rank's copy of the whole matrix ([*,*] <- D)."""
    S = D.like(el.STAR, el.STAR)
    S.assign(D)
    return S.get_local()


def _dist(el, g, dtype, device, A, U=None, V=None):
    import oracle
    U = el.MC if U is None else U
    V = el.MR if V is None else V
    D = el.DistMatrix(g, dtype, U, V, device, height=A.shape[0], width=A.shape[1])
    D.set_local(oracle.local_block(A, U, V, g.height, g.width, g.vc_rank))
    return D


def check_apply_and_explicit(el, g, dtype, device, A):
    """QRApplyQ NORMAL then ADJOINT restores B; QRExplicit gives Q^T Q = I and Q R = A,
    R upper with a non-negative diagonal."""
    m, n = A.shape
    k = min(m, n)
    eps = np.finfo(A.dtype).eps
    D = _dist(el, g, dtype, device, A)
    t, d = el.QR(D)
    why, Q = accept(A, full_matrix(el, D), t.get_local(), d.get_local())
    assert why is None, why
    B0 = random_matrix(m, NRHS, 7 + m, A.dtype)
    B = _dist(el, g, dtype, device, B0)
    el.QRApplyQ(el.LEFT, el.NORMAL, D, t, d, B)
    QB = full_matrix(el, B).astype(np.float64)
    bound = 10 * max(m, n) * eps * np.linalg.norm(B0.astype(np.float64))
    assert np.linalg.norm(QB - Q @ B0.astype(np.float64)) <= bound, "Q B"
    el.QRApplyQ(el.LEFT, el.ADJOINT, D, t, d, B)
    assert np.linalg.norm(full_matrix(el, B).astype(np.float64) - B0) <= bound, "Q^T Q B != B"
    E = _dist(el, g, dtype, device, A)
    Rm = E.like()
    el.QRExplicit(E, Rm)
    Qe, Re = full_matrix(el, E).astype(np.float64), full_matrix(el, Rm).astype(np.float64)
    assert Qe.shape == (m, k) and Re.shape == (k, n), (Qe.shape, Re.shape)
    assert np.array_equal(Re, np.triu(Re)) and (np.diag(Re) >= 0).all()
    assert np.linalg.norm(Qe.T @ Qe - np.eye(k)) <= 10 * max(m, n) * eps
    assert np.linalg.norm(Qe @ Re - A) <= 10 * max(m, n) * eps * np.linalg.norm(A.astype(np.float64))
    T = _dist(el, g, dtype, device, A)
    el.QRExplicitTriang(T)
    Rt = full_matrix(el, T).astype(np.float64)
    assert Rt.shape == (k, n) and np.linalg.norm(Rt - Re) <= 10 * max(m, n) * eps * np.linalg.norm(Re)
    return D, t, d, Q


def check_solves(el, g, dtype, device, A):
    """QRSolveAfter NORMAL / ADJOINT and LeastSquares in both orientations, m >= n."""
    m, n = A.shape
    D = _dist(el, g, dtype, device, A)
    t, d = el.QR(D)
    why, Q = accept(A, full_matrix(el, D), t.get_local(), d.get_local())
    assert why is None, why
    B = random_matrix(m, NRHS, 11 + m, A.dtype)
    C = random_matrix(n, NRHS, 13 + n, A.dtype)
    Bd, Cd = _dist(el, g, dtype, device, B), _dist(el, g, dtype, device, C)
    for solve in (lambda o, Y, X: el.QRSolveAfter(o, D, t, d, Y, X),
                  lambda o, Y, X: el.LeastSquares(o, _dist(el, g, dtype, device, A), Y, X)):
        X = Bd.like()
        solve(el.NORMAL, Bd, X)
        Xh = full_matrix(el, X)
        assert Xh.shape == (n, NRHS), Xh.shape
        why = check_least_squares(A, B, Xh)
        assert why is None, why
        for orient in (el.TRANSPOSE, el.ADJOINT):
            X = Bd.like()
            solve(orient, Cd, X)
            Xh = full_matrix(el, X)
            assert Xh.shape == (m, NRHS), Xh.shape
            why = check_min_norm(A, C, Xh, Q)
            assert why is None, why


def qr_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, shapes, nb: int, seed: int):
    """El::QR on [MC,MR] matrices with t and d on two different distributions,
    through `accept` on every rank; ApplyQ, Explicit and ExplicitTriang on the
    same shapes.  Against the 1 x 1 result only the acceptance is asserted: the
    1 x 1 grid takes the local recursion (leaves of 16 columns), the other grids
    panels of nb columns and SUMMA sums, so the panel boundaries do not coincide."""
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        npdt = np.float64 if dtype == el.F64 else np.float32
        el.SetBlocksize(nb)
        for (m, n) in shapes:
            A = random_matrix(m, n, seed + m + 3 * n, npdt)
            D, t, d, _ = check_apply_and_explicit(el, g, dtype, device, A)
            assert (t.Height(), t.Width(), d.Height(), d.Width()) == (min(m, n), 1, min(m, n), 1)
            # the scalars through another distribution give the same product
            tv = el.DistMatrix(g, dtype, el.VC, el.STAR, device, height=min(m, n), width=1)
            tv.assign(t)
            B0 = random_matrix(m, 3, 5, npdt)
            B1, B2 = _dist(el, g, dtype, device, B0), _dist(el, g, dtype, device, B0, el.VR, el.STAR)
            el.QRApplyQ(el.LEFT, el.ADJOINT, D, t, d, B1)
            el.QRApplyQ(el.LEFT, el.ADJOINT, D, tv, d, B2)
            assert np.array_equal(full_matrix(el, B1), full_matrix(el, B2)), "t on [VC,*], B on [VR,*]"
        finish()
    except Exception:
        traceback.print_exc()
        raise


def solve_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, m: int, n: int, nb: int,
                 seed: int):
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        npdt = np.float64 if dtype == el.F64 else np.float32
        el.SetBlocksize(nb)
        check_solves(el, g, dtype, device, random_matrix(m, n, seed, npdt))
        finish()
    except Exception:
        traceback.print_exc()
        raise
