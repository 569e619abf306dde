"""Inputs, acceptance, the numpy restatement and the multi-rank workers of the
El::HermitianTridiag tests (CPU over gloo, GPU host-staged or RCCL); see
_dist_workers."""
from __future__ import annotations

import traceback

import numpy as np

from _dist_workers import init, finish, _bits

NRHS = 7


def random_symmetric(n, seed, npdt):
    """A full symmetric matrix, uniform in [-1, 1], in the type."""
    import oracle
    G = oracle.hash_matrix(n, n, seed, -1.0, 1.0, npdt)
    return np.asfortranarray(np.tril(G) + np.tril(G, -1).T)


def one_triangle(S, lower, fill=np.nan):
    """S with the triangle the routine must not touch replaced by `fill`."""
    A = np.array(S, order="F", copy=True)
    A[np.triu_indices_from(A, 1) if lower else np.tril_indices_from(A, -1)] = fill
    return A


def symmetric_of(A, lower):
    """The float64 symmetric matrix the uplo triangle of A stands for."""
    A64 = A.astype(np.float64)
    H = np.tril(A64) if lower else np.triu(A64)
    return H + (np.tril(A64, -1).T if lower else np.triu(A64, 1).T)


def rebuild_q(packed, t, lower):
    """Q in float64 from the packed reflectors: LOWER H_0 .. H_{n-2} with v_k = [0_{k+1};
    1; A(k+2:n, k)], UPPER H_{n-1} .. H_1 with v_k = [A(0:k-1, k); 1; 0] and t(k-1)."""
    n = packed.shape[0]
    P = packed.astype(np.float64)
    t = np.asarray(t, np.float64).reshape(-1)
    Q = np.eye(n)
    order = range(n - 2, -1, -1) if lower else range(1, n)  # the last factor first
    for k in order:
        v = np.zeros(n)
        if lower:
            v[k + 1], v[k + 2:], tk = 1.0, P[k + 2:, k], t[k]
        else:
            v[k - 1], v[:k - 1], tk = 1.0, P[:k - 1, k], t[k - 1]
        Q -= tk * np.outer(v, v @ Q)
    return Q


def tridiagonal(packed, lower):
    """(d, e) of T from the returned matrix."""
    P = packed.astype(np.float64)
    return np.diag(P).copy(), (np.diag(P, -1) if lower else np.diag(P, 1)).copy()


def accept(A, packed, t, lower, quiet=False):
    """The acceptance every case shares.  A: what went in (in the type; only its uplo
    triangle counts); packed, t: what came out.  Returns (None or what went wrong, Q).
      * the uplo triangle and t are finite; 1 <= t <= 2;
      * |t (1 + |u|^2) - 2| <= 10 n eps;
      * ||S - Q T Q^T||_F <= 10 n eps ||S||_F;
      * ||Q^T Q - I||_F <= 10 n eps;
      * max |lambda(T) - lambda(S)| <= 10 n eps ||S||_2;
      * the other triangle is bit-identical to the input.
    S and T are rescaled by an exact power of two first, so scaled inputs neither
    overflow nor underflow in the float64 norms."""
    n = A.shape[0]
    eps = np.finfo(A.dtype).eps
    t = np.asarray(t).reshape(-1)
    if packed.shape != A.shape or t.shape != (max(n - 1, 0),):
        return f"packed {packed.shape}, t {t.shape} for n = {n}", None
    other = np.triu_indices(n, 1) if lower else np.tril_indices(n, -1)
    if not np.array_equal(_bits(np.ascontiguousarray(packed[other])), _bits(np.ascontiguousarray(A[other]))):
        return "the other triangle changed", None
    mine = np.tril_indices(n) if lower else np.triu_indices(n)
    if not (np.isfinite(packed[mine]).all() and np.isfinite(t).all()):
        return "not finite", None
    t64 = t.astype(np.float64)
    if not ((t64 >= 1).all() and (t64 <= 2).all()):
        return f"t outside [1, 2]: {t64.min()!r} .. {t64.max()!r}", None
    P = np.where(np.isfinite(packed), packed, 0).astype(np.float64)
    worst_t = 0.0
    for k in range(n - 1):
        u = P[k + 2:, k] if lower else P[:k, k + 1]
        worst_t = max(worst_t, abs(t64[k] * (1 + float(u @ u)) - 2))
    if n and worst_t > 10 * n * eps:
        return f"t (1 + |u|^2) - 2 = {worst_t:.3g} > 10 n eps", None
    Q = rebuild_q(P, t, lower)
    S = symmetric_of(np.where(np.isfinite(A), A, 0), lower)
    d, e = tridiagonal(P, lower)
    amax = np.abs(S).max(initial=0.0)
    sc = np.ldexp(1.0, -int(np.frexp(amax)[1])) if amax > 0 else 1.0
    S, d, e = S * sc, d * sc, e * sc
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    ns = np.linalg.norm(S)
    res = np.linalg.norm(S - Q @ T @ Q.T) / (n * eps * ns) if ns > 0 else 0.0
    orth = np.linalg.norm(Q.T @ Q - np.eye(n)) / (n * eps) if n else 0.0
    n2 = np.linalg.norm(S, 2) if n else 0.0
    eig = np.abs(np.linalg.eigvalsh(T) - np.linalg.eigvalsh(S)).max(initial=0.0) / (n * eps * n2) if n2 > 0 else 0.0
    if not quiet:
        print(f"tridiag {'L' if lower else 'U'} n={n} {A.dtype}: residual {res:.3g}, orthogonality {orth:.3g}, "
              f"eigenvalues {eig:.3g}, t {worst_t / (n * eps) if n else 0:.3g} of n eps")
    if not res <= 10:
        return f"residual {res:.3g} > 10 n eps ||S||_F", Q
    if not orth <= 10:
        return f"orthogonality {orth:.3g} > 10 n eps", Q
    if not eig <= 10:
        return f"eigenvalues {eig:.3g} > 10 n eps ||S||_2", Q
    return None, Q


def _reflector(alpha, x):
    """reflector::Col on (alpha, x) in x's type; x is scaled in place.  (beta, t)"""
    T = x.dtype.type
    mx = np.abs(x).max(initial=T(0))
    if mx == 0:
        return -alpha, T(2)
    nu = mx * np.sqrt(np.sum((x / mx) ** 2, dtype=x.dtype))
    nrm = np.hypot(alpha, nu)
    beta = nrm if alpha <= 0 else -nrm
    x /= (alpha - beta)
    return beta, T((beta - alpha) / beta)


def restated(A, lower, w=1):
    """The reduction restated in plain numpy, every operation in A's type: the
    blocked latrd form with panels of w columns (w = 1 is the unblocked loop).
    UPPER is LOWER on the matrix with both index orders reversed.  Returns (packed,
    t) with the other triangle as it came in."""
    if not lower:
        P, t = restated(np.asfortranarray(A[::-1, ::-1]), True, w)
        return np.asfortranarray(P[::-1, ::-1]), t[::-1].copy()
    dt = A.dtype
    n = A.shape[0]
    M = np.array(A, order="F", copy=True)
    M[np.triu_indices(n, 1)] = 0
    t = np.zeros(max(n - 1, 0), dt)
    for c0 in range(0, n - 1, w):
        wd = min(w, n - 1 - c0)
        V, W = np.zeros((n, wd), dt), np.zeros((n, wd), dt)
        for j in range(wd):
            c = c0 + j
            M[c:, c] -= V[c:, :j] @ W[c, :j] + W[c:, :j] @ V[c, :j]
            beta, t[c] = _reflector(M[c + 1, c], M[c + 2:, c])
            M[c + 1, c] = beta
            v = np.concatenate((np.ones(1, dt), M[c + 2:, c]))
            V[c + 1:, j] = v
            L = M[c + 1:, c + 1:]
            y = L @ v + np.tril(L, -1).T @ v
            Vp, Wp = V[c + 1:, :j], W[c + 1:, :j]
            y = t[c] * (y - Vp @ (Wp.T @ v) - Wp @ (Vp.T @ v))
            W[c + 1:, j] = y - (t[c] / dt.type(2)) * (y @ v) * v
        r = c0 + wd
        M[r:, r:] -= np.tril(V[r:] @ W[r:].T + W[r:] @ V[r:].T)
    out = np.array(A, order="F", copy=True)
    out[np.tril_indices(n)] = M[np.tril_indices(n)]
    return out, t


def exact_inputs(n, seed, npdt):
    """(name, full symmetric input) of the exact cases: tridiagonal and diagonal."""
    S = random_symmetric(n, seed, npdt)
    tri = np.asfortranarray(np.triu(np.tril(S, 1), -1))
    return [("tridiagonal", tri), ("diagonal", np.asfortranarray(np.diag(np.diag(S))))]


def check_exact(S, packed, t, lower):
    """A tridiagonal (or diagonal) input comes back with its diagonal and
    |off-diagonal| bit for bit, every t = 2 and zeros in the reflector positions."""
    n = S.shape[0]
    assert np.array_equal(_bits(np.diag(packed).copy()), _bits(np.diag(S).copy())), "diagonal changed"
    k = -1 if lower else 1
    assert np.array_equal(_bits(np.abs(np.diag(packed, k))), _bits(np.abs(np.diag(S, k)))), "|off-diagonal| changed"
    assert (np.asarray(t) == 2).all(), "t != 2"
    refl = np.tril(packed, -2) if lower else np.triu(packed, 2)
    assert (refl == 0).all(), "reflector positions not zero"
    assert n < 2 or t.shape == (n - 1,)


def zero_tail_input(n, c, seed, npdt, lower):
    """A symmetric input whose c-th reflector (in the order the reduction takes them)
    has an exactly zero tail: block diagonal with a leading block of c + 2, which the
    earlier reflectors leave block diagonal exactly.  UPPER: the same reversed, the
    scalar is t[n - 2 - c]."""
    S = random_symmetric(n, seed, npdt)
    S[c + 2:, :c + 2] = 0
    S[:c + 2, c + 2:] = 0
    return S if lower else np.asfortranarray(S[::-1, ::-1])


def scaled_symmetric(n, seed, npdt, up):
    """random_symmetric scaled by 2^+-500 (f64) / 2^+-50 (f32): products of
    three entries, and squares on the small side, leave the type's range."""
    e = (500 if npdt == np.float64 else 50) * (1 if up else -1)
    return np.asfortranarray(np.ldexp(random_symmetric(n, seed, npdt), e).astype(npdt))


def full_matrix(el, D):
    """Every rank's copy of the whole matrix ([*,*] <- D)."""
    S = D.like(el.STAR, el.STAR)
    S.assign(D)
    return S.get_local()


def _dist(el, g, dtype, device, A, U=None, V=None, calign=0, ralign=0):
    import oracle
    U = el.MC if U is None else U
    V = el.MR if V is None else V
    D = el.DistMatrix(g, dtype, U, V, device, height=A.shape[0], width=A.shape[1])
    if calign or ralign:
        D.Align(calign, ralign)
        D.Resize(A.shape[0], A.shape[1])
        D.assign(_dist(el, g, dtype, device, A, U, V))
        return D
    D.set_local(oracle.local_block(A, U, V, g.height, g.width, g.vc_rank))
    return D


def check_drivers(el, g, dtype, device, S, uplo, t_dist=None, calign=0, ralign=0):
    """el.HermitianTridiag through the acceptance, HermitianTridiagApplyQ in both
    orientations against the float64 Q, Q^T (Q B) = B, and ExplicitCondensed.  The
    other triangle carries a marker value that must come back.  Returns (packed, t)."""
    n = S.shape[0]
    lower = uplo == el.LOWER
    eps = np.finfo(S.dtype).eps
    A = one_triangle(S, lower, fill=S.dtype.type(12345))
    D = _dist(el, g, dtype, device, A, calign=calign, ralign=ralign)
    if t_dist is None:
        t = el.HermitianTridiag(uplo, D)
    else:  # the driver itself resizes and fills a t of another distribution (and a wrong size)
        from elemental_amd import _lib as L
        t = el.DistMatrix(g, dtype, t_dist[0], t_dist[1], device, height=3, width=2)
        L.call("elx_hermitian_tridiag", uplo, D.h, t.h)
    assert (t.Height(), t.Width()) == (max(n - 1, 0), 1)
    packed, th = full_matrix(el, D), full_matrix(el, t).reshape(-1)
    why, Q = accept(A, packed, th, lower)
    assert why is None, why
    B0 = np.asfortranarray(random_symmetric(max(n, NRHS), 7 + n, S.dtype)[:n, :NRHS])
    B = _dist(el, g, dtype, device, B0)
    bound = 10 * max(n, 1) * eps * np.linalg.norm(B0.astype(np.float64))
    el.HermitianTridiagApplyQ(el.LEFT, uplo, el.NORMAL, D, t, B)
    assert np.linalg.norm(full_matrix(el, B).astype(np.float64) - Q @ B0.astype(np.float64)) <= bound, "Q B"
    el.HermitianTridiagApplyQ(el.LEFT, uplo, el.ADJOINT, D, t, B)
    assert np.linalg.norm(full_matrix(el, B).astype(np.float64) - B0) <= bound, "Q^T (Q B) != B"
    el.HermitianTridiagApplyQ(el.LEFT, uplo, el.TRANSPOSE, D, t, B)
    assert np.linalg.norm(full_matrix(el, B).astype(np.float64) - Q.T @ B0.astype(np.float64)) <= bound, "Q^T B"
    E = _dist(el, g, dtype, device, A, calign=calign, ralign=ralign)
    el.HermitianTridiagExplicitCondensed(uplo, E)
    C = full_matrix(el, E)
    band = np.triu(np.tril(packed), -1) if lower else np.tril(np.triu(packed), 1)
    want = np.where(np.tril(np.ones_like(A, bool)) if lower else np.triu(np.ones_like(A, bool)), band, A)
    assert np.array_equal(C, want), "ExplicitCondensed"  # by value: a zeroed entry may be -0
    return packed, th


def tridiag_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, cases, seed: int):
    """El::HermitianTridiag, ApplyQ and ExplicitCondensed on [MC,MR] matrices with
    random alignments, t as [*,*] and as [MC,MR], both uplo, through `accept` on
    every rank.  cases: (n, nb)."""
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        npdt = np.float64 if dtype == el.F64 else np.float32
        rng = np.random.RandomState(seed)
        for (n, nb) in cases:
            el.SetBlocksize(nb)
            S = random_symmetric(n, seed + n, npdt)
            for uplo in (el.LOWER, el.UPPER):
                ca, ra = int(rng.randint(0, g.height)), int(rng.randint(0, g.width))
                # the 1 x 1 grid's result, on this rank alone
                P1, t1 = check_drivers(el, el.Grid(), dtype, device, S, uplo)
                for t_dist in (None, (el.MC, el.MR)):
                    P, t = check_drivers(el, g, dtype, device, S, uplo, t_dist, ca, ra)
                    # The grid runs another algorithm (panels of nb, distributed sums) than
                    # the 1 x 1 driver.  Both are backward stable, which bounds neither the
                    # reflectors nor T entry by entry (late columns amplify rounding), so
                    # "equal within the acceptance" is what the acceptance implies for the
                    # pair: both spectra lie within 10 n eps ||S||_2 of S's, hence within
                    # twice that of each other
                    lam = [np.linalg.eigvalsh(np.diag(d) + np.diag(e, 1) + np.diag(e, -1))
                           for d, e in (tridiagonal(P, uplo == el.LOWER), tridiagonal(P1, uplo == el.LOWER))]
                    bound = 20 * n * np.finfo(npdt).eps * np.linalg.norm(S.astype(np.float64), 2)
                    assert np.abs(lam[0] - lam[1]).max(initial=0) <= bound, "spectrum differs from 1 x 1"
                    assert t.shape == t1.shape
        finish()
    except Exception:
        traceback.print_exc()
        raise
