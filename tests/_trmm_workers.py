"""Multi-rank worker for El::Trmm (CPU over gloo, GPU host-staged); see _dist_workers."""
from __future__ import annotations

import traceback

import numpy as np

from _dist_workers import _tol, finish, init


def trmm_ref(side, uplo, orient, diag, alpha, Ag, Bg):
    """alpha op(tri(A)) B (LEFT) / alpha B op(tri(A)) (RIGHT) in float64 from the
    stored triangle alone (numpy; uplo 0 = LOWER, orient 0 = NORMAL, diag 1 = UNIT)."""
    T = (np.tril if uplo == 0 else np.triu)(np.nan_to_num(Ag.astype(np.float64)))
    if diag == 1:
        np.fill_diagonal(T, 1.0)
    if orient != 0:
        T = T.T
    B = Bg.astype(np.float64)
    return alpha * (T @ B if side == 0 else B @ T)


def masked_triangle(Ag, uplo, diag):
    """A with everything El::Trmm must not read set to NaN."""
    Ag = Ag.copy()
    k = Ag.shape[0]
    i, j = np.indices((k, k))
    Ag[(i < j) if uplo == 0 else (i > j)] = np.nan
    if diag == 1:
        Ag[np.diag_indices(k)] = np.nan
    return Ag


def trmm_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, m: int, n: int, nb: int,
                seed: int):
    """El::Trmm, every side x uplo x orientation x diag (Trmm/{LLN,...,RUT}.hpp),
    against numpy; the triangle (and unit diagonal) A must not read is NaN.  Each
    rank checks its own local block: ||got - want||_F <= 10 k eps ||ref||_F, k the
    order of A, and the result is finite."""
    import oracle
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        r, c = g.height, g.width
        npdt = np.float64 if dtype == el.F64 else np.float32
        el.SetBlocksize(nb)
        for side in (el.LEFT, el.RIGHT):
            for uplo in (el.LOWER, el.UPPER):
                for orient in (el.NORMAL, el.TRANSPOSE):
                    for diag in (el.NON_UNIT, el.UNIT):
                        k = m if side == el.LEFT else n
                        Ag = masked_triangle(oracle.hash_matrix(k, k, seed + 1, -1.0, 1.0, npdt), uplo, diag)
                        Bg = oracle.hash_matrix(m, n, seed + 2, -1.0, 1.0, npdt)
                        alpha = 0.75
                        ref = trmm_ref(side, uplo, orient, diag, alpha, Ag, Bg)
                        A = el.DistMatrix(g, dtype, el.MC, el.MR, device, height=k, width=k)
                        B = el.DistMatrix(g, dtype, el.MC, el.MR, device, height=m, width=n)
                        A.set_local(oracle.local_block(Ag, el.MC, el.MR, r, c, g.vc_rank))
                        B.set_local(oracle.local_block(Bg, el.MC, el.MR, r, c, g.vc_rank))
                        el.Trmm(side, uplo, orient, diag, alpha, A, B)
                        got = B.get_local().astype(np.float64)
                        want = oracle.local_block(ref, el.MC, el.MR, r, c, g.vc_rank)
                        num = np.linalg.norm(got - want) if got.size else 0.0
                        den = np.linalg.norm(ref) * k * _tol(dtype)
                        assert np.isfinite(got).all() and num <= 10 * den, \
                            (f"Trmm side {side} uplo {uplo} orient {orient} diag {diag} {m}x{n} nb {nb} "
                             f"grid {r}x{c} rank {rank}: {num / den:.3g}")
        finish()
    except Exception:
        traceback.print_exc()
        raise
