"""Inputs, acceptance and the multi-rank worker of the El::Cholesky tests (CPU
over gloo, GPU host-staged); see _dist_workers."""
from __future__ import annotations

import traceback

import numpy as np

from _dist_workers import _bits, _tol, finish, init


def hpd_matrix(n, seed, npdt):
    """A = G G^T + n I in float64, rounded to the type; G = hash_matrix in [-1, 1]."""
    import oracle
    G = oracle.hash_matrix(n, n, seed, 0.0, 1.0, npdt).astype(np.float64)
    return (G @ G.T + n * np.eye(n)).astype(npdt)


def other_triangle(n, uplo):
    """Mask of the strict triangle El::Cholesky(uplo, .) must neither read nor write
    (uplo 0 = LOWER)."""
    i, j = np.indices((n, n))
    return (i < j) if uplo == 0 else (i > j)


def masked(A, uplo):
    """A with the strict other triangle set to NaN."""
    A = np.array(A, order="F", copy=True)
    A[other_triangle(A.shape[0], uplo)] = np.nan
    return A


def accept(A, Ain, got, uplo):
    """The acceptance every case shares.  A: the symmetric matrix (in the type);
    Ain: what went in (other triangle NaN); got: what came out.  Returns
    (None or what went wrong, the residual over n eps ||A||_F).  The bound is
    10 n eps ||A||_F, the factor 10 being the project's convention for Trmm and
    Trsm: LAPACK's blocked potrf in the type (numpy) stays at or below 0.42 of
    the bare n eps ||A||_F on these matrices (n = 1 .. 39 and 40 .. 1100 in steps
    of 53, f32 and f64, G in [-1, 1]), and a missed update gives an O(1) / eps ratio."""
    n = A.shape[0]
    eps = np.finfo(A.dtype).eps
    oth = other_triangle(n, uplo)
    if not np.isfinite(got[~oth]).all():
        return "not finite on the uplo triangle", np.inf
    if not np.array_equal(_bits(got[oth]), _bits(Ain[oth])):
        return "the other triangle was written", np.inf
    T = np.where(oth, 0.0, got.astype(np.float64))
    L = T if uplo == 0 else T.T
    A64 = A.astype(np.float64)
    ratio = np.linalg.norm(np.tril(A64 - L @ L.T)) / max(n * eps * np.linalg.norm(A64), np.finfo(np.float64).tiny)
    print(f"cholesky residual n={n} {A.dtype} {'LU'[uplo]}: {ratio:.3g} of n eps ||A||_F")
    return (None if ratio <= 10 else f"residual {ratio:.3g} > 10 n eps ||A||_F"), ratio


def cholesky_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, n: int, nb: int,
                    seed: int):
    """El::Cholesky LOWER / UPPER on an [MC,MR] matrix whose other triangle is NaN.
    Each rank checks its own local block against numpy's factor of the float64
    matrix: ||got - want||_F <= 10 n eps cond_2(A) ||L||_F, the other triangle
    still NaN.  Then the not-HPD case (a negative diagonal entry inside a later
    leaf) must raise NonHPDMatrixError on every rank, and a valid factorization
    afterwards still passes."""
    import oracle
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        r, c = g.height, g.width
        npdt = np.float64 if dtype == el.F64 else np.float32
        el.SetBlocksize(nb)
        A = hpd_matrix(n, seed, npdt)
        A64 = A.astype(np.float64)
        Lref = np.linalg.cholesky(A64)
        bound = 10 * n * _tol(dtype) * np.linalg.cond(A64) * np.linalg.norm(Lref)

        def factor(uplo, Ain):
            D = el.DistMatrix(g, dtype, el.MC, el.MR, device, height=n, width=n)
            D.set_local(oracle.local_block(Ain, el.MC, el.MR, r, c, g.vc_rank))
            el.Cholesky(uplo, D)
            return D.get_local().astype(np.float64)

        def check(uplo):
            got = factor(uplo, masked(A, uplo))
            full = np.where(other_triangle(n, uplo), np.nan, Lref if uplo == el.LOWER else Lref.T)
            want = oracle.local_block(full, el.MC, el.MR, r, c, g.vc_rank)
            keep = np.isfinite(want)
            assert np.isnan(got[~keep]).all(), f"uplo {uplo} rank {rank}: the other triangle was written"
            assert np.isfinite(got[keep]).all(), f"uplo {uplo} rank {rank}: not finite"
            err = np.linalg.norm(got[keep] - want[keep]) if keep.any() else 0.0
            assert err <= bound, f"uplo {uplo} n {n} nb {nb} grid {r}x{c} rank {rank}: {err:.3g} > {bound:.3g}"

        for uplo in (el.LOWER, el.UPPER):
            check(uplo)
            j = n // 2
            Abad = masked(A, uplo)
            Abad[j, j] = -1.0
            try:
                factor(uplo, Abad)
            except el.NonHPDMatrixError as e:
                assert 1 <= e.column <= j + 1, (e.column, j)
            else:
                raise AssertionError(f"uplo {uplo} rank {rank}: no NonHPDMatrixError")
            check(uplo)
        finish()
    except Exception:
        traceback.print_exc()
        raise
