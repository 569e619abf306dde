"""Inputs, acceptance and the multi-rank worker of the El::TriangularInverse /
El::Trtrmm / El::HPDInverse tests (CPU over gloo, GPU host-staged); see
_dist_workers and _cholesky_workers.

Inputs: A = _cholesky_workers.hpd_matrix; L = numpy's float64 Cholesky factor of
A rounded to the type, U = L^T; for UNIT, diag(L)^-1 L (a unit triangle of modest
condition; L with its diagonal overwritten by ones has cond ~ 4e15) with NaN on
the diagonal that is fed in.  The strict other triangle is NaN in every case.

Acceptance, in float64: finite on the triangle, the other triangle (and the UNIT
diagonal) bit-identical to the input, then
  TriangularInverse  ||X T - I||_F and ||T X - I||_F <= 10 n eps ||T||_F ||X||_F
  Trtrmm             ||tri(got - L^T L)||_F          <= 10 n eps ||L||_F^2
  HPDInverse         ||A X - I||_F                   <= 10 n eps ||A||_F ||X||_F
The factor 10 is the project's convention.  LAPACK in the type (scipy's ?trtri /
?lauum / ?potri) on exactly these matrices, n = 1 .. 39 and 40 .. 1100 in steps of
53, seeds 100 + n, stays at or below these fractions of the bare bounds:
trtri NON_UNIT 0.13 (f32) / 0.032 (f64), trtri UNIT 0.004 / 0.004, lauum 0.11 /
0.10, potri 0.60 / 0.14.  A missed update gives a ratio of order 1 / eps."""
from __future__ import annotations

import traceback

import numpy as np

from _cholesky_workers import hpd_matrix, masked, other_triangle
from _dist_workers import _bits, _tol, finish, init

LOWER, UPPER, NON_UNIT, UNIT = 0, 1, 0, 1
_TINY = np.finfo(np.float64).tiny


def triangle(A, uplo, unit=False):
    """The clean triangular matrix T in A's type (zeros in the other triangle):
    numpy's float64 factor of A rounded to the type (L, or U = L^T); unit:
    diag(L)^-1 L, ones on the diagonal."""
    L = np.linalg.cholesky(A.astype(np.float64))
    if unit:
        L = L / np.diag(L)[:, None]
        L[np.diag_indices_from(L)] = 1.0
    L = L.astype(A.dtype)
    return np.asfortranarray(L if uplo == LOWER else L.T)


def fed(T, uplo, unit=False):
    """What goes in: T with the strict other triangle, and the UNIT diagonal, NaN."""
    Tin = masked(T, uplo)
    if unit:
        Tin[np.diag_indices_from(Tin)] = np.nan
    return Tin


def _untouched(n, uplo, unit):
    m = other_triangle(n, uplo)
    if unit:
        m = m | np.eye(n, dtype=bool)
    return m


def _shape_check(Tin, got, uplo, unit):
    keep = _untouched(Tin.shape[0], uplo, unit)
    if not np.isfinite(got[~keep]).all():
        return "not finite on the uplo triangle"
    if not np.array_equal(_bits(got[keep]), _bits(Tin[keep])):
        return "the other triangle (or the unit diagonal) was written"
    return None


def clean(got, uplo, unit=False):
    """got in float64 with zeros in the other triangle (and ones on a unit diagonal)."""
    n = got.shape[0]
    X = np.where(other_triangle(n, uplo), 0.0, got.astype(np.float64))
    if unit:
        X[np.diag_indices(n)] = 1.0
    return X


def accept_trtri(T, Tin, got, uplo, unit):
    """(None or what went wrong, the larger residual over n eps ||T||_F ||X||_F)."""
    why = _shape_check(Tin, got, uplo, unit)
    if why:
        return why, np.inf
    n = T.shape[0]
    eps = np.finfo(T.dtype).eps
    T64, X, I = T.astype(np.float64), clean(got, uplo, unit), np.eye(n)
    res = max(np.linalg.norm(X @ T64 - I), np.linalg.norm(T64 @ X - I))
    ratio = res / max(n * eps * np.linalg.norm(T64) * np.linalg.norm(X), _TINY)
    print(f"trtri residual n={n} {T.dtype} {'LU'[uplo]} {'unit' if unit else 'non-unit'}: "
          f"{ratio:.3g} of n eps ||T||_F ||X||_F")
    return (None if ratio <= 10 else f"residual {ratio:.3g} > 10 n eps ||T||_F ||X||_F"), ratio


def trtrmm_want(T, uplo):
    T64 = T.astype(np.float64)
    return T64.T @ T64 if uplo == LOWER else T64 @ T64.T


def accept_trtrmm(T, Tin, got, uplo):
    why = _shape_check(Tin, got, uplo, False)
    if why:
        return why, np.inf
    n = T.shape[0]
    eps = np.finfo(T.dtype).eps
    err = np.linalg.norm(clean(got, uplo) - np.where(other_triangle(n, uplo), 0.0, trtrmm_want(T, uplo)))
    ratio = err / max(n * eps * np.linalg.norm(T.astype(np.float64)) ** 2, _TINY)
    print(f"trtrmm error n={n} {T.dtype} {'LU'[uplo]}: {ratio:.3g} of n eps ||T||_F^2")
    return (None if ratio <= 10 else f"error {ratio:.3g} > 10 n eps ||T||_F^2"), ratio


def symmetrized(got, uplo):
    X = clean(got, uplo)
    return X + X.T - np.diag(np.diag(X))


def accept_hpd_inverse(A, Ain, got, uplo):
    why = _shape_check(Ain, got, uplo, False)
    if why:
        return why, np.inf
    n = A.shape[0]
    eps = np.finfo(A.dtype).eps
    A64, X = A.astype(np.float64), symmetrized(got, uplo)
    ratio = np.linalg.norm(A64 @ X - np.eye(n)) / max(n * eps * np.linalg.norm(A64) * np.linalg.norm(X), _TINY)
    print(f"hpd inverse residual n={n} {A.dtype} {'LU'[uplo]}: {ratio:.3g} of n eps ||A||_F ||X||_F")
    return (None if ratio <= 10 else f"residual {ratio:.3g} > 10 n eps ||A||_F ||X||_F"), ratio


def inverse_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, n: int, nb: int, seed: int):
    """The three functions, LOWER / UPPER (TriangularInverse also UNIT), on an [MC,MR]
    matrix whose other triangle is NaN.  Each rank checks its own local block against
    numpy's float64 result from the same input: ||got - want||_F <= 10 n eps cond_2(input)
    ||want||_F, the other triangle (and the UNIT diagonal) still NaN.  HPDInverse of a
    matrix with a negative diagonal entry raises NonHPDMatrixError on every rank."""
    import oracle
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        r, c = g.height, g.width
        npdt = np.float64 if dtype == el.F64 else np.float32
        el.SetBlocksize(nb)
        A = hpd_matrix(n, seed, npdt)

        def run(fn, Xin):
            D = el.DistMatrix(g, dtype, el.MC, el.MR, device, height=n, width=n)
            D.set_local(oracle.local_block(Xin, el.MC, el.MR, r, c, g.vc_rank))
            fn(D)
            return D.get_local().astype(np.float64)

        def check(what, fn, Xin, want_full, cond, keep_mask):
            got = run(fn, Xin)
            full = np.where(keep_mask, np.nan, want_full)
            want = oracle.local_block(full, el.MC, el.MR, r, c, g.vc_rank)
            keep = np.isfinite(want)
            assert np.isnan(got[~keep]).all(), f"{what} rank {rank}: the other triangle was written"
            assert np.isfinite(got[keep]).all(), f"{what} rank {rank}: not finite"
            err = np.linalg.norm(got[keep] - want[keep]) if keep.any() else 0.0
            bound = 10 * n * _tol(dtype) * cond * np.linalg.norm(want_full)
            assert err <= bound, f"{what} n {n} nb {nb} grid {r}x{c} rank {rank}: {err:.3g} > {bound:.3g}"

        A64 = A.astype(np.float64)
        for uplo in (el.LOWER, el.UPPER):
            for unit in (False, True):
                T = triangle(A, uplo, unit)
                T64 = T.astype(np.float64)
                diag = el.UNIT if unit else el.NON_UNIT
                check(f"TriangularInverse uplo {uplo} unit {unit}", lambda D: el.TriangularInverse(uplo, diag, D),
                      fed(T, uplo, unit), np.linalg.inv(T64), np.linalg.cond(T64), _untouched(n, uplo, unit))
            T = triangle(A, uplo)
            check(f"Trtrmm uplo {uplo}", lambda D: el.Trtrmm(uplo, D), fed(T, uplo), trtrmm_want(T, uplo),
                  np.linalg.cond(T.astype(np.float64)), other_triangle(n, uplo))
            check(f"HPDInverse uplo {uplo}", lambda D: el.HPDInverse(uplo, D), masked(A, uplo), np.linalg.inv(A64),
                  np.linalg.cond(A64), other_triangle(n, uplo))
            j = n // 2
            Abad = masked(A, uplo)
            Abad[j, j] = -1.0
            try:
                run(lambda D: el.HPDInverse(uplo, D), Abad)
            except el.NonHPDMatrixError as e:
                assert 1 <= e.column <= j + 1, (e.column, j)
            else:
                raise AssertionError(f"uplo {uplo} rank {rank}: no NonHPDMatrixError")
        finish()
    except Exception:
        traceback.print_exc()
        raise
