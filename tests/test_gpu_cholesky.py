"""El::Cholesky on the GPU: the in-LDS diagonal-block kernel (potrf.hip) through
elx_matrix_cholesky, the blocked driver on a 1x1 grid, the not-HPD path, the
argument checks, SolveAfter and the distributed driver.

Inputs: A = G G^T + n I in float64 rounded to the type, G = hash_matrix in
[-1, 1]; the strict other triangle is NaN.  Acceptance (_cholesky_workers.accept):
finite on the uplo triangle, the other triangle bit-identical to what went in,
||tri(A - L L^T)||_F <= 10 n eps ||A||_F."""
import random
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import _cholesky_workers as CW
import oracle
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPDT = {el.F64: np.float64, el.F32: np.float32}
BOTH_TYPES = [el.F64, el.F32]
BOTH_UPLO = [el.LOWER, el.UPPER]


def _port():
    """A free rendezvous port below the kernel's ephemeral range (see test_gpu_dist)."""
    for _ in range(200):
        p = random.randrange(20000, 32000)
        s = socket.socket()
        try:
            s.bind(("127.0.0.1", p))
            return p
        except OSError:
            continue
        finally:
            s.close()
    raise RuntimeError("no free port in 20000-32000")


def _spawn(fn, world, *args):
    mp.spawn(fn, args=(world, _port()) + args, nprocs=world, join=True)


def _leaf_max():
    return int(L.lib().elx_cholesky_leaf_max())


def _matrix_cholesky(dtype, uplo, Ain, pad):
    """elx_matrix_cholesky on the column-major Ain with lda = n (aligned) or n + 3
    and the base one element into the allocation (pad); everything around the
    matrix is NaN.  Returns the result, after checking that nothing outside the
    n x n matrix changed."""
    n = Ain.shape[0]
    lda, off = (n + 3, 1) if pad else (n, 0)
    buf = np.full(off + lda * n, np.nan, Ain.dtype)
    buf[off:].reshape(n, lda)[:, :n] = Ain.T
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    L.call("elx_matrix_cholesky", dtype, el.GPU, uplo, n, t.data_ptr() + off * Ain.dtype.itemsize, lda, None)
    L.call("elx_device_synchronize")
    out = t.cpu().numpy()
    inside = np.zeros(buf.shape, bool)
    inside[off:].reshape(n, lda)[:, :n] = True
    assert np.array_equal(_bits(out[~inside]), _bits(buf[~inside])), "written outside the matrix"
    return out[off:].reshape(n, lda)[:, :n].T


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_cholesky_leaf_kernel(dtype):
    """potrf_kernel alone (n <= kPotrfMax is one leaf): the panel (16), MFMA-tile
    and LDS edges, LOWER and UPPER, aligned and misaligned."""
    npdt = NPDT[dtype]
    bad = []
    for n in (1, 2, 15, 16, 17, 31, 33, 63, 65, 127, _leaf_max()):
        A = CW.hpd_matrix(n, 100 + n, npdt)
        for uplo in BOTH_UPLO:
            Ain = CW.masked(A, uplo)
            for pad in (False, True):
                why, _ = CW.accept(A, Ain, _matrix_cholesky(dtype, uplo, Ain, pad), uplo)
                if why:
                    bad.append((n, "LU"[uplo], "padded" if pad else "aligned", why))
    assert not bad, f"{len(bad)} cases: {bad}"


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("n", [5, 17, 40])
def test_cholesky_leaf_integer(dtype, n):
    """A = L0 L0^T with L0 integer (off the diagonal in [-2, 2], diagonal in
    {1, 2, 4}): the factor must equal L0 to the acceptance bound, ||L - L0||_F <=
    10 n eps ||A||_F.  (The leaf is a panel algorithm with MFMA updates, not the
    plain column loop, so this is the bound and not bit-equality; every
    intermediate value is in fact an integer or a quarter of one.)"""
    npdt = NPDT[dtype]
    rng = np.random.default_rng(n)
    L0 = np.tril(rng.integers(-2, 3, (n, n)), -1).astype(np.float64)
    L0[np.diag_indices(n)] = rng.choice([1.0, 2.0, 4.0], n)
    A = (L0 @ L0.T).astype(npdt)
    for uplo in BOTH_UPLO:
        Ain = CW.masked(A, uplo)
        got = _matrix_cholesky(dtype, uplo, Ain, False)
        why, _ = CW.accept(A, Ain, got, uplo)
        assert why is None, why
        T = np.where(CW.other_triangle(n, uplo), 0.0, got.astype(np.float64))
        Lg = T if uplo == el.LOWER else T.T
        err = np.linalg.norm(Lg - L0)
        print(f"integer n={n}: ||L - L0||_F = {err:.3g}")
        assert err <= 10 * n * np.finfo(npdt).eps * np.linalg.norm(A.astype(np.float64))


def _driver_case(dtype, uplo, n, seed, g=None):
    npdt = NPDT[dtype]
    A = CW.hpd_matrix(n, seed, npdt)
    Ain = CW.masked(A, uplo)
    D = el.DistMatrix(g or el.Grid(), dtype, height=n, width=n)
    D.set_local(Ain)
    el.Cholesky(uplo, D)
    why, _ = CW.accept(A, Ain, D.get_local(), uplo)
    assert why is None, (n, uplo, why)
    return A, D


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("n", [129, 300, 1100])
def test_cholesky_driver(dtype, n):
    """1x1 grid, default Blocksize: 129 is the first size with two blocks, 300 has
    a ragged last block, 1100 three levels of the recursive split."""
    nb0 = el.Blocksize()
    el.SetBlocksize(128)
    try:
        for uplo in BOTH_UPLO:
            _driver_case(dtype, uplo, n, 200 + n)
    finally:
        el.SetBlocksize(nb0)


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_cholesky_driver_small_blocks(dtype):
    nb0 = el.Blocksize()
    el.SetBlocksize(32)
    try:
        for uplo in BOTH_UPLO:
            _driver_case(dtype, uplo, 100, 77)
    finally:
        el.SetBlocksize(nb0)


def test_cholesky_not_hpd():
    """A negative diagonal entry inside the first leaf (j = 0, 7) and inside a later
    one (j = 200 of n = 300), and an all-NaN diagonal: NonHPDMatrixError with 1 <=
    column <= j + 1 (exactly 1 for j = 0), and a valid factorization afterwards
    passes."""
    n = 300
    nb0 = el.Blocksize()
    el.SetBlocksize(128)
    try:
        A = CW.hpd_matrix(n, 9, np.float64)
        g = el.Grid()
        for uplo in BOTH_UPLO:
            for j in (0, 7, 200, None):
                Abad = CW.masked(A, uplo)
                if j is None:
                    Abad[np.diag_indices(n)] = np.nan
                else:
                    Abad[j, j] = -1.0
                D = el.DistMatrix(g, el.F64, height=n, width=n)
                D.set_local(Abad)
                with pytest.raises(el.NonHPDMatrixError, match="A was not numerically HPD") as ei:
                    el.Cholesky(uplo, D)
                col = ei.value.column
                if j is None:
                    assert col == 1
                else:
                    assert 1 <= col <= j + 1
                    if j == 0:
                        assert col == 1
                _driver_case(el.F64, uplo, n, 9)
    finally:
        el.SetBlocksize(nb0)


def test_cholesky_argument_checks():
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, height=6, width=5)
    with pytest.raises(L.LogicError, match="A must be square"):
        el.Cholesky(el.LOWER, A)
    H = el.DistMatrix(g, el.BF16, height=4, width=4)
    with pytest.raises(L.LogicError, match="Cholesky: only float and double are supported"):
        el.Cholesky(el.LOWER, H)
    t = torch.zeros(64, dtype=torch.float64).cuda()
    p = t.data_ptr()
    with pytest.raises(L.LogicError, match="Cholesky: only float and double are supported"):
        L.call("elx_matrix_cholesky", el.BF16, el.GPU, el.LOWER, 4, p, 4, None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_cholesky", el.F64, el.GPU, el.LOWER, 4, p, 3, None)
    L.call("elx_device_synchronize")
    assert (t.cpu().numpy() == 0).all()  # nothing was launched


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_cholesky_solve_after(dtype):
    """CholeskySolveAfter, n = 300 with 40 right-hand sides, NORMAL: ||X - A^-1 B||_oo
    <= 100 eps n ||B||_1, the reference's own threshold (tests/lapack_like/
    Cholesky.cpp:39-43, relErr > 100 fails); A^-1 B from numpy in float64."""
    npdt = NPDT[dtype]
    n, nrhs = 300, 40
    nb0 = el.Blocksize()
    el.SetBlocksize(128)
    try:
        B0 = oracle.hash_matrix(n, nrhs, 12, 0.0, 1.0, npdt)
        g = el.Grid()
        for uplo in BOTH_UPLO:
            A, D = _driver_case(dtype, uplo, n, 11, g)
            X = np.linalg.solve(A.astype(np.float64), B0.astype(np.float64))
            B = el.DistMatrix(g, dtype, height=n, width=nrhs)
            B.set_local(B0)
            el.CholeskySolveAfter(uplo, el.NORMAL, D, B)
            err = np.abs(B.get_local().astype(np.float64) - X).sum(axis=1).max()
            bound = 100 * np.finfo(npdt).eps * n * np.abs(B0.astype(np.float64)).sum(axis=0).max()
            print(f"solve_after {'LU'[uplo]}: {err:.3g} <= {bound:.3g}")
            assert err <= bound
    finally:
        el.SetBlocksize(nb0)


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1), (4, 2)])
def test_gpu_cholesky_distributed(world, height):
    """El::Cholesky LOWER / UPPER (n = 45, nb = 16: a ragged last block, two levels
    of the recursive split), host-staged ranks; each rank checks its local block
    against numpy's factor and the not-HPD case."""
    _spawn(CW.cholesky_worker, world, height, el.GPU, el.F64, 45, 16, 41)
