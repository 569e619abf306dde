"""El::TriangularInverse / El::Trtrmm / El::HPDInverse on the GPU: the in-LDS leaf
kernels (trtri.hip) through the elx_matrix_* entry points, an exact integer case,
the blocked drivers on a 1x1 grid, the not-HPD path, the argument checks and the
distributed drivers.  Inputs and bounds: _inverse_workers."""
import random
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import _cholesky_workers as CW
import _inverse_workers as IW
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPDT = {el.F64: np.float64, el.F32: np.float32}
BOTH_TYPES = [el.F64, el.F32]
BOTH_UPLO = [el.LOWER, el.UPPER]
LEAF_SIZES = (1, 2, 15, 16, 17, 31, 33, 63, 65, 127, 128)


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


def _matrix_call(name, dtype, Xin, pad, *head):
    """elx_matrix_<name> on the column-major Xin with lda = n (aligned) or n + 3 and
    the base one element into the allocation (pad); everything around the matrix is
    NaN.  Returns the result, after checking that nothing outside the n x n matrix
    changed."""
    n = Xin.shape[0]
    lda, off = (n + 3, 1) if pad else (n, 0)
    buf = np.full(off + lda * n, np.nan, Xin.dtype)
    buf[off:].reshape(n, lda)[:, :n] = Xin.T
    t = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    L.call(name, dtype, el.GPU, *head, n, t.data_ptr() + off * Xin.dtype.itemsize, lda, None)
    L.call("elx_device_synchronize")
    out = t.cpu().numpy()
    inside = np.zeros(buf.shape, bool)
    inside[off:].reshape(n, lda)[:, :n] = True
    assert np.array_equal(_bits(out[~inside]), _bits(buf[~inside])), "written outside the matrix"
    return out[off:].reshape(n, lda)[:, :n].T


def test_leaf_is_one_block():
    """The leaf sizes below are single launches only if the leaf holds 128 rows."""
    assert int(L.lib().elx_cholesky_leaf_max()) == max(LEAF_SIZES)


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_trtri_leaf_kernel(dtype):
    """trtri_kernel alone (n <= 128 is one leaf): one diagonal block, the 16 / 32 / 64
    levels with ragged last blocks, LOWER and UPPER, NON_UNIT and UNIT, aligned and
    misaligned."""
    npdt = NPDT[dtype]
    bad = []
    for n in LEAF_SIZES:
        A = CW.hpd_matrix(n, 100 + n, npdt)
        for uplo in BOTH_UPLO:
            for unit in (False, True):
                T = IW.triangle(A, uplo, unit)
                Tin = IW.fed(T, uplo, unit)
                for pad in (False, True):
                    got = _matrix_call("elx_matrix_triangular_inverse", dtype, Tin, pad, uplo,
                                       el.UNIT if unit else el.NON_UNIT)
                    why, _ = IW.accept_trtri(T, Tin, got, uplo, unit)
                    if why:
                        bad.append((n, "LU"[uplo], "unit" if unit else "non-unit", "padded" if pad else "aligned", why))
    assert not bad, f"{len(bad)} cases: {bad}"


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_lauum_leaf_kernel(dtype):
    """lauum_kernel alone: 1 to 36 tiles, LOWER and UPPER, aligned and misaligned."""
    npdt = NPDT[dtype]
    bad = []
    for n in LEAF_SIZES:
        A = CW.hpd_matrix(n, 100 + n, npdt)
        for uplo in BOTH_UPLO:
            T = IW.triangle(A, uplo)
            Tin = IW.fed(T, uplo)
            for pad in (False, True):
                why, _ = IW.accept_trtrmm(T, Tin, _matrix_call("elx_matrix_trtrmm", dtype, Tin, pad, uplo), uplo)
                if why:
                    bad.append((n, "LU"[uplo], "padded" if pad else "aligned", why))
    assert not bad, f"{len(bad)} cases: {bad}"


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_hpd_inverse_leaf_kernels(dtype):
    """The three leaves in a row on one block (elx_matrix_hpd_inverse, n <= 128)."""
    npdt = NPDT[dtype]
    bad = []
    for n in LEAF_SIZES:
        A = CW.hpd_matrix(n, 100 + n, npdt)
        for uplo in BOTH_UPLO:
            Ain = CW.masked(A, uplo)
            for pad in (False, True):
                got = _matrix_call("elx_matrix_hpd_inverse", dtype, Ain, pad, uplo)
                why, _ = IW.accept_hpd_inverse(A, Ain, got, uplo)
                if why:
                    bad.append((n, "LU"[uplo], "padded" if pad else "aligned", why))
    assert not bad, f"{len(bad)} cases: {bad}"


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("n", [5, 17, 40])
def test_leaf_integer(dtype, n):
    """L0 integer lower (off the diagonal in [-2, 2], diagonal in {1, 2, 4}): Trtrmm
    must equal L0^T L0 (U0 U0^T) within the Trtrmm bound; every value is a small
    integer, so the products are in fact exact.  The inverse of the same L0 meets the
    residual bound."""
    npdt = NPDT[dtype]
    rng = np.random.default_rng(n)
    L0 = np.tril(rng.integers(-2, 3, (n, n)), -1).astype(np.float64)
    L0[np.diag_indices(n)] = rng.choice([1.0, 2.0, 4.0], n)
    for uplo in BOTH_UPLO:
        T = np.asfortranarray((L0 if uplo == el.LOWER else L0.T).astype(npdt))
        Tin = IW.fed(T, uplo)
        got = _matrix_call("elx_matrix_trtrmm", dtype, Tin, False, uplo)
        why, _ = IW.accept_trtrmm(T, Tin, got, uplo)
        assert why is None, why
        err = np.linalg.norm(IW.clean(got, uplo) - np.where(CW.other_triangle(n, uplo), 0.0, IW.trtrmm_want(T, uplo)))
        print(f"integer n={n}: ||tri(got - L0^T L0)||_F = {err:.3g}")
        assert err <= 10 * n * np.finfo(npdt).eps * np.linalg.norm(L0) ** 2
        got = _matrix_call("elx_matrix_triangular_inverse", dtype, Tin, False, uplo, el.NON_UNIT)
        why, _ = IW.accept_trtri(T, Tin, got, uplo, False)
        assert why is None, why


def _driver_cases(dtype, uplo, n, seed, g=None):
    """All three functions on a 1x1-grid DistMatrix."""
    npdt = NPDT[dtype]
    g = g or el.Grid()
    A = CW.hpd_matrix(n, seed, npdt)

    def run(fn, Xin):
        D = el.DistMatrix(g, dtype, height=n, width=n)
        D.set_local(Xin)
        fn(D)
        return D.get_local()

    for unit in (False, True):
        T = IW.triangle(A, uplo, unit)
        Tin = IW.fed(T, uplo, unit)
        diag = el.UNIT if unit else el.NON_UNIT
        why, _ = IW.accept_trtri(T, Tin, run(lambda D: el.TriangularInverse(uplo, diag, D), Tin), uplo, unit)
        assert why is None, (n, uplo, unit, why)
    T = IW.triangle(A, uplo)
    Tin = IW.fed(T, uplo)
    why, _ = IW.accept_trtrmm(T, Tin, run(lambda D: el.Trtrmm(uplo, D), Tin), uplo)
    assert why is None, (n, uplo, why)
    Ain = CW.masked(A, uplo)
    why, _ = IW.accept_hpd_inverse(A, Ain, run(lambda D: el.HPDInverse(uplo, D), Ain), uplo)
    assert why is None, (n, uplo, why)


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("n", [129, 300, 1100])
def test_inverse_drivers(dtype, n):
    """1x1 grid, Blocksize 128: 129 is the first size with two blocks, 300 has a
    ragged last block, 1100 three levels of the recursive split."""
    nb0 = el.Blocksize()
    el.SetBlocksize(128)
    try:
        for uplo in BOTH_UPLO:
            _driver_cases(dtype, uplo, n, 200 + n)
    finally:
        el.SetBlocksize(nb0)


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_inverse_drivers_small_blocks(dtype):
    nb0 = el.Blocksize()
    el.SetBlocksize(32)
    try:
        for uplo in BOTH_UPLO:
            _driver_cases(dtype, uplo, 100, 77)
    finally:
        el.SetBlocksize(nb0)


@pytest.mark.parametrize("sweep", ["0", "256"])
def test_inverse_drivers_sweep_knob(sweep, monkeypatch):
    """ELX_INVERSE_SWEEP=0: the recursive split down to single leaves, every panel a
    Trsm / Syrk / Trmm call on views (the path a grid of more than one rank takes);
    256: n = 300 is cut into a single leaf and a local sweep of two."""
    monkeypatch.setenv("ELX_INVERSE_SWEEP", sweep)
    nb0 = el.Blocksize()
    el.SetBlocksize(128)
    try:
        for uplo in BOTH_UPLO:
            _driver_cases(el.F64, uplo, 300, 500)
    finally:
        el.SetBlocksize(nb0)


def test_hpd_inverse_not_hpd():
    """A negative diagonal entry inside a later leaf (j = 200 of n = 300):
    NonHPDMatrixError with 1 <= column <= j + 1, and a valid call afterwards passes."""
    n, j = 300, 200
    nb0 = el.Blocksize()
    el.SetBlocksize(128)
    try:
        A = CW.hpd_matrix(n, 9, np.float64)
        g = el.Grid()
        for uplo in BOTH_UPLO:
            Abad = CW.masked(A, uplo)
            Abad[j, j] = -1.0
            D = el.DistMatrix(g, el.F64, height=n, width=n)
            D.set_local(Abad)
            with pytest.raises(el.NonHPDMatrixError, match="A was not numerically HPD") as ei:
                el.HPDInverse(uplo, D)
            assert 1 <= ei.value.column <= j + 1
            Ain = CW.masked(A, uplo)
            D.set_local(Ain)
            el.HPDInverse(uplo, D)
            why, _ = IW.accept_hpd_inverse(A, Ain, D.get_local(), uplo)
            assert why is None, why
    finally:
        el.SetBlocksize(nb0)


def test_inverse_argument_checks():
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, height=6, width=5)
    H = el.DistMatrix(g, el.BF16, height=4, width=4)
    calls = {
        "TriangularInverse": lambda D: el.TriangularInverse(el.LOWER, el.NON_UNIT, D),
        "Trtrmm": lambda D: el.Trtrmm(el.LOWER, D),
        "HPDInverse": lambda D: el.HPDInverse(el.LOWER, D),
    }
    for who, fn in calls.items():
        with pytest.raises(L.LogicError, match="A must be square"):
            fn(A)
        with pytest.raises(L.LogicError, match=f"{who}: only float and double are supported"):
            fn(H)
    t = torch.zeros(64, dtype=torch.float64).cuda()
    p = t.data_ptr()
    matrix_calls = {
        "TriangularInverse": ("elx_matrix_triangular_inverse", (el.LOWER, el.NON_UNIT)),
        "Trtrmm": ("elx_matrix_trtrmm", (el.LOWER,)),
        "HPDInverse": ("elx_matrix_hpd_inverse", (el.LOWER,)),
    }
    for who, (name, head) in matrix_calls.items():
        with pytest.raises(L.LogicError, match=f"{who}: only float and double are supported"):
            L.call(name, el.BF16, el.GPU, *head, 4, p, 4, None)
        with pytest.raises(L.LogicError, match="leading dimension"):
            L.call(name, el.F64, el.GPU, *head, 4, p, 3, None)
    L.call("elx_device_synchronize")
    assert (t.cpu().numpy() == 0).all()  # nothing was launched


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1), (4, 2)])
def test_gpu_inverse_distributed(world, height):
    """The three functions, LOWER / UPPER (n = 45, nb = 16: a ragged last block, two
    levels of the recursive split), host-staged ranks; each rank checks its local
    block against numpy's float64 result and the not-HPD case."""
    mp.spawn(IW.inverse_worker, args=(world, _port(), height, el.GPU, el.F64, 45, 16, 41), nprocs=world, join=True)
