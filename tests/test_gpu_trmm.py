"""El::Trmm on the GPU: the triangle-aware MFMA kernel (trmm.hip) through
elx_matrix_trmm, the argument checks, and the distributed driver."""
import random
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import _trmm_workers as TW
import oracle
from _trmm_workers import masked_triangle, trmm_ref
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPDT = {el.F64: np.float64, el.F32: np.float32}


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


def _padded(X, ld, off):
    """Device tensor holding the column-major X with leading dimension ld, `off`
    elements into the allocation; returns (tensor, pointer to X(0,0))."""
    rows, cols = X.shape
    buf = np.full(off + ld * cols, np.nan, X.dtype)  # the padding must not be read either
    buf[off:].reshape(cols, ld)[:, :rows] = X.T
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + off * X.dtype.itemsize


def _unpad(t, shape, ld, off):
    rows, cols = shape
    return t.cpu().numpy()[off:].reshape(cols, ld)[:, :rows].T


def _exact_case(dtype, side, uplo, orient, diag, m, n, pad):
    """One integer-valued case (A in [-3,3], B in [-4,4], alpha 2: every partial
    sum below 2^12, exact in f32 and f64).  Returns None or what went wrong."""
    npdt = NPDT[dtype]
    k = m if side == el.LEFT else n
    rng = np.random.default_rng(1000 * m + n)
    A0 = rng.integers(-3, 4, (k, k)).astype(npdt)
    B0 = rng.integers(-4, 5, (m, n)).astype(npdt)
    A = masked_triangle(A0, uplo, diag)
    want = trmm_ref(side, uplo, orient, diag, 2.0, A, B0)
    lda, ldb, off = (k + 3, m + 1, 1) if pad else (k, m, 0)
    tA, pA = _padded(A, lda, off)
    tB, pB = _padded(B0, ldb, off)
    torch.cuda.synchronize()
    L.call("elx_matrix_trmm", dtype, el.GPU, side, uplo, orient, diag, m, n, 2.0, pA, lda, pB, ldb, None)
    L.call("elx_device_synchronize")
    got = _unpad(tB, (m, n), ldb, off).astype(np.float64)
    if not np.isfinite(got).all():
        return "not finite"
    if not np.array_equal(got, want):
        return f"{int((got != want).sum())} of {m * n} entries differ"
    return None


KERNEL_SHAPES = [(1, 1), (15, 3), (16, 16), (17, 5), (127, 9), (128, 130), (129, 17), (257, 33), (300, 1)]


def _run_exact(side, shapes):
    bad = []
    for dtype in (el.F64, el.F32):
        for uplo in (el.LOWER, el.UPPER):
            for orient in (el.NORMAL, el.TRANSPOSE):
                for diag in (el.NON_UNIT, el.UNIT):
                    for (m, n) in shapes:
                        for pad in (False, True):
                            why = _exact_case(dtype, side, uplo, orient, diag, m, n, pad)
                            if why:
                                bad.append((("f32", "f64")[dtype], "LU"[uplo], "NT"[orient], "NU"[diag], m, n,
                                            "padded" if pad else "aligned", why))
    assert not bad, f"{len(bad)} cases: {bad}"


def test_trmm_kernel_exact():
    """trmm_tri through elx_matrix_trmm (LEFT): sizes around the 16-slab, the 16x16
    MFMA tile and the 128 / 256 row-tile edges, so the diagonal crosses slabs at
    every offset; aligned (lda = ldb = m) and misaligned (lda = m + 3, ldb = m + 1,
    bases one element in).  The unread triangle (and a UNIT diagonal) is NaN."""
    _run_exact(el.LEFT, KERNEL_SHAPES)


def test_trmm_matrix_right_exact():
    """side = RIGHT of the Matrix entry: B := 2 B op(tri(A)) through the transposes."""
    _run_exact(el.RIGHT, [(33, 129), (130, 17)])


def test_trmm_argument_checks():
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, height=6, width=5)
    B = el.DistMatrix(g, el.F64, height=6, width=4)
    with pytest.raises(L.LogicError, match="Triangular matrix must be square"):
        el.Trmm(el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 1.0, A, B)
    A = el.DistMatrix(g, el.F64, height=5, width=5)
    with pytest.raises(L.LogicError, match="Nonconformal Trmm"):
        el.Trmm(el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 1.0, A, B)
    with pytest.raises(L.LogicError, match="Nonconformal Trmm"):
        el.Trmm(el.RIGHT, el.LOWER, el.NORMAL, el.NON_UNIT, 1.0, A, B)
    t = torch.zeros(64, dtype=torch.float64).cuda()
    p = t.data_ptr()
    with pytest.raises(L.LogicError, match="only float and double"):
        L.call("elx_matrix_trmm", el.BF16, el.GPU, el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 4, 4, 1.0, p, 4, p + 128,
               4, None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_trmm", el.F64, el.GPU, el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 4, 4, 1.0, p, 3, p + 128,
               4, None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_trmm", el.F64, el.GPU, el.RIGHT, el.LOWER, el.NORMAL, el.NON_UNIT, 3, 4, 1.0, p, 3, p + 128,
               3, None)
    L.call("elx_device_synchronize")
    assert (t.cpu().numpy() == 0).all()  # nothing was launched


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1), (4, 2)])
def test_gpu_trmm_distributed(world, height):
    """El::Trmm, all 16 side/uplo/orientation/diag cases (m = 45, n = 23, nb = 16:
    ragged blocks, three levels of the recursive split), host-staged ranks."""
    _spawn(TW.trmm_worker, world, height, el.GPU, el.F64, 45, 23, 16, 41)


def test_gpu_trmm_distributed_f32():
    _spawn(TW.trmm_worker, 1, 1, el.GPU, el.F32, 45, 23, 16, 43)


@pytest.mark.parametrize("dtype", [el.F64, el.F32])
@pytest.mark.parametrize("m,n", [(700, 300), (2100, 1100)])
def test_gpu_trmm_large(dtype, m, n):
    """1x1 grid, default Blocksize: m = 700 recurses over six 128-row leaves (a
    ragged last one) with the updates as direct GEMMs; m = 2100 takes the widened
    512-row leaves (four and a ragged 52).  LEFT, LOWER / UPPER x NORMAL / TRANSPOSE."""
    npdt = NPDT[dtype]
    g = el.Grid()
    el.SetBlocksize(128)
    Bg = oracle.hash_matrix(m, n, 52, -1.0, 1.0, npdt)
    for uplo in (el.LOWER, el.UPPER):
        Ag = masked_triangle(oracle.hash_matrix(m, m, 51, -1.0, 1.0, npdt), uplo, el.NON_UNIT)
        for orient in (el.NORMAL, el.TRANSPOSE):
            A = el.DistMatrix(g, dtype, height=m, width=m)
            B = el.DistMatrix(g, dtype, height=m, width=n)
            A.set_local(Ag)
            B.set_local(Bg)
            el.Trmm(el.LEFT, uplo, orient, el.NON_UNIT, 0.75, A, B)
            got = B.get_local().astype(np.float64)
            ref = trmm_ref(el.LEFT, uplo, orient, el.NON_UNIT, 0.75, Ag, Bg)
            err = np.linalg.norm(got - ref) / (np.linalg.norm(ref) * m * np.finfo(npdt).eps)
            assert np.isfinite(got).all() and err <= 10, (uplo, orient, err)


def test_gpu_trmm_triangle_on_cpu():
    """The triangle on the CPU and B on the GPU: A is proxied to B's device."""
    m, n = 70, 40
    g = el.Grid()
    el.SetBlocksize(16)
    try:
        Ag = masked_triangle(oracle.hash_matrix(m, m, 61, -1.0, 1.0, np.float64), el.LOWER, el.NON_UNIT)
        Bg = oracle.hash_matrix(m, n, 62, -1.0, 1.0, np.float64)
        A = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=m, width=m)
        B = el.DistMatrix(g, el.F64, el.MC, el.MR, el.GPU, height=m, width=n)
        A.set_local(Ag)
        B.set_local(Bg)
        el.Trmm(el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 0.75, A, B)
        got = B.get_local()
        ref = trmm_ref(el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 0.75, Ag, Bg)
        assert np.isfinite(got).all()
        assert np.linalg.norm(got - ref) <= 10 * np.linalg.norm(ref) * m * np.finfo(np.float64).eps
    finally:
        el.SetBlocksize(128)
