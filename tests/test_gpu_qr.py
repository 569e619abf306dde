"""El::QR on the GPU: the multi-workgroup panel kernel (geqrf.hip) through
elx_matrix_qr, the column recursion above it, the special inputs, ApplyQ,
Explicit, the solves and the distributed drivers.

Inputs: hash_matrix in [-1, 1] rounded to the type.  Acceptance
(_qr_workers.accept): Q rebuilt in float64 from the packed reflectors; finite,
d = +-1, diag(R) >= 0, 1 <= t <= 2, |t (1 + |u|^2) - 2| <= 10 m eps,
||A - Q R||_F <= 10 max(m, n) eps ||A||_F, ||Q^T Q - I||_F <= 10 max(m, n) eps."""
import random
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import _qr_workers as QW
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPDT = {el.F64: np.float64, el.F32: np.float32}
BOTH_TYPES = [el.F64, el.F32]


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


def _w():
    return int(L.lib().elx_qr_leaf_cols())


def _r():
    return int(L.lib().elx_qr_leaf_rows())


def _matrix_qr(dtype, A, pad=False):
    """elx_matrix_qr on the column-major A with lda = m (aligned) or m + 3 and the
    base one element into the allocation (pad); everything around the matrix is
    NaN, tau and sig have a guard word on either side.  Returns (packed, t, d) after
    checking that nothing outside the matrix, tau and sig changed."""
    m, n = A.shape
    k = min(m, n)
    es = A.dtype.itemsize
    lda, off = (m + 3, 1) if pad else (m, 0)
    buf = np.full(off + lda * n, np.nan, A.dtype)
    buf[off:].reshape(n, lda)[:, :m] = A.T
    t = torch.from_numpy(buf).cuda()
    tau = torch.from_numpy(np.full(k + 2, -7, A.dtype)).cuda()
    sig = torch.from_numpy(np.full(k + 2, -7, A.dtype)).cuda()
    torch.cuda.synchronize()
    L.call("elx_matrix_qr", dtype, el.GPU, m, n, t.data_ptr() + off * es, lda, tau.data_ptr() + es,
           sig.data_ptr() + es, None)
    L.call("elx_device_synchronize")
    out = t.cpu().numpy()
    inside = np.zeros(buf.shape, bool)
    inside[off:].reshape(n, lda)[:, :m] = True
    assert np.array_equal(_bits(out[~inside]), _bits(buf[~inside])), "written outside the matrix"
    th, dh = tau.cpu().numpy(), sig.cpu().numpy()
    assert th[0] == -7 and th[-1] == -7 and dh[0] == -7 and dh[-1] == -7, "written outside tau / sig"
    return np.asfortranarray(out[off:].reshape(n, lda)[:, :m].T), th[1:-1].copy(), dh[1:-1].copy()


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_qr_leaf_kernel(dtype):
    """The leaf alone (n <= w): m on every edge of the rows-per-workgroup chunk, n on
    every edge of the panel width, n > m included; aligned and padded; two runs on
    the same input are bit-identical."""
    npdt = NPDT[dtype]
    w, R = _w(), _r()
    bad = []
    for m in (1, 2, w - 1, w, w + 1, R - 1, R, R + 1, 2 * R + 3):
        for n in (1, 2, w - 1, w):
            A = QW.random_matrix(m, n, 1000 + 7 * m + n, npdt)
            first = None
            for pad in (False, True):
                P, t, d = _matrix_qr(dtype, A, pad)
                why, _ = QW.accept(A, P, t, d)
                if why:
                    bad.append((m, n, "padded" if pad else "aligned", why))
                if first is None:
                    first = (P, t, d)
                elif not all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(first, (P, t, d))):
                    bad.append((m, n, "two runs differ"))
    assert not bad, f"{len(bad)} cases: {bad}"


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_qr_recursion(dtype):
    """The column recursion: the first split (17), ragged halves (33 x 31), more than
    one block of reflectors (515), tall, wide (the n > m tail) and more than two
    workgroups per leaf."""
    npdt = NPDT[dtype]
    R = _r()
    bad = []
    for (m, n) in [(17, 17), (33, 31), (129, 129), (300, 37), (37, 300), (2 * R + 3, 145), (515, 515)]:
        A = QW.random_matrix(m, n, 2000 + m + n, npdt)
        why, _ = QW.accept(A, *_matrix_qr(dtype, A, m % 2 == 1))
        if why:
            bad.append((m, n, why))
    assert not bad, bad


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_qr_special_inputs(dtype):
    """On the leaf and across a leaf boundary: an exactly zero column at 0, w and
    n - 1 gives t = 2, diagonal 0, d = +1; inputs scaled by 2^+-600 (f64) / 2^+-80
    (f32) pass the whole acceptance."""
    npdt = NPDT[dtype]
    w, R = _w(), _r()
    for (m, n) in ((2 * R + 3, w), (300, 37)):
        for c in sorted({0, min(w, n - 1), n - 1}):
            A = QW.random_matrix(m, n, 5 + c, npdt)
            A[:, c] = 0
            P, t, d = _matrix_qr(dtype, A)
            assert t[c] == 2 and P[c, c] == 0 and d[c] == 1, (m, n, c, t[c], P[c, c], d[c])
            why, _ = QW.accept(A, P, t, d)
            assert why is None, (m, n, c, why)
        A = QW.random_matrix(m, n, 9, npdt)
        A[1:, 0] = 0
        A[0, 0] = -0.75
        P, t, d = _matrix_qr(dtype, A)
        assert t[0] == 2 and P[0, 0] == 0.75 and d[0] == 1, (t[0], P[0, 0], d[0])
        assert QW.accept(A, P, t, d)[0] is None
        for up in (True, False):
            A = QW.scaled_input(m, n, 21, npdt, up)
            why, _ = QW.accept(A, *_matrix_qr(dtype, A))
            assert why is None, (m, n, up, why)


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_qr_nan_propagates(dtype):
    """A NaN at row 0 of the second workgroup, in column c: column c and, from row c
    down, every column right of it become NaN; the columns left of it are bit for
    bit the factorization of the left part alone and pass the acceptance; the call
    returns."""
    npdt = NPDT[dtype]
    w, R = _w(), _r()
    for (m, n, c) in ((2 * R + 3, w, 5), (300, 37, 3), (300, 37, 20)):
        A = QW.random_matrix(m, n, 3 + c, npdt)
        A[R, c] = np.nan
        P, t, d = _matrix_qr(dtype, A)
        assert np.isnan(P[:, c]).all() and np.isnan(P[c:, c:]).all() and np.isnan(t[c:]).all(), (m, n, c)
        if c < w:  # inside the first leaf: the columns left of c never see column c
            left = np.asfortranarray(A[:, :c])
            Pl, tl, dl = _matrix_qr(dtype, left)
            assert np.array_equal(_bits(np.asfortranarray(P[:, :c])), _bits(Pl)), (m, n, c)
            assert np.array_equal(_bits(t[:c]), _bits(tl)) and np.array_equal(_bits(d[:c]), _bits(dl))
            assert QW.accept(left, Pl, tl, dl)[0] is None
        else:  # the first leaf is complete before column c is touched
            left = np.asfortranarray(A[:, :w])
            assert QW.accept(left, np.asfortranarray(P[:, :w]), t[:w], d[:w])[0] is None


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("shape", [(70, 70), (515, 130), (130, 515)])
def test_qr_drivers(dtype, shape):
    """el.QR, QRApplyQ, QRExplicit and QRExplicitTriang on a 1 x 1 grid; QRSolveAfter
    in both orientations and LeastSquares where m >= n."""
    g = el.Grid()
    A = QW.random_matrix(*shape, shape[0] + shape[1], NPDT[dtype])
    QW.check_apply_and_explicit(el, g, dtype, el.GPU, A)
    if shape[0] >= shape[1]:
        QW.check_solves(el, g, dtype, el.GPU, A)


def test_qr_argument_checks():
    g = el.Grid()

    def dm(m, n, dtype=el.F64, seed=1):
        D = el.DistMatrix(g, dtype, height=m, width=n)
        if dtype in NPDT:
            D.set_local(QW.random_matrix(m, n, seed, NPDT[dtype]))
        return D
    A = dm(6, 4)
    t, d = el.QR(A)
    B, X = dm(6, 2), dm(1, 1)
    with pytest.raises(L.LogicError, match="ApplyQ: only LEFT is supported"):
        el.QRApplyQ(el.RIGHT, el.NORMAL, A, t, d, B)
    with pytest.raises(L.LogicError, match="A and B do not conform"):
        el.QRSolveAfter(el.NORMAL, A, t, d, dm(4, 2), X)
    W = dm(4, 6)
    tw, dw = el.QR(W)
    with pytest.raises(L.LogicError, match="Must have full column rank"):
        el.QRSolveAfter(el.NORMAL, W, tw, dw, dm(4, 2), X)
    with pytest.raises(L.UnsupportedError):
        el.LeastSquares(el.NORMAL, dm(4, 6), dm(4, 2), X)
    with pytest.raises(L.LogicError, match="QR: only float and double are supported"):
        el.QR(dm(4, 4, el.BF16))
    buf = torch.zeros(64, dtype=torch.float64).cuda()
    with pytest.raises(L.LogicError, match="QR: only float and double are supported"):
        L.call("elx_matrix_qr", el.BF16, el.GPU, 4, 4, buf.data_ptr(), 4, buf.data_ptr() + 256, buf.data_ptr() + 384,
               None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_qr", el.F64, el.GPU, 4, 4, buf.data_ptr(), 3, buf.data_ptr() + 256, buf.data_ptr() + 384,
               None)
    L.call("elx_device_synchronize")
    assert (buf.cpu().numpy() == 0).all()  # nothing was launched


def _need_gpus(world):
    return pytest.mark.skipif(el.device_count() < world, reason=f"needs >= {world} GPUs (one RCCL rank per GPU)")


@pytest.mark.parametrize("world,height", [pytest.param(2, 1, marks=_need_gpus(2)),
                                          pytest.param(2, 2, marks=_need_gpus(2))])
def test_gpu_qr_rccl(world, height):
    """The distributed driver over RCCL on 1 x 2 and 2 x 1 grids, 150 x 150 and
    150 x 60, nb = 32: the panel staging and the block reflector on views."""
    import os
    os.environ["ELX_TEST_BACKEND"] = "rccl"
    try:
        mp.spawn(QW.qr_worker, args=(world, _port(), height, el.GPU, el.F64, [(150, 150), (150, 60)], 32, 51),
                 nprocs=world, join=True)
    finally:
        os.environ.pop("ELX_TEST_BACKEND", None)


def test_gpu_qr_host_staged_grid():
    """The same driver on a 2 x 2 grid of ranks sharing one GPU (host-staged
    collectives), nb = 16."""
    mp.spawn(QW.qr_worker, args=(4, _port(), 2, el.GPU, el.F64, [(45, 45), (45, 20)], 16, 53), nprocs=4, join=True)
