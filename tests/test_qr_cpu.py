"""El::QR without a GPU: the distributed driver on Device::CPU matrices over gloo
(the host column loop of qr::PanelHouseholder in the leaves), ApplyQ, Explicit,
SolveAfter, LeastSquares, the special inputs, the argument checks and the drop-in
C++ surface."""
import os
import random
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import _qr_workers as QW
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [(19, 19), (23, 11), (11, 23)]
HOST_SHAPES = [(1, 1), (5, 3), (16, 16), (17, 17), (33, 31), (129, 129), (300, 37), (37, 300)]
NPDT = {el.F64: np.float64, el.F32: np.float32}


def _port():
    """A free rendezvous port below the kernel's ephemeral range (see test_dist_cpu)."""
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


def _matrix_qr(npdt, A, pad=False, device=el.CPU):
    """elx_matrix_qr on the column-major A on the host, lda = m or m + 3 with NaN
    around the matrix; tau and sig have a guard word on either side."""
    m, n = A.shape
    k = min(m, n)
    lda = m + 3 if pad else m
    buf = np.full((n, lda), np.nan, npdt)  # row q of buf = column q of the matrix
    buf[:, :m] = A.T
    tau, sig = np.full(k + 2, -7, npdt), np.full(k + 2, -7, npdt)
    L.call("elx_matrix_qr", el.F64 if npdt == np.float64 else el.F32, device, m, n, buf.ctypes.data, lda,
           tau[1:].ctypes.data, sig[1:].ctypes.data, None)
    assert np.isnan(buf[:, m:]).all(), "written outside the matrix"
    assert tau[0] == -7 and tau[-1] == -7 and sig[0] == -7 and sig[-1] == -7, "written outside tau / sig"
    return np.asfortranarray(buf[:, :m].T), tau[1:-1].copy(), sig[1:-1].copy()


def test_reference_meets_the_bounds():
    """The bounds are reachable: LAPACK's f64 QR, and a plain numpy restatement of
    the unblocked algorithm in each type, pass the acceptance at every shape the QR
    tests use; numpy's lstsq meets both solve bounds on the solve inputs."""
    R, w = 256, 16
    shapes = set(HOST_SHAPES + RAGGED + [(2 * R + 3, 145), (515, 515), (70, 70), (515, 130), (130, 515), (150, 150),
                                         (150, 60), (45, 45), (45, 20), (37, 20)])
    shapes |= {(m, n) for m in (1, 2, w - 1, w, w + 1, R - 1, R, R + 1, 2 * R + 3) for n in (1, 2, w - 1, w)}
    for (m, n) in sorted(shapes):
        for npdt in (np.float64, np.float32):
            A = QW.random_matrix(m, n, 100 + m + n, npdt)
            why, _ = QW.accept(A, *QW.unblocked_reference(A))
            assert why is None, (m, n, npdt.__name__, why)
        A = QW.random_matrix(m, n, 100 + m + n, np.float64)
        k = min(m, n)
        Q, Rm = np.linalg.qr(A, mode="complete")
        eps = np.finfo(np.float64).eps
        # LAPACK against the acceptance's own bounds (at the larger shapes it stays
        # under 0.12 and 0.6 of the bare max(m, n) eps; a 2 x 1 input reaches 0.32)
        assert np.linalg.norm(A - Q[:, :k] @ Rm[:k]) <= 10 * max(m, n) * eps * np.linalg.norm(A)
        assert np.linalg.norm(Q.T @ Q - np.eye(m)) <= 10 * max(m, n) * eps
    for (m, n) in [(37, 20), (70, 70), (515, 130)]:
        A = QW.random_matrix(m, n, 41, np.float64)
        B = QW.random_matrix(m, QW.NRHS, 11 + m, np.float64)
        C = QW.random_matrix(n, QW.NRHS, 13 + n, np.float64)
        assert QW.check_least_squares(A, B, np.linalg.lstsq(A, B, rcond=None)[0]) is None
        Q = np.linalg.qr(A, mode="complete")[0]
        assert QW.check_min_norm(A, C, np.linalg.lstsq(A.T, C, rcond=None)[0], Q) is None


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1), (4, 2), (8, 2)])
def test_qr(world, height):
    """El::QR, ApplyQ, Explicit and ExplicitTriang on ragged shapes with nb = 4 (the
    last panel ragged, m < n included).  Every grid's result goes through the
    acceptance; bit-identity with the 1 x 1 result is NOT asserted (its panel
    boundaries differ, see qr_worker)."""
    mp.spawn(QW.qr_worker, args=(world, _port(), height, el.CPU, el.F64, RAGGED, 4, 31), nprocs=world, join=True)


def test_qr_f32():
    mp.spawn(QW.qr_worker, args=(4, _port(), 2, el.CPU, el.F32, RAGGED, 4, 37), nprocs=4, join=True)


@pytest.mark.parametrize("dtype", [el.F64, el.F32])
def test_qr_solves_2x2(dtype):
    """QRSolveAfter NORMAL / TRANSPOSE / ADJOINT and LeastSquares at 37 x 20 on a
    2 x 2 grid with nb = 8."""
    mp.spawn(QW.solve_worker, args=(4, _port(), 2, el.CPU, dtype, 37, 20, 8, 41), nprocs=4, join=True)


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
def test_matrix_qr_cpu(npdt):
    """The local driver on the host: the leaf alone (n <= 16), every split of the
    recursion, tall and wide, lda = m and m + 3, guard words untouched."""
    bad = []
    for (m, n) in HOST_SHAPES:
        A = QW.random_matrix(m, n, 100 + m + n, npdt)
        for pad in (False, True):
            why, _ = QW.accept(A, *_matrix_qr(npdt, A, pad))
            if why:
                bad.append((m, n, pad, why))
    assert not bad, bad


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
def test_qr_cpu_special_inputs(npdt):
    """An exactly zero column: t = 2, diagonal 0, d = +1.  A column that is zero
    below the diagonal with a negative alpha ends with a positive diagonal.  Inputs
    scaled by 2^+-600 (f64) / 2^+-80 (f32), where a plain sum of squares gives
    Inf / 0, pass the whole acceptance."""
    for (m, n) in ((40, 12), (300, 37)):
        for c in (0, min(16, n - 1), n - 1):
            A = QW.random_matrix(m, n, 5 + c, npdt)
            A[:, c] = 0  # stays exactly zero under the earlier reflectors
            P, t, d = _matrix_qr(npdt, A)
            assert t[c] == 2 and P[c, c] == 0 and d[c] == 1, (m, n, c, t[c], P[c, c], d[c])
            why, _ = QW.accept(A, P, t, d)
            assert why is None, (m, n, c, why)
        A = QW.random_matrix(m, n, 9, npdt)
        A[1:, 0] = 0
        A[0, 0] = -0.75
        P, t, d = _matrix_qr(npdt, A)
        assert t[0] == 2 and P[0, 0] == 0.75 and d[0] == 1, (t[0], P[0, 0], d[0])
        assert QW.accept(A, P, t, d)[0] is None
        A[0, 0] = 0.75  # beta = -alpha < 0: the signature flips the row
        P, t, d = _matrix_qr(npdt, A)
        assert t[0] == 2 and P[0, 0] == 0.75 and d[0] == -1, (t[0], P[0, 0], d[0])
        assert QW.accept(A, P, t, d)[0] is None
        for up in (True, False):
            A = QW.scaled_input(m, n, 21, npdt, up)
            with np.errstate(over="ignore", under="ignore"):
                plain = np.sum(A[:, 0] * A[:, 0])
            assert np.isinf(plain) or plain == 0
            why, _ = QW.accept(A, *_matrix_qr(npdt, A))
            assert why is None, (m, n, up, why)


def test_qr_cpu_nan_propagates():
    """A NaN reaches its own column and the columns right of it; the columns left
    of it are the factorization of the left part alone."""
    m, n, c = 40, 20, 7
    A = QW.random_matrix(m, n, 3, np.float64)
    A[25, c] = np.nan
    P, t, d = _matrix_qr(np.float64, A)
    Pl, tl, dl = _matrix_qr(np.float64, np.asfortranarray(A[:, :c]))
    assert np.array_equal(_bits(np.asfortranarray(P[:, :c])), _bits(Pl)) and np.array_equal(t[:c], tl)
    assert QW.accept(np.asfortranarray(A[:, :c]), Pl, tl, dl)[0] is None
    assert np.isnan(P[:, c]).all() and np.isnan(P[c:, c:]).all() and np.isnan(t[c:]).all()


def test_qr_cpu_argument_checks():
    g = el.Grid()

    def dm(m, n, dtype=el.F64, seed=1):
        D = el.DistMatrix(g, dtype, el.MC, el.MR, el.CPU, height=m, width=n)
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
    with pytest.raises(L.LogicError, match="A and B do not conform"):
        el.QRSolveAfter(el.ADJOINT, A, t, d, B, X)
    W = dm(4, 6)
    tw, dw = el.QR(W)
    with pytest.raises(L.LogicError, match="Must have full column rank"):
        el.QRSolveAfter(el.NORMAL, W, tw, dw, dm(4, 2), X)
    with pytest.raises(L.UnsupportedError):
        el.LeastSquares(el.NORMAL, dm(4, 6), dm(4, 2), X)
    H = dm(4, 4, el.BF16)
    with pytest.raises(L.LogicError, match="QR: only float and double are supported"):
        el.QR(H)
    buf, tau, sig = np.zeros(16), np.zeros(4), np.zeros(4)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_qr", el.F64, el.CPU, 4, 4, buf.ctypes.data, 3, tau.ctypes.data, sig.ctypes.data, None)
    with pytest.raises(L.LogicError, match="QR: only float and double are supported"):
        L.call("elx_matrix_qr", el.BF16, el.CPU, 4, 4, buf.ctypes.data, 4, tau.ctypes.data, sig.ctypes.data, None)
    assert (buf == 0).all() and (tau == 0).all() and (sig == 0).all()
    assert int(L.lib().elx_qr_leaf_cols()) == 16 and int(L.lib().elx_qr_leaf_rows()) == 256


def _build_and_run(tmp_path, name, extra=()):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o",
                           str(exe), "-L", libdir, "-lelemental_amd", f"-Wl,-rpath,{libdir}"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "OK" in res.stdout


def test_cpp_qr_api(tmp_path):
    """El::QR on Matrix and DistMatrix, qr::ApplyQ, SolveAfter, Explicit,
    ExplicitTriang and LeastSquares through include/El.hpp, Device::CPU, against a
    hand-computed 3 x 2 case."""
    _build_and_run(tmp_path, "test_qr_api")


def test_cpp_qr_host_shapes(tmp_path):
    """The stand-alone program over the C ABI (its own main; it can be linked
    against a sanitized host build by hand): the CPU LocalQR code on the test shapes."""
    _build_and_run(tmp_path, "qr_host_check")
