"""El::TriangularInverse / El::Trtrmm / El::HPDInverse without a GPU: the distributed
drivers on Device::CPU matrices over gloo (the host loops of LVar3Unb and LUnblocked
in the leaves), the residual acceptance through the Matrix entry points, the
argument checks, and the drop-in C++ surface.  Inputs and bounds: _inverse_workers."""
import os
import random
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import _cholesky_workers as CW
import _inverse_workers as IW
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1), (4, 2)])
def test_inverse_distributed_cpu(world, height):
    """The three functions, LOWER / UPPER (the inverse also UNIT), n = 45 with nb = 16
    (a ragged last block, two levels of the split), the other triangle NaN, every
    rank against numpy; HPDInverse of a non-HPD matrix raises on all ranks."""
    mp.spawn(IW.inverse_worker, args=(world, _port(), height, el.CPU, el.F64, 45, 16, 41), nprocs=world, join=True)


def _matrix_call(name, dtype, Xin, lda, *head):
    """elx_matrix_<name> on the column-major Xin inside a NaN-filled buffer of leading
    dimension lda; returns the result after checking the padding rows."""
    n = Xin.shape[0]
    buf = np.full((n, lda), np.nan, Xin.dtype)  # row q of buf = column q of the matrix
    buf[:, :n] = Xin.T
    L.call(name, dtype, el.CPU, *head, n, buf.ctypes.data, lda, None)
    assert np.isnan(buf[:, n:]).all()
    return buf[:, :n].T


@pytest.mark.parametrize("dtype", [el.F64, el.F32])
@pytest.mark.parametrize("uplo", [el.LOWER, el.UPPER])
def test_matrix_inverse_cpu_residuals(dtype, uplo):
    """The Matrix entry points attach the buffer to a 1x1 DistMatrix: n = 300 runs the
    blocked drivers (three 128-row leaves), lda = n + 3; the residual acceptance of
    _inverse_workers for all three functions, the inverse also UNIT."""
    npdt = NPDT[dtype]
    n, lda = 300, 303
    A = CW.hpd_matrix(n, 8, npdt)
    for unit in (False, True):
        T = IW.triangle(A, uplo, unit)
        Tin = IW.fed(T, uplo, unit)
        got = _matrix_call("elx_matrix_triangular_inverse", dtype, Tin, lda, uplo, el.UNIT if unit else el.NON_UNIT)
        why, _ = IW.accept_trtri(T, Tin, got, uplo, unit)
        assert why is None, why
    T = IW.triangle(A, uplo)
    Tin = IW.fed(T, uplo)
    why, _ = IW.accept_trtrmm(T, Tin, _matrix_call("elx_matrix_trtrmm", dtype, Tin, lda, uplo), uplo)
    assert why is None, why
    Ain = CW.masked(A, uplo)
    why, _ = IW.accept_hpd_inverse(A, Ain, _matrix_call("elx_matrix_hpd_inverse", dtype, Ain, lda, uplo), uplo)
    assert why is None, why


@pytest.mark.parametrize("sweep", ["0", "8"])
def test_inverse_cpu_small_blocks_other_distribution(sweep, monkeypatch):
    """nb = 4 on n = 19 (five leaves, three levels) from a [VC,*] matrix: the drivers
    work on an [MC,MR] copy and write it back.  ELX_INVERSE_SWEEP=0: the recursive
    split down to single leaves; 8: the split above local sweeps of two leaves."""
    monkeypatch.setenv("ELX_INVERSE_SWEEP", sweep)
    n = 19
    g = el.Grid()
    nb0 = el.Blocksize()
    el.SetBlocksize(4)
    try:
        A = CW.hpd_matrix(n, 31, np.float64)
        for uplo in (el.LOWER, el.UPPER):
            Ain = CW.masked(A, uplo)
            D = el.DistMatrix(g, el.F64, el.VC, el.STAR, el.CPU, height=n, width=n)
            D.set_local(Ain)
            el.HPDInverse(uplo, D)
            why, _ = IW.accept_hpd_inverse(A, Ain, D.get_local(), uplo)
            assert why is None, why
    finally:
        el.SetBlocksize(nb0)


def test_hpd_inverse_cpu_not_hpd():
    """A negative diagonal entry raises NonHPDMatrixError from the Cholesky stage with
    its column; the library stays usable."""
    n = 40
    g = el.Grid()
    nb0 = el.Blocksize()
    el.SetBlocksize(16)
    try:
        A = CW.hpd_matrix(n, 7, np.float64)
        Abad = CW.masked(A, el.LOWER)
        Abad[25, 25] = -1.0
        D = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=n, width=n)
        D.set_local(Abad)
        with pytest.raises(el.NonHPDMatrixError, match="A was not numerically HPD") as ei:
            el.HPDInverse(el.LOWER, D)
        assert 1 <= ei.value.column <= 26
        Ain = CW.masked(A, el.LOWER)
        D.set_local(Ain)
        el.HPDInverse(el.LOWER, D)
        assert IW.accept_hpd_inverse(A, Ain, D.get_local(), el.LOWER)[0] is None
    finally:
        el.SetBlocksize(nb0)


def test_inverse_cpu_argument_checks():
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=6, width=5)
    H = el.DistMatrix(g, el.BF16, el.MC, el.MR, el.CPU, height=4, width=4)
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
    S = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=4, width=4)
    with pytest.raises(L.LogicError, match="bad UpperOrLower"):
        el.Trtrmm(7, S)
    with pytest.raises(L.LogicError, match="bad UnitOrNonUnit"):
        el.TriangularInverse(el.LOWER, 7, S)
    buf = np.zeros(16)
    p = buf.ctypes.data
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_triangular_inverse", el.F64, el.CPU, el.LOWER, el.NON_UNIT, 4, p, 3, None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_trtrmm", el.F64, el.CPU, el.LOWER, 4, p, 3, None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_hpd_inverse", el.F64, el.CPU, el.LOWER, 4, p, 3, None)
    with pytest.raises(L.LogicError, match="Trtrmm: only float and double are supported"):
        L.call("elx_matrix_trtrmm", el.BF16, el.CPU, el.LOWER, 4, p, 4, None)
    assert (buf == 0).all()


def test_cpp_inverse_api(tmp_path):
    """El::TriangularInverse, Trtrmm and HPDInverse on DistMatrix and Matrix,
    LocalTriangularInverse, LocalHPDInverse and a caught NonHPDMatrixException through
    include/El.hpp, Device::CPU, against a hand-computed 3 x 3 case."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_inverse_api"
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_inverse_api.cpp"), "-o", str(exe), "-L", libdir,
                           "-lelemental_amd", f"-Wl,-rpath,{libdir}"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "OK" in res.stdout
