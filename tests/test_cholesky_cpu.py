"""El::Cholesky without a GPU: the distributed driver on Device::CPU matrices over
gloo (the host loop of LowerVariant3Unblocked in the leaves), SolveAfter, the
argument checks, and the drop-in C++ surface."""
import os
import random
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import _cholesky_workers as CW
import oracle
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1), (4, 2), (8, 2)])
def test_cholesky(world, height):
    """El::Cholesky LOWER / UPPER, ragged blocks (n = 19, nb = 4: five leaves, three
    levels of the recursive split, Trsm and Syrk on views of views), the other
    triangle NaN, against numpy; the not-HPD case raises on all ranks."""
    mp.spawn(CW.cholesky_worker, args=(world, _port(), height, el.CPU, el.F64, 19, 4, 31), nprocs=world, join=True)


@pytest.mark.parametrize("dtype", [el.F64, el.F32])
@pytest.mark.parametrize("uplo", [el.LOWER, el.UPPER])
def test_cholesky_cpu_residual_and_solve(dtype, uplo):
    """1x1 grid on the CPU device, n = 70 with nb = 16: the shared acceptance
    (residual <= 10 n eps ||A||_F, other triangle untouched) and SolveAfter within
    the reference's own bound (tests/lapack_like/Cholesky.cpp:39-43: ||X - A^-1 B||_oo
    <= 100 eps n ||B||_1)."""
    npdt = np.float64 if dtype == el.F64 else np.float32
    n, nrhs = 70, 9
    g = el.Grid()
    nb0 = el.Blocksize()
    el.SetBlocksize(16)
    try:
        A = CW.hpd_matrix(n, 5, npdt)
        Ain = CW.masked(A, uplo)
        D = el.DistMatrix(g, dtype, el.MC, el.MR, el.CPU, height=n, width=n)
        D.set_local(Ain)
        el.Cholesky(uplo, D)
        why, _ = CW.accept(A, Ain, D.get_local(), uplo)
        assert why is None, why
        B0 = oracle.hash_matrix(n, nrhs, 6, 0.0, 1.0, npdt)
        B = el.DistMatrix(g, dtype, el.MC, el.MR, el.CPU, height=n, width=nrhs)
        B.set_local(B0)
        el.CholeskySolveAfter(uplo, el.NORMAL, D, B)
        X = np.linalg.solve(A.astype(np.float64), B0.astype(np.float64))
        err = np.abs(B.get_local().astype(np.float64) - X).sum(axis=1).max()
        assert err <= 100 * np.finfo(npdt).eps * n * np.abs(B0.astype(np.float64)).sum(axis=0).max()
    finally:
        el.SetBlocksize(nb0)


def test_cholesky_cpu_not_hpd_column():
    """The first column of the CPU leaf loop reports exactly its own column; a NaN
    pivot fails like a non-positive one; the library stays usable."""
    n = 12
    g = el.Grid()
    A = CW.hpd_matrix(n, 7, np.float64)
    for j, val in ((0, -1.0), (5, 0.0), (11, np.nan)):
        Abad = CW.masked(A, el.LOWER)
        Abad[j, j] = val
        D = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=n, width=n)
        D.set_local(Abad)
        with pytest.raises(el.NonHPDMatrixError, match="A was not numerically HPD") as ei:
            el.Cholesky(el.LOWER, D)
        assert ei.value.column == j + 1
    D.set_local(CW.masked(A, el.LOWER))
    el.Cholesky(el.LOWER, D)
    assert CW.accept(A, CW.masked(A, el.LOWER), D.get_local(), el.LOWER)[0] is None


def test_cholesky_cpu_argument_checks():
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=6, width=5)
    with pytest.raises(L.LogicError, match="A must be square"):
        el.Cholesky(el.LOWER, A)
    H = el.DistMatrix(g, el.BF16, el.MC, el.MR, el.CPU, height=4, width=4)
    with pytest.raises(L.LogicError, match="Cholesky: only float and double are supported"):
        el.Cholesky(el.LOWER, H)
    A = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=5, width=5)
    B = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=4, width=3)
    with pytest.raises(L.LogicError, match="A and B must be the same height"):
        el.CholeskySolveAfter(el.LOWER, el.NORMAL, A, B)
    buf = np.zeros(16)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_cholesky", el.F64, el.CPU, el.LOWER, 4, buf.ctypes.data, 3, None)
    assert (buf == 0).all()


def test_matrix_cholesky_cpu_blocked():
    """elx_matrix_cholesky attaches the buffer to a 1x1 DistMatrix: n = 300 runs the
    blocked driver (three 128-row leaves), lda = n + 3."""
    n, lda = 300, 303
    A = CW.hpd_matrix(n, 8, np.float64)
    for uplo in (el.LOWER, el.UPPER):
        Ain = CW.masked(A, uplo)
        buf = np.full((n, lda), np.nan)  # row q of buf = column q of the matrix
        buf[:, :n] = Ain.T
        L.call("elx_matrix_cholesky", el.F64, el.CPU, uplo, n, buf.ctypes.data, lda, None)
        assert np.isnan(buf[:, n:]).all()
        why, _ = CW.accept(A, Ain, buf[:, :n].T, uplo)
        assert why is None, why


def test_cpp_cholesky_api(tmp_path):
    """El::Cholesky on DistMatrix and Matrix, cholesky::SolveAfter, HPDSolve and a
    caught NonHPDMatrixException through include/El.hpp, Device::CPU, against a
    hand-computed 3 x 3 case."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_cholesky_api"
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_cholesky_api.cpp"), "-o", str(exe), "-L", libdir,
                           "-lelemental_amd", f"-Wl,-rpath,{libdir}"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "OK" in res.stdout
