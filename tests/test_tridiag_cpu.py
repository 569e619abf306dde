"""El::HermitianTridiag without a GPU: the host column loop through
elx_matrix_hermitian_tridiag, the distributed driver on Device::CPU matrices over
gloo, ApplyQ, ExplicitCondensed, the exact and special inputs, the argument
checks and the drop-in C++ surface."""
import os
import random
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import _tridiag_workers as TW
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SIZES = [0, 1, 2, 3, 16, 17, 33, 129, 300]
# the GPU tests' sizes with the panel width 32 and 256 rows per workgroup
GPU_SIZES = [1, 2, 3, 31, 32, 33, 34, 65, 70, 127, 128, 129, 255, 256, 257, 258, 300, 515]
DIST_CASES = [(45, 16), (19, 8)]
NPDT = {el.F64: np.float64, el.F32: np.float32}
UPLOS = [el.LOWER, el.UPPER]


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


def _matrix_tridiag(npdt, A, uplo, pad=False):
    """elx_matrix_hermitian_tridiag on the column-major A on the host, lda = n or
    n + 3 with NaN around the matrix; tau has a guard word on either side."""
    n = A.shape[0]
    k = max(n - 1, 0)
    lda = max(1, n + 3 if pad else n)
    buf = np.full((max(n, 1), lda), np.nan, npdt)  # row q of buf = column q of the matrix
    buf[:n, :n] = A.T
    tau = np.full(k + 2, -7, npdt)
    L.call("elx_matrix_hermitian_tridiag", el.F64 if npdt == np.float64 else el.F32, el.CPU, uplo, n,
           buf.ctypes.data, lda, tau[1:].ctypes.data, None)
    assert np.isnan(buf[:n, n:]).all(), "written outside the matrix"
    assert tau[0] == -7 and tau[-1] == -7, "written outside tau"
    return np.asfortranarray(buf[:n, :n].T), tau[1:-1].copy()


def test_reference_meets_the_bounds():
    """The bounds are reachable: the numpy restatement of the unblocked loop and of
    the blocked latrd form (panels of 16, 32 and 64) in each type passes the
    acceptance at every size the tests use, in both uplo; so does LAPACK's sytrd
    where SciPy is installed.  The exact cases hold on the restatement too."""
    sizes = sorted(set(HOST_SIZES + GPU_SIZES + [n for n, _ in DIST_CASES]))
    for n in sizes:
        for npdt in (np.float64, np.float32):
            S = TW.random_symmetric(n, 100 + n, npdt)
            for lower in (True, False):
                for w in ((1, 16, 32, 64) if n <= 129 else (32, 64) if n <= 300 else (32,)):
                    why, _ = TW.accept(S, *TW.restated(S, lower, w), lower, quiet=True)
                    assert why is None, (n, npdt.__name__, lower, w, why)
    for npdt in (np.float64, np.float32):
        for lower in (True, False):
            for name, S in TW.exact_inputs(65, 3, npdt):
                for w in (1, 32):
                    TW.check_exact(S, *TW.restated(S, lower, w), lower)
            for up in (True, False):
                S = TW.scaled_symmetric(70, 21, npdt, up)
                why, _ = TW.accept(S, *TW.restated(S, lower, 32), lower, quiet=True)
                assert why is None, (npdt.__name__, lower, up, why)
    try:
        from scipy.linalg import lapack
    except ImportError:
        return
    for n in (17, 129, 300):
        S = TW.random_symmetric(n, 100 + n, np.float64)
        eps = np.finfo(np.float64).eps
        for lower in (True, False):
            c, d, e, tau, info = lapack.dsytrd(S, lower=int(lower))
            assert info == 0
            # the same storage and the same product; LAPACK's last scalar is 0 (H = I),
            # so only the three norms are compared with the acceptance's bounds
            Q = TW.rebuild_q(c, tau, lower)
            T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
            assert np.linalg.norm(S - Q @ T @ Q.T) <= 10 * n * eps * np.linalg.norm(S)
            assert np.linalg.norm(Q.T @ Q - np.eye(n)) <= 10 * n * eps
            assert np.abs(np.linalg.eigvalsh(T) - np.linalg.eigvalsh(S)).max() <= 10 * n * eps * np.linalg.norm(S, 2)


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
@pytest.mark.parametrize("uplo", UPLOS)
def test_matrix_tridiag_cpu(npdt, uplo):
    """The local driver on the host: every size, lda = n and n + 3, NaN in the unused
    triangle and around the matrix, guard words around tau untouched."""
    lower = uplo == el.LOWER
    bad = []
    for n in HOST_SIZES:
        A = TW.one_triangle(TW.random_symmetric(n, 100 + n, npdt), lower)
        for pad in (False, True):
            why, _ = TW.accept(A, *_matrix_tridiag(npdt, A, uplo, pad), lower)
            if why:
                bad.append((n, pad, why))
    assert not bad, bad


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
@pytest.mark.parametrize("uplo", UPLOS)
def test_matrix_tridiag_cpu_composed_panel(npdt, uplo, monkeypatch):
    """ELX_TRIDIAG_PANEL=level2 on the host: the blocked driver (panels of 32, the
    rank-2k update on the triangle) around the panel composed from exec::Gemv,
    SymvAccumulate, the QR leaf, RowScale and Ger, through the same acceptance and
    the exact cases."""
    monkeypatch.setenv("ELX_TRIDIAG_PANEL", "level2")
    lower = uplo == el.LOWER
    bad = []
    for n in (2, 3, 33, 34, 65, 129):
        A = TW.one_triangle(TW.random_symmetric(n, 100 + n, npdt), lower)
        why, _ = TW.accept(A, *_matrix_tridiag(npdt, A, uplo, n % 2 == 1), lower)
        if why:
            bad.append((n, why))
    assert not bad, bad
    for name, S in TW.exact_inputs(65, 3, npdt):
        TW.check_exact(S, *_matrix_tridiag(npdt, TW.one_triangle(S, lower, 0), uplo), lower)


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
@pytest.mark.parametrize("uplo", UPLOS)
def test_tridiag_cpu_exact_and_special(npdt, uplo):
    """Tridiagonal and diagonal inputs come back exactly; a column whose tail is
    exactly zero gives t = 2; inputs scaled by 2^+-500 (f64) / 2^+-50 (f32) pass the
    acceptance; a NaN propagates and the call returns."""
    lower = uplo == el.LOWER
    n = 65
    for name, S in TW.exact_inputs(n, 3, npdt):
        TW.check_exact(S, *_matrix_tridiag(npdt, TW.one_triangle(S, lower, 0), uplo), lower)
    for c in (0, 32, n - 3):
        S = TW.zero_tail_input(n, c, 5 + c, npdt, lower)
        A = TW.one_triangle(S, lower)
        P, t = _matrix_tridiag(npdt, A, uplo)
        assert t[c if lower else n - 2 - c] == 2, (c, t)
        why, _ = TW.accept(A, P, t, lower)
        assert why is None, (c, why)
    for up in (True, False):
        S = TW.scaled_symmetric(70, 21, npdt, up)
        A = TW.one_triangle(S, lower)
        why, _ = TW.accept(A, *_matrix_tridiag(npdt, A, uplo), lower)
        assert why is None, (up, why)
    S = TW.random_symmetric(40, 9, npdt)
    S[30, 20] = S[20, 30] = np.nan
    P, t = _matrix_tridiag(npdt, S, uplo)
    assert np.isnan(t).any() and np.isnan(np.diag(P)).any()


@pytest.mark.parametrize("world,height", [(2, 1), (2, 2), (4, 2), (8, 2)])
def test_tridiag_grids(world, height):
    """El::HermitianTridiag, ApplyQ and ExplicitCondensed over gloo on 1 x 2, 2 x 1,
    2 x 2 and 2 x 4 grids: n = 45 with nb = 16 and n = 19 with nb = 8, random
    alignments, t as [*,*] and as [MC,MR], every result through the acceptance and
    against the 1 x 1 result."""
    mp.spawn(TW.tridiag_worker, args=(world, _port(), height, el.CPU, el.F64, DIST_CASES, 31), nprocs=world, join=True)


def test_tridiag_grid_f32():
    mp.spawn(TW.tridiag_worker, args=(4, _port(), 2, el.CPU, el.F32, DIST_CASES, 37), nprocs=4, join=True)


@pytest.mark.parametrize("dtype", [el.F64, el.F32])
def test_tridiag_drivers_cpu(dtype):
    """el.HermitianTridiag, HermitianTridiagApplyQ in both orientations against the
    float64 Q, Q^T (Q B) = B and ExplicitCondensed on a 1 x 1 grid, nb = 8 so that
    ApplyQ runs several blocks and a ragged one."""
    g = el.Grid()
    el.SetBlocksize(8)
    try:
        for n in (1, 2, 3, 19, 45):
            S = TW.random_symmetric(n, 50 + n, NPDT[dtype])
            for uplo in UPLOS:
                TW.check_drivers(el, g, dtype, el.CPU, S, uplo)
    finally:
        el.SetBlocksize(128)


def test_tridiag_cpu_argument_checks():
    g = el.Grid()

    def dm(m, n, dtype=el.F64, seed=1):
        D = el.DistMatrix(g, dtype, el.MC, el.MR, el.CPU, height=m, width=n)
        if dtype in NPDT:
            D.set_local(np.asfortranarray(TW.random_symmetric(max(m, n), seed, NPDT[dtype])[:m, :n]))
        return D
    A = dm(6, 6)
    t = el.HermitianTridiag(el.LOWER, A)
    B = dm(6, 2)
    with pytest.raises(L.LogicError, match="ApplyQ: only LEFT is supported"):
        el.HermitianTridiagApplyQ(el.RIGHT, el.LOWER, el.NORMAL, A, t, B)
    with pytest.raises(L.LogicError, match="same height"):
        el.HermitianTridiagApplyQ(el.LEFT, el.LOWER, el.NORMAL, A, t, dm(5, 2))
    with pytest.raises(L.LogicError, match="must be square"):
        el.HermitianTridiag(el.LOWER, dm(6, 4))
    with pytest.raises(L.LogicError, match="HermitianTridiag: only float and double are supported"):
        el.HermitianTridiag(el.LOWER, dm(4, 4, el.BF16))
    buf, tau = np.zeros(16), np.zeros(4)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_hermitian_tridiag", el.F64, el.CPU, el.LOWER, 4, buf.ctypes.data, 3, tau.ctypes.data, None)
    with pytest.raises(L.LogicError, match="HermitianTridiag: only float and double are supported"):
        L.call("elx_matrix_hermitian_tridiag", el.BF16, el.CPU, el.LOWER, 4, buf.ctypes.data, 4, tau.ctypes.data, None)
    with pytest.raises(L.LogicError, match="bad UpperOrLower"):
        L.call("elx_matrix_hermitian_tridiag", el.F64, el.CPU, 77, 4, buf.ctypes.data, 4, tau.ctypes.data, None)
    with pytest.raises(L.LogicError, match="null"):
        L.call("elx_matrix_hermitian_tridiag", el.F64, el.CPU, el.LOWER, 4, None, 4, tau.ctypes.data, None)
    assert (buf == 0).all() and (tau == 0).all()
    assert int(L.lib().elx_tridiag_panel_cols()) == 32 and int(L.lib().elx_tridiag_rows()) == 256


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


def test_cpp_tridiag_api(tmp_path):
    """El::HermitianTridiag on Matrix and DistMatrix, herm_tridiag::ApplyQ and
    ExplicitCondensed through include/El.hpp, Device::CPU, against a hand-computed
    3 x 3 case in both uplo."""
    _build_and_run(tmp_path, "test_tridiag_api")


def test_cpp_tridiag_host_shapes(tmp_path):
    """The stand-alone program over the C ABI (its own main; it can be linked
    against a sanitized host build by hand): the CPU driver on the test sizes."""
    _build_and_run(tmp_path, "tridiag_host_check")
