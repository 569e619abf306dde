"""El::LU without a GPU: the distributed driver on Device::CPU matrices over gloo
(the host column loop of lu::Panel in the leaves), DistPermutation, SolveAfter,
LinearSolve, the argument checks and the drop-in C++ surface."""
import os
import random
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import _lu_workers as LW
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = [(19, 19), (23, 11), (11, 23)]


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
def test_lu(world, height):
    """El::LU on ragged shapes with nb = 4 (five panels, the last ragged): the
    shared acceptance, forced pivots across process rows, the singular cases on
    every rank, DistPermutation bit-exact against numpy."""
    mp.spawn(LW.lu_worker, args=(world, _port(), height, el.CPU, el.F64, RAGGED, 4, 31), nprocs=world, join=True)


def test_lu_f32():
    mp.spawn(LW.lu_worker, args=(4, _port(), 2, el.CPU, el.F32, [(19, 19)], 4, 37), nprocs=4, join=True)


@pytest.mark.parametrize("dtype", [el.F64, el.F32])
def test_lu_solves_2x2(dtype):
    """LUSolveAfter NORMAL / TRANSPOSE / ADJOINT and LinearSolve on a 2 x 2 grid,
    n = 37 with nb = 8, within the reference's bound."""
    mp.spawn(LW.solve_worker, args=(4, _port(), 2, el.CPU, dtype, 37, 5, 8, 41), nprocs=4, join=True)


def _matrix_lu(npdt, A, pad):
    """elx_matrix_lu on the column-major A, lda = m or m + 3 with NaN around."""
    m, n = A.shape
    lda = m + 3 if pad else m
    buf = np.full((n, lda), np.nan, npdt)  # row q of buf = column q of the matrix
    buf[:, :m] = A.T
    piv = np.full(min(m, n) + 2, -7, np.int32)
    L.call("elx_matrix_lu", el.F64 if npdt == np.float64 else el.F32, el.CPU, m, n, buf.ctypes.data, lda,
           piv[1:].ctypes.data, None)
    assert np.isnan(buf[:, m:]).all() and piv[0] == -7 and piv[-1] == -7
    return np.asfortranarray(buf[:, :m].T), piv[1:-1].astype(np.int64)


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
def test_matrix_lu_cpu(npdt):
    """The local driver on the host: the leaf alone (n <= 16), every split of the
    recursion (17, 33, 129), m < n, against the shared acceptance and the forced
    pivots (530 x 130, 37 x 60: pivots recovered exactly, L and U within the bound)."""
    bad = []
    for (m, n) in [(1, 1), (5, 3), (16, 16), (17, 17), (33, 31), (129, 129), (300, 37), (37, 300)]:
        A = LW.random_matrix(m, n, 100 + m + n, npdt)
        for pad in (False, True):
            LU, piv = _matrix_lu(npdt, A, pad)
            why, _ = LW.accept(A, LU, piv)
            if why:
                bad.append((m, n, pad, why))
    for (m, n) in [(40, 40), (300, 37), (530, 130), (37, 60)]:
        perm = LW.forced_perm(m, min(m, n), LW.far_rows(m, min(m, n)))
        A, L0, U0 = LW.forced_input(m, n, perm, m + n, npdt)
        LU, piv = _matrix_lu(npdt, A, False)
        why = LW.check_forced(A, LU, piv, perm, L0, U0)
        if why:
            bad.append((m, n, "forced", why))
    assert not bad, bad


@pytest.mark.parametrize("npdt", [np.float64, np.float32])
def test_lu_cpu_nan_rule(npdt):
    """The documented pivot rule on the host leaf: a NaN never beats a number, and a
    column with nothing but zeros and NaNs left reports that column's zero pivot."""
    for (m, n) in ((256, 4), (515, 16), (515, 40)):
        A, Z = LW.nan_inputs(m, n, 77 + m + n, npdt, 256)
        why = LW.check_nan_rule(A, *_matrix_lu(npdt, A, False))
        assert why is None, (m, n, why)
        with pytest.raises(el.SingularMatrixError, match=r"column 2$"):
            _matrix_lu(npdt, Z, False)


def test_lu_cpu_singular_column():
    """An exactly zero column c raises SingularMatrixError naming column c + 1 (the
    first column, one inside a later leaf, the last); two equal rows of a
    forced-pivot input make the last pivot exactly zero; the library stays usable."""
    n = 40
    g = el.Grid()
    A = LW.random_matrix(n, n, 9, np.float64)
    for c in (0, 16, n - 1):
        Az = A.copy()
        Az[:, c] = 0
        D = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=n, width=n)
        D.set_local(Az)
        with pytest.raises(el.SingularMatrixError, match=rf"column {c + 1}$"):
            el.LU(D)
    perm = LW.forced_perm(n, n, LW.far_rows(n, n))
    Af, _, _ = LW.forced_input(n, n, perm, 3, np.float64)
    Af[perm[n - 1]] = Af[perm[5]]
    D = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=n, width=n)
    D.set_local(Af)
    with pytest.raises(el.SingularMatrixError, match=rf"column {n}$"):
        el.LU(D)
    D.set_local(A)
    P = el.LU(D)
    assert LW.accept(A, D.get_local(), P.swap_dests())[0] is None


def test_permutation_cpu_bits():
    """PermuteRows then InversePermuteRows is bit-identical to the input (-0.0 and
    NaN payloads included) and PermuteRows equals numpy indexing by explicit_vector()."""
    g = el.Grid()
    m = 29
    D = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=m, width=m)
    D.set_local(LW.random_matrix(m, m, 4, np.float64))
    P = el.LU(D)
    assert P.Height() == m and len(P.swap_dests()) == m
    for npdt, dtype in ((np.float64, el.F64), (np.float32, el.F32)):
        B0 = LW.payload_matrix(m, 6, 5, npdt)
        B = el.DistMatrix(g, dtype, el.MC, el.MR, el.CPU, height=m, width=6)
        B.set_local(B0)
        P.PermuteRows(B)
        assert np.array_equal(_bits(B.get_local()), _bits(B0[P.explicit_vector()]))
        P.InversePermuteRows(B)
        assert np.array_equal(_bits(B.get_local()), _bits(B0))
    I = el.Permutation().MakeIdentity(m)
    B.set_local(B0)
    I.PermuteRows(B)
    assert np.array_equal(_bits(B.get_local()), _bits(B0)) and len(I.swap_dests()) == 0


def test_lu_cpu_argument_checks():
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=6, width=5)
    A.set_local(LW.random_matrix(6, 5, 1, np.float64))
    P = el.LU(A)
    B = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=6, width=2)
    with pytest.raises(L.LogicError, match="A must be square"):
        el.LUSolveAfter(el.NORMAL, A, P, B)
    with pytest.raises(L.LogicError, match="A must be square"):
        el.LinearSolve(A, B)
    S = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=5, width=5)
    S.set_local(LW.random_matrix(5, 5, 2, np.float64))
    P5 = el.LU(S)
    with pytest.raises(L.LogicError, match="A and B must be the same height"):
        el.LUSolveAfter(el.NORMAL, S, P5, B)
    with pytest.raises(L.LogicError, match="P and B must be the same height"):
        P5.PermuteRows(B)
    H = el.DistMatrix(g, el.BF16, el.MC, el.MR, el.CPU, height=4, width=4)
    with pytest.raises(L.LogicError, match="LU: only float and double are supported"):
        el.LU(H)
    buf = np.zeros(16)
    piv = np.zeros(4, np.int32)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_lu", el.F64, el.CPU, 4, 4, buf.ctypes.data, 3, piv.ctypes.data, None)
    with pytest.raises(L.LogicError, match="LU: only float and double are supported"):
        L.call("elx_matrix_lu", el.BF16, el.CPU, 4, 4, buf.ctypes.data, 4, piv.ctypes.data, None)
    assert (buf == 0).all()
    assert int(L.lib().elx_lu_leaf_cols()) == 16 and int(L.lib().elx_lu_leaf_rows()) > 0


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


def test_cpp_lu_api(tmp_path):
    """El::LU on Matrix and DistMatrix, lu::SolveAfter, LinearSolve, P.PermuteRows and
    a caught SingularMatrixException through include/El.hpp, Device::CPU, against a
    hand-computed 3 x 3 case."""
    _build_and_run(tmp_path, "test_lu_api")


def test_cpp_lu_host_shapes(tmp_path):
    """The stand-alone program over the C ABI that the sanitizer check builds (here
    without the sanitizer): the CPU LocalLU and Permutation code on the test shapes."""
    _build_and_run(tmp_path, "lu_host_check")
