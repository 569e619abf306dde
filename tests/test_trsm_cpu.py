"""Trsm without a GPU: the path plan (host code), the drop-in C++ surface, and the
exact family of _trsm_cases through elx_matrix_trsm and El::Trsm on Device::CPU,
which proves the inputs and the oracle that test_gpu_trsm uses."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _trsm_cases as TC
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trsm_plan(tmp_path):
    """kernels.hpp trsm_plan / trsm_batched_ok, the functions exec::Trsm,
    launch_trsm and TrsmLeft call: every boundary pinned (tests/cpp/test_trsm_plan.cpp)."""
    gxx = shutil.which("g++")
    if gxx is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("no g++ / HIP headers")
    exe = tmp_path / "test_trsm_plan"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I", os.path.join(ROOT, "elemental_amd", "csrc", "kernels"),
                           os.path.join(ROOT, "tests", "cpp", "test_trsm_plan.cpp"), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]


def test_trsm_plan_query_matches_table():
    """elx_trsm_plan names the path the table of _trsm_cases gives for every shape."""
    for (m, n), want in TC.PATHS.items():
        for dtype, name in ((el.F64, want[0]), (el.F32, want[1])):
            got, nbytes = TC.plan(dtype, m, n)
            assert got == name and nbytes == m * 65 * (8 if dtype == el.F64 else 4), (m, n, dtype, got, nbytes)


def test_cpp_trsm_api(tmp_path):
    """El::Trsm on Matrix through include/El.hpp, Device::CPU, against a
    hand-computed 3 x 3 case (LEFT, RIGHT, UNIT, checkIfSingular)."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_trsm_api"
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_trsm_api.cpp"), "-o", str(exe), "-L", libdir,
                           "-lelemental_amd", f"-Wl,-rpath,{libdir}"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "OK" in res.stdout


def test_trsm_matrix_exact_cpu():
    """elx_matrix_trsm on Device::CPU (the host substitution loop in f32 and f64)
    reproduces the exact family bit for bit, aligned and padded, A and the padding
    untouched."""
    TC.run_matrix(el.CPU, el.LEFT, TC.CPU_SHAPES)
    TC.run_matrix(el.CPU, el.RIGHT, TC.RIGHT_SHAPES)


def test_trsm_family_f32_models():
    """float32 numpy models of both GPU algorithms on the family: row-oriented
    substitution, and the inverse (substitution on the identity) applied as a
    product, each exact at the shapes that cross the 8-row batch, the wave, the
    64-row block and the LDS limit."""
    f = np.float32
    for (m, n) in [(129, 70), (256, 40), (300, 9)]:
        for unit in (False, True):
            T, B, Xl, _ = TC.family(m, n, unit)
            TC.bounds(m, n, unit, m)
            T32, R = T.astype(f), (TC.ALPHA * B).astype(f)

            def subst(rhs):
                X = rhs.copy()
                for i in range(m):
                    X[i] = (X[i] - T32[i, :i] @ X[:i]) / T32[i, i]
                return X
            assert np.array_equal(subst(R), Xl.astype(f)), (m, n, unit, "substitution")
            W = subst(np.eye(m, dtype=f))
            assert np.array_equal(W @ R, Xl.astype(f)), (m, n, unit, "inverse and product")


def test_trsm_family_large():
    """The conditions on the inputs of the largest GPU cases hold: float64 solves
    T X = alpha B exactly and every bound stays below 2^22 (m = 2100 with 256-row
    blocks, m = 700 with 300-row blocks)."""
    for unit in (False, True):
        assert max(TC.bounds(2100, 1030, unit, 256)) < TC.LIMIT
        assert max(TC.bounds(700, 1200, unit, 300)) < TC.LIMIT


def test_trsm_dist_exact_cpu():
    """El::Trsm on a 1x1 grid of Device::CPU matrices, all 16 side / uplo /
    orientation / diag cases at nb = 16, (45, 70), bit for bit in f32 and f64."""
    TC.run_dist(el.CPU, TC.all_sixteen(el.F64, 45, 70) + TC.all_sixteen(el.F32, 45, 70), 16)
