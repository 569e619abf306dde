"""The Strassen-Winograd schedule on Device::CPU (cpu_gemm plus plain loops for the
sums), forced with ELX_GEMM_STRASSEN_MIN: the same code that drives the gfx950
kernels, checked bit for bit without a GPU."""
import numpy as np
import pytest

import _strassen_cases as sc
from elemental_amd import _lib as L

OPS = {"N": L.NORMAL, "T": L.TRANSPOSE}
DT = {"f64": (L.F64, np.float64), "f32": (L.F32, np.float32)}


def run(dt, ta, tb, m, n, k, alpha, beta, pad=0):
    code, npdt = DT[dt]
    A0, B0, C0, P = sc.case(m, n, k, ta, tb, pad)
    A, B = np.asfortranarray(A0.astype(npdt)), np.asfortranarray(B0.astype(npdt))
    C = sc.start_c(C0, m, beta, npdt)
    L.call("elx_matrix_gemm", code, L.CPU, OPS[ta], OPS[tb], m, n, k, alpha, A.ctypes.data, A.shape[0],
           B.ctypes.data, B.shape[0], beta, C.ctypes.data, C.shape[0], None)
    levels = L.lib().elx_gemm_last_levels()
    return C, sc.expected(C0, P, m, alpha, beta).astype(npdt), levels


@pytest.fixture
def forced(monkeypatch):
    monkeypatch.setenv("ELX_GEMM_STRASSEN_MIN", sc.FORCE_MIN)
    monkeypatch.delenv("ELX_GEMM_STRASSEN", raising=False)
    return monkeypatch


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ta", ["N", "T"])
@pytest.mark.parametrize("tb", ["N", "T"])
def test_orientations_exact(forced, dt, ta, tb):
    for alpha, beta in sc.PAIRS:
        got, want, levels = run(dt, ta, tb, 256, 256, 256, alpha, beta)
        assert levels == 1
        assert np.array_equal(got, want), f"{dt} {ta}{tb} alpha={alpha} beta={beta}"


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ta,tb", [("N", "N"), ("T", "N"), ("N", "T"), ("T", "T")])
def test_ragged_halves_padded_ld_exact(forced, dt, ta, tb):
    """384 x 640 x 512: three different halves, leading dimensions 3 rows larger
    than the row counts; the padding rows of C stay as they were."""
    for alpha, beta in sc.PAIRS:
        got, want, levels = run(dt, ta, tb, 384, 640, 512, alpha, beta, pad=3)
        assert levels == 1
        assert np.array_equal(got, want), f"{dt} {ta}{tb} alpha={alpha} beta={beta}"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_levels_exact(forced, dt):
    forced.setenv("ELX_GEMM_STRASSEN", "2")
    got, want, levels = run(dt, "N", "T", 512, 512, 512, 0.5, -0.5)
    assert levels == 2
    assert np.array_equal(got, want)
    got, want, levels = run(dt, "T", "N", 512, 512, 512, 1.0, 0.0)
    assert levels == 2
    assert np.array_equal(got, want)


def test_not_taken(forced):
    """An odd dimension, a dimension below the threshold, the off switch, and the
    CPU device without a forced threshold all run the plain loop."""
    got, want, levels = run("f64", "N", "N", 257, 256, 256, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
    got, want, levels = run("f64", "N", "N", 256, 256, 126, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
    forced.setenv("ELX_GEMM_STRASSEN", "0")
    got, want, levels = run("f64", "N", "N", 256, 256, 256, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
    forced.delenv("ELX_GEMM_STRASSEN")
    forced.delenv("ELX_GEMM_STRASSEN_MIN")
    got, want, levels = run("f64", "N", "N", 256, 256, 256, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
