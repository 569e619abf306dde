"""The recursion rule of the Strassen-Winograd path on Device::CPU: with
ELX_GEMM_STRASSEN unset up to two levels run, the second only where a
sub-product's own min(m, n, k) reaches the inner threshold, which only
ELX_GEMM_STRASSEN_MIN2 moves.  Integer cases of _strassen_cases, so every form
equals the exact product."""
import numpy as np
import pytest

import _strassen_cases as sc
from elemental_amd import _lib as L

OPS = {"N": L.NORMAL, "T": L.TRANSPOSE}
DT = {"f64": (L.F64, np.float64), "f32": (L.F32, np.float32)}
KNOBS = ("ELX_GEMM_STRASSEN", "ELX_GEMM_STRASSEN_MIN", "ELX_GEMM_STRASSEN_MIN2")


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
def knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_default_rule(knobs, dt):
    """512^3 with the outer threshold forced to 128: the 256^3 sub-products stay
    below the inner default (8192), one level; MIN2 = 128 splits them as well."""
    knobs.setenv("ELX_GEMM_STRASSEN_MIN", sc.FORCE_MIN)
    for alpha, beta in sc.PAIRS:
        got, want, levels = run(dt, "N", "N", 512, 512, 512, alpha, beta)
        assert levels == 1
        assert np.array_equal(got, want), f"one level alpha={alpha} beta={beta}"
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", sc.FORCE_MIN)
    for alpha, beta in sc.PAIRS:
        got, want, levels = run(dt, "N", "N", 512, 512, 512, alpha, beta)
        assert levels == 2
        assert np.array_equal(got, want), f"two levels alpha={alpha} beta={beta}"


@pytest.mark.parametrize("ta,tb", [("N", "N"), ("T", "N"), ("N", "T"), ("T", "T")])
def test_two_levels_by_min2_ragged_padded(knobs, ta, tb):
    """768 x 1280 x 512 with ld padded by 3: halves 384 x 640 x 256 and quarters
    192 x 320 x 128, all different, through both levels in every orientation."""
    knobs.setenv("ELX_GEMM_STRASSEN_MIN", sc.FORCE_MIN)
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", sc.FORCE_MIN)
    got, want, levels = run("f64", ta, tb, 768, 1280, 512, 0.5, -0.5, pad=3)
    assert levels == 2
    assert np.array_equal(got, want)


def test_inner_threshold_is_its_own(knobs):
    """MIN2 above the sub-product keeps one level; ELX_GEMM_STRASSEN=1 keeps one
    level whatever MIN2 says; =2 takes MIN for both levels unless MIN2 is given."""
    knobs.setenv("ELX_GEMM_STRASSEN_MIN", sc.FORCE_MIN)
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", "258")
    got, want, levels = run("f64", "N", "T", 512, 512, 512, 0.5, -0.5)
    assert levels == 1 and np.array_equal(got, want)
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", "256")
    got, want, levels = run("f64", "N", "T", 512, 512, 512, 0.5, -0.5)
    assert levels == 2 and np.array_equal(got, want)
    knobs.setenv("ELX_GEMM_STRASSEN", "1")
    got, want, levels = run("f64", "N", "T", 512, 512, 512, 0.5, -0.5)
    assert levels == 1 and np.array_equal(got, want)
    knobs.setenv("ELX_GEMM_STRASSEN", "2")
    knobs.delenv("ELX_GEMM_STRASSEN_MIN2")
    got, want, levels = run("f64", "N", "T", 512, 512, 512, 0.5, -0.5)
    assert levels == 2 and np.array_equal(got, want)
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", "258")
    got, want, levels = run("f64", "N", "T", 512, 512, 512, 0.5, -0.5)
    assert levels == 1 and np.array_equal(got, want)


def test_cpu_without_a_forced_threshold(knobs):
    """No knob, and MIN2 alone: the host path stays on the plain loop."""
    got, want, levels = run("f64", "N", "N", 512, 512, 512, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", sc.FORCE_MIN)
    got, want, levels = run("f64", "N", "N", 512, 512, 512, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
