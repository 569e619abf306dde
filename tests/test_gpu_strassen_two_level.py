"""Two Strassen-Winograd levels, the default of the large f64 / f32 products,
forced at small sizes on the gfx950 kernels: the recursion rule (the inner
threshold is ELX_GEMM_STRASSEN_MIN2's alone), exactness on integer operands,
the rounding of two levels against the bound the suite holds one El::Gemm to,
and determinism."""
import numpy as np
import pytest

import _strassen_cases as sc
import oracle
from elemental_amd import _lib as L

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPS = {"N": L.NORMAL, "T": L.TRANSPOSE}
NPDT = {"f64": np.float64, "f32": np.float32}
KNOBS = ("ELX_GEMM_STRASSEN", "ELX_GEMM_STRASSEN_MIN", "ELX_GEMM_STRASSEN_MIN2")


def dev(a: np.ndarray) -> "torch.Tensor":
    return torch.from_numpy(np.ravel(np.asfortranarray(a), order="F").copy()).cuda()


def host(t, shape):
    return np.asfortranarray(t.cpu().numpy().reshape(shape, order="F"))


def gemm(dt, ta, tb, m, n, k, alpha, beta, A, B, C):
    dA, dB, dC = dev(A), dev(B), dev(C)
    torch.cuda.synchronize()
    L.call("elx_gemm_" + dt, OPS[ta], OPS[tb], m, n, k, alpha, dA.data_ptr(), A.shape[0], dB.data_ptr(), B.shape[0],
           beta, dC.data_ptr(), C.shape[0], None)
    levels = L.lib().elx_gemm_last_levels()
    L.call("elx_device_synchronize")
    return host(dC, C.shape), levels


def run_exact(dt, ta, tb, m, n, k, alpha, beta, pad=0):
    npdt = NPDT[dt]
    A0, B0, C0, P = sc.case(m, n, k, ta, tb, pad)
    got, levels = gemm(dt, ta, tb, m, n, k, alpha, beta, A0.astype(npdt), B0.astype(npdt), sc.start_c(C0, m, beta, npdt))
    return got, sc.expected(C0, P, m, alpha, beta).astype(npdt), levels


@pytest.fixture
def knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("ELX_GEMM_STRASSEN_MIN", sc.FORCE_MIN)
    return monkeypatch


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_default_rule_exact(knobs, dt):
    """512^3, outer threshold 128: one level under the inner default, two with
    MIN2 = 128, one again with ELX_GEMM_STRASSEN=1; exact each time."""
    for alpha, beta in sc.PAIRS:
        got, want, levels = run_exact(dt, "N", "N", 512, 512, 512, alpha, beta)
        assert levels == 1 and np.array_equal(got, want), f"default alpha={alpha} beta={beta}"
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", sc.FORCE_MIN)
    for alpha, beta in sc.PAIRS:
        got, want, levels = run_exact(dt, "T", "N", 512, 512, 512, alpha, beta)
        assert levels == 2 and np.array_equal(got, want), f"MIN2 alpha={alpha} beta={beta}"
    knobs.setenv("ELX_GEMM_STRASSEN", "1")
    got, want, levels = run_exact(dt, "N", "T", 512, 512, 512, 0.5, -0.5)
    assert levels == 1 and np.array_equal(got, want)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ta,tb", [("N", "N"), ("T", "T")])
def test_two_levels_ragged_padded_exact(knobs, dt, ta, tb):
    """768 x 1280 x 512 with ld padded by 3: quarters of 192 x 320 x 128, no
    multiple of the tile, unaligned quadrant views, through both levels."""
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", sc.FORCE_MIN)
    for alpha, beta in sc.PAIRS:
        got, want, levels = run_exact(dt, ta, tb, 768, 1280, 512, alpha, beta, pad=3)
        assert levels == 2
        assert np.array_equal(got, want), f"{dt} {ta}{tb} alpha={alpha} beta={beta}"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_rounding_two_levels(knobs, dt):
    """Uniform(-0.1, 0.1) at 1024^3, alpha = 0.5, beta = -0.5, two levels: the
    parity ratio against the float64 product stays within 10, the bound of one
    El::Gemm.  The one-level and plain ratios are printed beside it."""
    n = 1024
    npdt = NPDT[dt]
    A, B, C = (oracle.hash_matrix(n, n, seed, -0.1, 0.1, npdt) for seed in (31, 32, 33))
    A64, B64, C64 = (x.astype(np.float64) for x in (A, B, C))
    ref = 0.5 * (A64 @ B64) - 0.5 * C64
    eps = np.finfo(npdt).eps
    ratio = {}
    for want, setting in ((2, "2"), (1, "1"), (0, "0")):
        knobs.setenv("ELX_GEMM_STRASSEN", setting)
        got, levels = gemm(dt, "N", "N", n, n, n, 0.5, -0.5, A, B, C)
        assert levels == want
        ratio[want] = oracle.parity_ratio(got, ref, A, B, n, eps)
    print(f"parity ratio {dt} NN 1024^3: two levels {ratio[2]:.3g}, one level {ratio[1]:.3g}, plain {ratio[0]:.3g}")
    assert ratio[2] <= 10, f"{dt}: two levels {ratio[2]}, one {ratio[1]}, plain {ratio[0]}"


def test_two_levels_deterministic(knobs):
    knobs.setenv("ELX_GEMM_STRASSEN_MIN2", sc.FORCE_MIN)
    A = oracle.hash_matrix(512, 512, 21, -0.1, 0.1)
    B = oracle.hash_matrix(512, 512, 22, -0.1, 0.1)
    C = oracle.hash_matrix(512, 512, 23, -0.1, 0.1)
    one, l1 = gemm("f64", "N", "N", 512, 512, 512, 0.5, -0.5, A, B, C)
    two, l2 = gemm("f64", "N", "N", 512, 512, 512, 0.5, -0.5, A, B, C)
    assert l1 == 2 and l2 == 2
    assert np.array_equal(one, two)
