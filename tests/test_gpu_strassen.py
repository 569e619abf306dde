"""One Strassen-Winograd level over the gfx950 ring kernels (core/strassen.cpp,
quad_sum / quad_scatter in kernels/blas1.hip), forced at small sizes with
ELX_GEMM_STRASSEN_MIN: exact on integer operands, the path asserted through
elx_gemm_last_levels, and the rounding of one level measured against the bound
the suite holds one El::Gemm to."""
import numpy as np
import pytest

import _strassen_cases as sc
import oracle
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

OPS = {"N": L.NORMAL, "T": L.TRANSPOSE}
NPDT = {"f64": np.float64, "f32": np.float32}


def dev(a: np.ndarray) -> "torch.Tensor":
    return torch.from_numpy(np.ravel(np.asfortranarray(a), order="F").copy()).cuda()


def host(t, shape):
    return np.asfortranarray(t.cpu().numpy().reshape(shape, order="F"))


def gemm(dt, ta, tb, m, n, k, alpha, beta, A, B, C):
    """elx_gemm_<dt> on host arrays (leading dimension = rows held); returns (C, levels)."""
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
def forced(monkeypatch):
    monkeypatch.setenv("ELX_GEMM_STRASSEN_MIN", sc.FORCE_MIN)
    monkeypatch.delenv("ELX_GEMM_STRASSEN", raising=False)
    return monkeypatch


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ta", ["N", "T"])
@pytest.mark.parametrize("tb", ["N", "T"])
def test_orientations_exact(forced, dt, ta, tb):
    """256^3: the halves are exactly one 128-tile."""
    for alpha, beta in sc.PAIRS:
        got, want, levels = run_exact(dt, ta, tb, 256, 256, 256, alpha, beta)
        assert levels == 1
        assert np.array_equal(got, want), f"{dt} {ta}{tb} alpha={alpha} beta={beta}"


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ta,tb", [("N", "N"), ("T", "N"), ("N", "T"), ("T", "T")])
def test_ragged_halves_padded_ld_exact(forced, dt, ta, tb):
    """384 x 640 x 512 (halves 192 x 320 x 256, no multiples of the tile) with
    lda, ldb, ldc 3 rows larger than the row counts: the quadrant views are not
    16-B aligned, and C's padding rows must stay as they were."""
    for alpha, beta in sc.PAIRS:
        got, want, levels = run_exact(dt, ta, tb, 384, 640, 512, alpha, beta, pad=3)
        assert levels == 1
        assert np.array_equal(got, want), f"{dt} {ta}{tb} alpha={alpha} beta={beta}"


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ta", ["N", "T"])
def test_tall_whole_chunks_exact(forced, dt, ta):
    """16384 x 256 x 256: halves of 8192 rows, so quad_sum (S, with ta = N) and
    quad_scatter sweep whole unrolled 16-B chunks (2048 f64 / 4096 f32 rows) as
    they do at full size; with ta = T the long dimension is S's columns."""
    for alpha, beta in sc.PAIRS:
        got, want, levels = run_exact(dt, ta, "N", 16384, 256, 256, alpha, beta)
        assert levels == 1
        assert np.array_equal(got, want), f"{dt} {ta}N alpha={alpha} beta={beta}"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_two_levels_exact(forced, dt):
    forced.setenv("ELX_GEMM_STRASSEN", "2")
    for ta, tb, alpha, beta in [("N", "N", 1.0, 0.0), ("T", "T", 0.5, -0.5)]:
        got, want, levels = run_exact(dt, ta, tb, 512, 512, 512, alpha, beta)
        assert levels == 2
        assert np.array_equal(got, want), f"{dt} {ta}{tb}"


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_not_taken(forced, dt):
    """An odd dimension and the off switch run the plain kernel (0 levels), exactly;
    so does the default threshold."""
    got, want, levels = run_exact(dt, "N", "N", 257, 256, 256, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
    forced.setenv("ELX_GEMM_STRASSEN", "0")
    got, want, levels = run_exact(dt, "N", "N", 256, 256, 256, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)
    forced.delenv("ELX_GEMM_STRASSEN")
    forced.delenv("ELX_GEMM_STRASSEN_MIN")
    got, want, levels = run_exact(dt, "N", "N", 256, 256, 256, 0.5, -0.5)
    assert levels == 0 and np.array_equal(got, want)


def test_deterministic(forced):
    A = oracle.hash_matrix(512, 512, 21, -0.1, 0.1)
    B = oracle.hash_matrix(512, 512, 22, -0.1, 0.1)
    C = oracle.hash_matrix(512, 512, 23, -0.1, 0.1)
    one, l1 = gemm("f64", "N", "N", 512, 512, 512, 0.5, -0.5, A, B, C)
    two, l2 = gemm("f64", "N", "N", 512, 512, 512, 0.5, -0.5, A, B, C)
    assert l1 == 1 and l2 == 1
    assert np.array_equal(one, two)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("ta", ["N", "T"])
def test_rounding_one_level(forced, dt, ta):
    """Uniform(-0.1, 0.1) at 1024^3, alpha = 0.5, beta = -0.5: the parity ratio
    against the float64 product stays within 10, the bound of one El::Gemm; the
    plain path's ratio on the same inputs is printed beside it."""
    n = 1024
    npdt = NPDT[dt]
    A, B, C = (oracle.hash_matrix(n, n, seed, -0.1, 0.1, npdt) for seed in (31, 32, 33))
    A64, B64, C64 = (x.astype(np.float64) for x in (A, B, C))
    ref = 0.5 * ((A64 if ta == "N" else A64.T) @ B64) - 0.5 * C64
    got, levels = gemm(dt, ta, "N", n, n, n, 0.5, -0.5, A, B, C)
    assert levels == 1
    forced.setenv("ELX_GEMM_STRASSEN", "0")
    plain, levels0 = gemm(dt, ta, "N", n, n, n, 0.5, -0.5, A, B, C)
    assert levels0 == 0
    eps = np.finfo(npdt).eps
    r1 = oracle.parity_ratio(got, ref, A, B, n, eps)
    r0 = oracle.parity_ratio(plain, ref, A, B, n, eps)
    print(f"parity ratio {dt} {ta}N 1024^3: one level {r1:.3g}, plain {r0:.3g}")
    assert r1 <= 10, f"{dt} {ta}N: one level {r1}, plain {r0}"


def test_distributed_single_update_reaches_it(forced):
    """El::Gemm on a 1 x 1 grid: SummaC's single-update shortcut runs one local
    GEMM, which takes the path."""
    n = 512
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, el.MC, el.MR, el.GPU, height=n, width=n).fill_hash(1, -0.1, 0.1)
    B = el.DistMatrix(g, el.F64, el.MC, el.MR, el.GPU, height=n, width=n).fill_hash(2, -0.1, 0.1)
    C = el.DistMatrix(g, el.F64, el.MC, el.MR, el.GPU, height=n, width=n).fill_hash(3, -0.1, 0.1)
    el.Gemm(el.NORMAL, el.NORMAL, 0.5, A, B, -0.5, C)
    assert L.lib().elx_gemm_last_levels() == 1
    got = C.get_local()
    Ag, Bg, Cg = (oracle.hash_matrix(n, n, seed, -0.1, 0.1) for seed in (1, 2, 3))
    ref = oracle.gemm("N", "N", 0.5, Ag, Bg, -0.5, Cg)
    r = oracle.parity_ratio(got, ref, Ag, Bg, n, np.finfo(np.float64).eps)
    assert r <= 10, f"parity ratio {r}"
