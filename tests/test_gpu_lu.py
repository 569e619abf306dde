"""El::LU on the GPU: the multi-workgroup panel kernels (getrf.hip) through
elx_matrix_lu, the column recursion above them, the singular paths, Permutation,
the solves and the two-rank RCCL driver.

Inputs: hash_matrix in [-1, 1] rounded to the type, and forced-pivot matrices
A[perm] = L0 U0 whose every entry is exact (_lu_workers.forced_input).  Acceptance
(_lu_workers.accept): a valid swap sequence, finite, max |L| <= 1 exactly,
||P A - L U||_F <= 10 max(m, n) eps ||A||_F."""
import random
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import _lu_workers as LW
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPDT = {el.F64: np.float64, el.F32: np.float32}
BOTH_TYPES = [el.F64, el.F32]


def _port():
    """A free rendezvous port below the kernel's ephemeral range (see test_gpu_dist)."""
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


def _w():
    return int(L.lib().elx_lu_leaf_cols())


def _r():
    return int(L.lib().elx_lu_leaf_rows())


def _matrix_lu(dtype, A, pad):
    """elx_matrix_lu on the column-major A with lda = m (aligned) or m + 3 and the
    base one element into the allocation (pad); everything around the matrix is
    NaN, the pivot array has a guard word on either side.  Returns (LU, piv) after
    checking that nothing outside the matrix and the pivots changed."""
    m, n = A.shape
    k = min(m, n)
    lda, off = (m + 3, 1) if pad else (m, 0)
    buf = np.full(off + lda * n, np.nan, A.dtype)
    buf[off:].reshape(n, lda)[:, :m] = A.T
    t = torch.from_numpy(buf).cuda()
    piv = torch.full((k + 2,), -7, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    L.call("elx_matrix_lu", dtype, el.GPU, m, n, t.data_ptr() + off * A.dtype.itemsize, lda, piv.data_ptr() + 4, None)
    L.call("elx_device_synchronize")
    out = t.cpu().numpy()
    inside = np.zeros(buf.shape, bool)
    inside[off:].reshape(n, lda)[:, :m] = True
    assert np.array_equal(_bits(out[~inside]), _bits(buf[~inside])), "written outside the matrix"
    p = piv.cpu().numpy()
    assert p[0] == -7 and p[-1] == -7, "written outside the pivots"
    return np.asfortranarray(out[off:].reshape(n, lda)[:, :m].T), p[1:-1].astype(np.int64)


def _edge_perm(m, k):
    """Forced pivot rows on the edges of the leaf: the last row of the matrix, the
    first and last row of a workgroup's chunk, a row inside the top w rows (the
    finish kernel's sources and destinations overlap), and a row that stays."""
    R, w = _r(), _w()
    want = [m - 1, 5 % m, 2, R - 1, R, 2 * R - 1, 2 * R, 0, w - 1]
    first, seen = [], set()
    for j in range(k):
        x = want[j] if j < len(want) else m - 2 - j
        x %= m
        while x in seen:
            x = (x + 1) % m
        seen.add(x)
        first.append(x)
    return LW.forced_perm(m, k, first)


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_lu_leaf_kernel(dtype):
    """The leaf alone (n <= w): m on every edge of the rows-per-workgroup chunk, n
    on every edge of the panel width, aligned and padded; random and forced-pivot
    inputs."""
    npdt = NPDT[dtype]
    w, R = _w(), _r()
    bad = []
    for m in (1, 2, w - 1, w, w + 1, R - 1, R, R + 1, 2 * R + 3):
        for n in (1, 2, w - 1, w):
            if n > m:
                continue
            A = LW.random_matrix(m, n, 1000 + 7 * m + n, npdt)
            for pad in (False, True):
                why, _ = LW.accept(A, *_matrix_lu(dtype, A, pad))
                if why:
                    bad.append((m, n, "padded" if pad else "aligned", why))
            perm = _edge_perm(m, n)
            Af, L0, U0 = LW.forced_input(m, n, perm, m + n, npdt)
            why = LW.check_forced(Af, *_matrix_lu(dtype, Af, True), perm, L0, U0)
            if why:
                bad.append((m, n, "forced", why))
    assert not bad, f"{len(bad)} cases: {bad}"


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_lu_recursion(dtype):
    """The column recursion: the first split (17), ragged halves (33 x 31), a Trsm
    and GEMM of every kind (129, 515), tall, wide (the n > m tail) and more than two
    workgroups per leaf; forced pivots at 530 x 130 and 37 x 60."""
    npdt = NPDT[dtype]
    R = _r()
    bad = []
    for (m, n) in [(17, 17), (33, 31), (129, 129), (300, 37), (37, 300), (2 * R + 3, 145), (515, 515)]:
        A = LW.random_matrix(m, n, 2000 + m + n, npdt)
        why, _ = LW.accept(A, *_matrix_lu(dtype, A, m % 2 == 1))
        if why:
            bad.append((m, n, why))
    for (m, n) in [(530, 130), (37, 60)]:
        perm = _edge_perm(m, min(m, n))
        Af, L0, U0 = LW.forced_input(m, n, perm, m + n, npdt)
        why = LW.check_forced(Af, *_matrix_lu(dtype, Af, False), perm, L0, U0)
        if why:
            bad.append((m, n, "forced", why))
    assert not bad, bad


def test_lu_singular():
    """An exactly zero column c (the first, the first of the second leaf, the last)
    raises SingularMatrixError naming column c + 1; two equal rows of a forced-pivot
    input make the last pivot exactly zero; a valid factorization afterwards passes."""
    n, w = 70, _w()
    g = el.Grid()
    A = LW.random_matrix(n, n, 9, np.float64)
    for c in (0, w, n - 1):
        Az = A.copy()
        Az[:, c] = 0
        D = el.DistMatrix(g, el.F64, height=n, width=n)
        D.set_local(Az)
        with pytest.raises(el.SingularMatrixError, match=rf"column {c + 1}$"):
            el.LU(D)
        with pytest.raises(el.SingularMatrixError, match=rf"column {c + 1}$"):
            _matrix_lu(el.F64, Az, False)
    perm = _edge_perm(n, n)
    Af, _, _ = LW.forced_input(n, n, perm, 3, np.float64)
    Af[perm[n - 1]] = Af[perm[5]]
    with pytest.raises(el.SingularMatrixError, match=rf"column {n}$"):
        _matrix_lu(el.F64, Af, False)
    why, _ = LW.accept(A, *_matrix_lu(el.F64, A, False))
    assert why is None, why


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_lu_nan_rule(dtype):
    """The documented pivot rule on the GPU leaf: a NaN never beats a number, also
    where the NaN sits in row 0 of a wave or of a workgroup (m <= R: one workgroup;
    2R + 3: three, with a NaN in thread 0 of the first two); a column with nothing
    but zeros and NaNs left reports the zero pivot of that column."""
    npdt = NPDT[dtype]
    w, R = _w(), _r()
    for (m, n) in ((R, 4), (R + 1, w), (2 * R + 3, w), (2 * R + 3, 40)):
        A, Z = LW.nan_inputs(m, n, 77 + m + n, npdt, R)
        why = LW.check_nan_rule(A, *_matrix_lu(dtype, A, False))
        assert why is None, (m, n, why)
        with pytest.raises(el.SingularMatrixError, match=r"column 2$"):
            _matrix_lu(dtype, Z, False)


@pytest.mark.parametrize("dtype", BOTH_TYPES)
def test_permutation_bits(dtype):
    """1 x 1 GPU grid: PermuteRows then InversePermuteRows is bit-identical to the
    input (-0.0 and NaN payloads included); PermuteRows equals numpy indexing by
    explicit_vector()."""
    npdt = NPDT[dtype]
    g = el.Grid()
    m = 300
    D = el.DistMatrix(g, dtype, height=m, width=m)
    D.set_local(LW.random_matrix(m, m, 4, npdt))
    P = el.LU(D)
    assert P.Height() == m
    v = P.explicit_vector()
    assert sorted(v.tolist()) == list(range(m)) and not np.array_equal(v, np.arange(m))
    B0 = LW.payload_matrix(m, 9, 5, npdt)
    for (U, V) in ((el.MC, el.MR), (el.STAR, el.VR)):
        B = el.DistMatrix(g, dtype, U, V, height=m, width=9)
        B.set_local(B0)
        P.PermuteRows(B)
        assert np.array_equal(_bits(B.get_local()), _bits(B0[v]))
        P.InversePermuteRows(B)
        assert np.array_equal(_bits(B.get_local()), _bits(B0))


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("n", [70, 515])
def test_lu_solves(dtype, n):
    """el.LU through the shared acceptance, then LUSolveAfter NORMAL / TRANSPOSE /
    ADJOINT and LinearSolve with 9 right-hand sides within the reference's bound."""
    npdt = NPDT[dtype]
    g = el.Grid()
    A = LW.random_matrix(n, n, n, npdt)
    D = el.DistMatrix(g, dtype, height=n, width=n)
    D.set_local(A)
    P = el.LU(D)
    why, _ = LW.accept(A, D.get_local(), P.swap_dests())
    assert why is None, why

    def dist(M, U=el.MC, V=el.MR):
        X = el.DistMatrix(g, dtype, U, V, height=M.shape[0], width=M.shape[1])
        X.set_local(M)
        return X
    LW.check_solves(el, g, el.GPU, dtype, n, 9, n + 1, dist)


def test_lu_argument_checks():
    g = el.Grid()
    A = el.DistMatrix(g, el.F64, height=6, width=5)
    A.set_local(LW.random_matrix(6, 5, 1, np.float64))
    P = el.LU(A)
    B = el.DistMatrix(g, el.F64, height=6, width=2)
    with pytest.raises(L.LogicError, match="A must be square"):
        el.LUSolveAfter(el.NORMAL, A, P, B)
    S = el.DistMatrix(g, el.F64, height=5, width=5)
    S.set_local(LW.random_matrix(5, 5, 2, np.float64))
    P5 = el.LU(S)
    with pytest.raises(L.LogicError, match="A and B must be the same height"):
        el.LUSolveAfter(el.NORMAL, S, P5, B)
    H = el.DistMatrix(g, el.BF16, height=4, width=4)
    with pytest.raises(L.LogicError, match="LU: only float and double are supported"):
        el.LU(H)
    t = torch.zeros(64, dtype=torch.float64).cuda()
    piv = torch.zeros(4, dtype=torch.int32).cuda()
    with pytest.raises(L.LogicError, match="LU: only float and double are supported"):
        L.call("elx_matrix_lu", el.BF16, el.GPU, 4, 4, t.data_ptr(), 4, piv.data_ptr(), None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_lu", el.F64, el.GPU, 4, 4, t.data_ptr(), 3, piv.data_ptr(), None)
    L.call("elx_device_synchronize")
    assert (t.cpu().numpy() == 0).all()  # nothing was launched


def _need_gpus(world):
    return pytest.mark.skipif(el.device_count() < world, reason=f"needs >= {world} GPUs (one RCCL rank per GPU)")


@pytest.mark.parametrize("world,height", [pytest.param(2, 1, marks=_need_gpus(2)),
                                          pytest.param(2, 2, marks=_need_gpus(2))])
def test_gpu_lu_rccl(world, height):
    """The distributed driver over RCCL on 1 x 2 and 2 x 1 grids, n = 150, nb = 32:
    the panel staging, the device-side row exchange and the updates on views."""
    import os
    os.environ["ELX_TEST_BACKEND"] = "rccl"
    try:
        mp.spawn(LW.lu_worker, args=(world, _port(), height, el.GPU, el.F64, [(150, 150)], 32, 51), nprocs=world,
                 join=True)
    finally:
        os.environ.pop("ELX_TEST_BACKEND", None)


def test_gpu_lu_host_staged_grid():
    """The same driver on a 2 x 2 grid of ranks sharing one GPU (host-staged
    collectives): the row exchange kernels with more than one process row."""
    mp.spawn(LW.lu_worker, args=(4, _port(), 2, el.GPU, el.F64, [(45, 45), (45, 20)], 16, 53), nprocs=4, join=True)
