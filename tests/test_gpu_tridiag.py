"""El::HermitianTridiag on the GPU: the fused panel kernels (sytrd.hip) through
elx_matrix_hermitian_tridiag, the blocked driver above them, the exact and special
inputs, ApplyQ, ExplicitCondensed and the distributed drivers.

Inputs: symmetric, uniform in [-1, 1], rounded to the type; the triangle the call
must not touch is NaN.  Acceptance (_tridiag_workers.accept): Q rebuilt in float64
from the packed reflectors; finite, 1 <= t <= 2, |t (1 + |u|^2) - 2| <= 10 n eps,
||S - Q T Q^T||_F <= 10 n eps ||S||_F, ||Q^T Q - I||_F <= 10 n eps, max |lambda(T) -
lambda(S)| <= 10 n eps ||S||_2, the other triangle bit-identical."""
import random
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import _tridiag_workers as TW
from _dist_workers import _bits
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NPDT = {el.F64: np.float64, el.F32: np.float32}
BOTH_TYPES = [el.F64, el.F32]
UPLOS = [el.LOWER, el.UPPER]


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
    return int(L.lib().elx_tridiag_panel_cols())


def _r():
    return int(L.lib().elx_tridiag_rows())


def _matrix_tridiag(dtype, A, uplo, pad=False):
    """elx_matrix_hermitian_tridiag on the column-major A with lda = n (aligned) or
    n + 3 and the base one element into the allocation (pad); everything around the
    matrix is NaN, tau has a guard word on either side.  Returns (packed, t) after
    checking that nothing outside the matrix and tau changed (the other triangle is
    compared by the acceptance)."""
    n = A.shape[0]
    k = max(n - 1, 0)
    es = A.dtype.itemsize
    lda, off = (n + 3, 1) if pad else (n, 0)
    buf = np.full(off + lda * n, np.nan, A.dtype)
    buf[off:].reshape(n, lda)[:, :n] = A.T
    t = torch.from_numpy(buf).cuda()
    tau = torch.from_numpy(np.full(k + 2, -7, A.dtype)).cuda()
    torch.cuda.synchronize()
    L.call("elx_matrix_hermitian_tridiag", dtype, el.GPU, uplo, n, t.data_ptr() + off * es, lda,
           tau.data_ptr() + es, None)
    L.call("elx_device_synchronize")
    out = t.cpu().numpy()
    inside = np.zeros(buf.shape, bool)
    inside[off:].reshape(n, lda)[:, :n] = True
    assert np.array_equal(_bits(out[~inside]), _bits(buf[~inside])), "written outside the matrix"
    th = tau.cpu().numpy()
    assert th[0] == -7 and th[-1] == -7, "written outside tau"
    return np.asfortranarray(out[off:].reshape(n, lda)[:, :n].T), th[1:-1].copy()


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("uplo", UPLOS)
def test_tridiag_panel_edges(dtype, uplo):
    """n on every edge of the panel width w, of the Symv tile (128) and of the rows
    per workgroup R; aligned, and lda = n + 3 with the base one element in; nothing
    outside the triangle, tau and the guards written; two runs bit-identical."""
    npdt = NPDT[dtype]
    lower = uplo == el.LOWER
    w, R = _w(), _r()
    bad = []
    for n in sorted({1, 2, 3, w - 1, w, w + 1, w + 2, 2 * w + 1, 127, 128, 129, R - 1, R, R + 1, R + 2, 2 * R + 3}):
        A = TW.one_triangle(TW.random_symmetric(n, 1000 + 7 * n, npdt), lower)
        for pad in (False, True):
            P, t = _matrix_tridiag(dtype, A, uplo, pad)
            why, _ = TW.accept(A, P, t, lower)
            if why:
                bad.append((n, "padded" if pad else "aligned", why))
            # the same call on the same layout again: the same bits
            again = _matrix_tridiag(dtype, A, uplo, pad)
            if not all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(again, (P, t))):
                bad.append((n, "padded" if pad else "aligned", "two runs differ"))
    assert not bad, f"{len(bad)} cases: {bad}"


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("uplo", UPLOS)
@pytest.mark.parametrize("panel", ["fused", "level2"])
def test_tridiag_blocked(dtype, uplo, panel, monkeypatch):
    """Several panels, a ragged last panel and more than two workgroups; the fused
    kernels and the panel composed from the Level-2 routines (ELX_TRIDIAG_PANEL=
    level2, read at every call), each accepted on its own."""
    npdt = NPDT[dtype]
    lower = uplo == el.LOWER
    if panel == "level2":
        monkeypatch.setenv("ELX_TRIDIAG_PANEL", "level2")
    else:
        monkeypatch.delenv("ELX_TRIDIAG_PANEL", raising=False)
    bad = []
    for n in (300, 515):
        A = TW.one_triangle(TW.random_symmetric(n, 2000 + n, npdt), lower)
        why, _ = TW.accept(A, *_matrix_tridiag(dtype, A, uplo, n % 2 == 1), lower)
        if why:
            bad.append((n, why))
    assert not bad, bad


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("uplo", UPLOS)
def test_tridiag_exact_and_special(dtype, uplo):
    """The tridiagonal and diagonal exact cases at n = 2w + 1; a column whose tail is
    exactly zero at positions 0, w and n - 3 gives t = 2; inputs scaled by 2^+-500
    (f64) / 2^+-50 (f32) at n = 70 and 300 pass the acceptance; a NaN in one trailing
    entry propagates and the call returns."""
    npdt = NPDT[dtype]
    lower = uplo == el.LOWER
    w = _w()
    n = 2 * w + 1
    for name, S in TW.exact_inputs(n, 3, npdt):
        TW.check_exact(S, *_matrix_tridiag(dtype, TW.one_triangle(S, lower, 0), uplo), lower)
    for c in (0, w, n - 3):
        A = TW.one_triangle(TW.zero_tail_input(n, c, 5 + c, npdt, lower), lower)
        P, t = _matrix_tridiag(dtype, A, uplo)
        assert t[c if lower else n - 2 - c] == 2, (c, t)
        why, _ = TW.accept(A, P, t, lower)
        assert why is None, (c, why)
    for m in (70, 300):
        for up in (True, False):
            A = TW.one_triangle(TW.scaled_symmetric(m, 21, npdt, up), lower)
            why, _ = TW.accept(A, *_matrix_tridiag(dtype, A, uplo), lower)
            assert why is None, (m, up, why)
    S = TW.random_symmetric(n, 9, npdt)
    S[n - 5, n // 2] = S[n // 2, n - 5] = np.nan
    P, t = _matrix_tridiag(dtype, S, uplo)
    assert np.isnan(t).any() and np.isnan(np.diag(P)).any()


@pytest.mark.parametrize("dtype", BOTH_TYPES)
@pytest.mark.parametrize("n", [70, 515])
def test_tridiag_drivers(dtype, n):
    """el.HermitianTridiag, HermitianTridiagApplyQ and ExplicitCondensed on a 1 x 1
    grid, both uplo."""
    g = el.Grid()
    S = TW.random_symmetric(n, 50 + n, NPDT[dtype])
    for uplo in UPLOS:
        TW.check_drivers(el, g, dtype, el.GPU, S, uplo)


def test_tridiag_argument_checks():
    g = el.Grid()

    def dm(m, n, dtype=el.F64, seed=1):
        D = el.DistMatrix(g, dtype, height=m, width=n)
        if dtype in NPDT:
            D.set_local(np.asfortranarray(TW.random_symmetric(max(m, n), seed, NPDT[dtype])[:m, :n]))
        return D
    A = dm(6, 6)
    t = el.HermitianTridiag(el.LOWER, A)
    with pytest.raises(L.LogicError, match="ApplyQ: only LEFT is supported"):
        el.HermitianTridiagApplyQ(el.RIGHT, el.LOWER, el.NORMAL, A, t, dm(6, 2))
    with pytest.raises(L.LogicError, match="must be square"):
        el.HermitianTridiag(el.LOWER, dm(6, 4))
    with pytest.raises(L.LogicError, match="HermitianTridiag: only float and double are supported"):
        el.HermitianTridiag(el.LOWER, dm(4, 4, el.BF16))
    buf = torch.zeros(64, dtype=torch.float64).cuda()
    with pytest.raises(L.LogicError, match="HermitianTridiag: only float and double are supported"):
        L.call("elx_matrix_hermitian_tridiag", el.BF16, el.GPU, el.LOWER, 4, buf.data_ptr(), 4, buf.data_ptr() + 256,
               None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_hermitian_tridiag", el.F64, el.GPU, el.LOWER, 4, buf.data_ptr(), 3, buf.data_ptr() + 256,
               None)
    with pytest.raises(L.LogicError, match="bad UpperOrLower"):
        L.call("elx_matrix_hermitian_tridiag", el.F64, el.GPU, 77, 4, buf.data_ptr(), 4, buf.data_ptr() + 256, None)
    with pytest.raises(L.LogicError, match="null"):
        L.call("elx_matrix_hermitian_tridiag", el.F64, el.GPU, el.LOWER, 4, buf.data_ptr(), 4, None, None)
    L.call("elx_device_synchronize")
    assert (buf.cpu().numpy() == 0).all()  # nothing was launched


def _need_gpus(world):
    return pytest.mark.skipif(el.device_count() < world, reason=f"needs >= {world} GPUs (one RCCL rank per GPU)")


@pytest.mark.parametrize("world,height", [pytest.param(2, 1, marks=_need_gpus(2)),
                                          pytest.param(2, 2, marks=_need_gpus(2))])
def test_gpu_tridiag_rccl(world, height):
    """The distributed driver over RCCL on 1 x 2 and 2 x 1 grids, n = 150, nb = 32."""
    import os
    os.environ["ELX_TEST_BACKEND"] = "rccl"
    try:
        mp.spawn(TW.tridiag_worker, args=(world, _port(), height, el.GPU, el.F64, [(150, 32)], 51), nprocs=world,
                 join=True)
    finally:
        os.environ.pop("ELX_TEST_BACKEND", None)


def test_gpu_tridiag_host_staged_grid():
    """The same driver on a 2 x 2 grid of ranks sharing one GPU (host-staged
    collectives), n = 45, nb = 16."""
    mp.spawn(TW.tridiag_worker, args=(4, _port(), 2, el.GPU, el.F64, [(45, 16)], 53), nprocs=4, join=True)
