"""Level 2 on the GPU: the gfx950 kernels (gemv_n, gemv_t, symv, ger, syr, syr2 and the
fixed-order reduce) through the raw-pointer C ABI at every shape their launch
constants make interesting, the drivers on GPU DistMatrices, and the C++ surface on
Device::GPU.  The checks and their bounds are the ones of the CPU tests
(_level2_workers)."""
import os
import random
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import _level2_workers as W
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

R, C, T = (int(L.lib().elx_level2_gemv_rows()), int(L.lib().elx_level2_gemv_cols()),
           int(L.lib().elx_level2_symv_tile()))
ALL_TYPES = [el.F64, el.F32, el.F16, el.BF16]
REAL_TYPES = [el.F64, el.F32]
INCS = [(1, 1), (3, 1), (1, 3), (3, 3)]
DIST_SIZES = [(37, 29), (2 * 128 + 5, 2 * 128 + 3)]


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


def split_shape(trans):
    return (40 * R, 3) if trans else (17, 40 * C)


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_gpu_gemv(dtype, trans):
    """Every edge shape on the 16-byte path (lda = m) and on the element path (lda = m +
    3, the base off by one element, NaN in all padding), strides 1 and 3, guards around
    y, bit-identical reruns; the shape that takes the split path, asserted through the
    plan query, so the partials and the reduce launch are what is checked there."""
    o = el.TRANSPOSE if trans else el.NORMAL
    unsplit = 0
    for q, (m, n) in enumerate(W.gemv_shapes(R, C) + [split_shape(trans)]):
        incx, incy = INCS[q % 4]
        W.check_gemv(el.GPU, dtype, trans, m, n, False, incx, incy, 11 + q)
        W.check_gemv(el.GPU, dtype, trans, m, n, True, incy, incx, 13 + q)
        if q % 3 == 0 or max(m, n) > 2 * R + 3:
            W.check_gemv(el.GPU, dtype, trans, m, n, q % 2 == 0, incx, incy, 17 + q, exact=True)
        unsplit += int(L.lib().elx_level2_gemv_splits(o, m, n)) == 1
    assert int(L.lib().elx_level2_gemv_splits(o, *split_shape(trans))) > 1
    assert unsplit > 0, "no shape took the single launch"
    W.check_gemv_conventions(el.GPU, dtype)


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("dtype", REAL_TYPES)
def test_gpu_symv(dtype, lower):
    """Every element of the other strict triangle is NaN; padded and unaligned; beta = 0
    over a NaN y; equal to Gemv on the symmetrized matrix within the bound; reruns
    bit-identical; SymvAccumulate with the two non-trivial index maps."""
    for q, n in enumerate(W.symv_sizes(T)):
        W.check_symv(el.GPU, dtype, lower, n, False, 21 + q)
        W.check_symv(el.GPU, dtype, lower, n, True, 23 + q)
        W.check_symv(el.GPU, dtype, lower, n, q % 2 == 0, 27 + q, exact=True)
    for imap in W.SYMV_MAPS:
        for (m, n) in [(T + 1, 2 * T + 1), (2 * T + 1, T - 1), (5, 3)]:
            W.check_symv_accumulate(el.GPU, dtype, lower, m, n, imap, 29)


@pytest.mark.parametrize("terms", [0, 1, 2])
@pytest.mark.parametrize("dtype", REAL_TYPES)
def test_gpu_updates(dtype, terms):
    """Ger on the Gemv shapes, Syr and Syr2 on the Symv sizes and both triangles: the
    other triangle and all padding compared by bits before and after."""
    if terms == 0:
        for q, (m, n) in enumerate(W.gemv_shapes(R, C)):
            W.check_update(el.GPU, dtype, 0, True, m, n, q % 2 == 1, q % 3 == 0, 31 + q, exact=q % 4 == 0)
        return
    for q, n in enumerate(W.symv_sizes(T)):
        for lower in (True, False):
            W.check_update(el.GPU, dtype, terms, lower, n, n, False, q % 2 == 0, 37 + q)
            W.check_update(el.GPU, dtype, terms, lower, n, n, True, q % 2 == 1, 41 + q, exact=q % 2 == 0)


def test_gpu_level2_one_rank():
    """The drivers on one rank (the 1 x 1 grid: Symv goes straight to the local kernel)."""
    mp.spawn(W.level2_worker, args=(1, _port(), 1, el.GPU, el.F64, DIST_SIZES, 3), nprocs=1, join=True)


def _need_gpus(world):
    return pytest.mark.skipif(el.device_count() < world, reason=f"needs >= {world} GPUs (one RCCL rank per GPU)")


@pytest.mark.parametrize("world,height", [pytest.param(2, 1, marks=_need_gpus(2)),
                                          pytest.param(4, 2, marks=_need_gpus(4))])
def test_gpu_level2_rccl(world, height):
    """The drivers over RCCL on 1 x 2 and 2 x 2 grids, one GPU per rank."""
    os.environ["ELX_TEST_BACKEND"] = "rccl"
    try:
        mp.spawn(W.level2_worker, args=(world, _port(), height, el.GPU, el.F64, DIST_SIZES, 7), nprocs=world,
                 join=True)
    finally:
        os.environ.pop("ELX_TEST_BACKEND", None)


def test_gpu_level2_host_staged_grid():
    """The same drivers on a 2 x 2 grid of ranks sharing one GPU (host-staged
    collectives), f32."""
    mp.spawn(W.level2_worker, args=(4, _port(), 2, el.GPU, el.F32, DIST_SIZES[:1], 9), nprocs=4, join=True)


def test_gpu_dist_gemv_bf16():
    """The distributed Gemv on bf16 GPU matrices, 2 x 2 ranks sharing one GPU: the
    redistributions for 2-byte elements under the per-stage rounding bound."""
    mp.spawn(W.gemv16_worker, args=(4, _port(), 2, el.GPU, el.BF16, 37, 29, 7), nprocs=4, join=True)


def test_gpu_mixed_devices():
    """Operands on different devices are refused (a GPU matrix needs a device to exist,
    so this argument check lives here)."""
    g = el.Grid()

    def dm(h, w, device):
        D = el.DistMatrix(g, el.F64, el.MC, el.MR, device, height=h, width=w)
        el.Fill(D, 1.0)
        return D

    with pytest.raises(L.LogicError, match="mixed devices"):
        el.Gemv(el.NORMAL, 1.0, dm(8, 8, el.CPU), dm(8, 1, el.GPU), 0.0, dm(8, 1, el.CPU))
    with pytest.raises(L.LogicError, match="mixed devices"):
        el.Syr(el.LOWER, 1.0, dm(8, 1, el.CPU), dm(8, 8, el.GPU))


def test_gpu_cpp_level2_api():
    """tests/cpp/test_level2_api.cpp built with -DEL_TEST_GPU by __graft_entry__.build():
    every new El:: overload once on Device::GPU."""
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp", "_build", "test_level2_api_gpu")
    assert os.path.exists(exe), f"{exe} missing: run __graft_entry__.build()"
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "OK" in res.stdout
