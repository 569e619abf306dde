"""Trsm on the GPU, every local path: trsm_kernel<T, LDS, IDENT> and
tri_inverse_batched_kernel (trsm.hip) through elx_matrix_trsm and El::Trsm on the
exact family of _trsm_cases (bit for bit, NaN-masked, padded, the path checked),
the argument checks, and the distributed driver per column."""
import random
import socket

import pytest
import torch.multiprocessing as mp

import _dist_workers as W
import _trsm_cases as TC
from elemental_amd import _lib as L
from elemental_amd import el

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


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


def _spawn(fn, world, *args):
    mp.spawn(fn, args=(world, _port()) + args, nprocs=world, join=True)


@pytest.mark.parametrize("uplo", [el.LOWER, el.UPPER])
@pytest.mark.parametrize("dtype", [el.F64, el.F32])
def test_trsm_kernel_exact(dtype, uplo):
    """elx_matrix_trsm (LEFT) at every shape of _trsm_cases.PATHS: substitution and
    inverse, in LDS and on global memory, the 8-row batch and its remainder, dead
    lanes in a second wave, the LDS sizes on both sides of 64 KiB and at the
    limit.  NORMAL / TRANSPOSE x NON_UNIT / UNIT, aligned (lda = ldb = m) and
    padded (lda = m + 3, ldb = m + 1, bases one element in, padding NaN).  Each
    result equals X in every bit, A and B's padding are unchanged, and the launch
    is the one kernels.hpp trsm_plan names for the shape."""
    TC.run_matrix(el.GPU, el.LEFT, TC.KERNEL_SHAPES, (dtype,), (uplo,))


def test_trsm_matrix_right_exact():
    """side = RIGHT of the Matrix entry: B := 2 B op(tri(A))^-1 through the transposes."""
    TC.run_matrix(el.GPU, el.RIGHT, TC.RIGHT_SHAPES)


def test_trsm_argument_checks():
    t = torch.zeros(64, dtype=torch.float64).cuda()
    p = t.data_ptr()
    with pytest.raises(L.LogicError, match="only float and double"):
        L.call("elx_matrix_trsm", el.BF16, el.GPU, el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 4, 4, 1.0, p, 4, p + 128,
               4, None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_trsm", el.F64, el.GPU, el.LEFT, el.LOWER, el.NORMAL, el.NON_UNIT, 4, 4, 1.0, p, 3, p + 128,
               4, None)
    with pytest.raises(L.LogicError, match="leading dimension"):
        L.call("elx_matrix_trsm", el.F64, el.GPU, el.RIGHT, el.LOWER, el.NORMAL, el.NON_UNIT, 3, 4, 1.0, p, 3, p + 128,
               3, None)
    with pytest.raises(L.LogicError, match="Trsm: bad UnitOrNonUnit"):
        L.call("elx_matrix_trsm", el.F64, el.GPU, el.LEFT, el.LOWER, el.NORMAL, 2, 4, 4, 1.0, p, 4, p + 128, 4, None)
    L.call("elx_device_synchronize")
    assert (t.cpu().numpy() == 0).all()  # nothing was launched


@pytest.mark.parametrize("updates", ["gemm", "summa"])
def test_trsm_batched_all_sixteen(updates, monkeypatch):
    """El::Trsm on a 1x1 grid, nb = 16, (45, 70): the width 70 >= 4 nb takes the
    batched path (one tri_inverse_batched launch over three blocks, a ragged 13),
    every side / uplo / orientation / diag, f64 and f32; updates between blocks as
    direct GEMMs, or (ELX_TRSM_SUMMA=1) through the SUMMA pipeline."""
    if updates == "summa":
        monkeypatch.setenv("ELX_TRSM_SUMMA", "1")
    TC.run_dist(el.GPU, TC.all_sixteen(el.F64, 45, 70) + TC.all_sixteen(el.F32, 45, 70), 16)


def test_trsm_batched_flat(monkeypatch):
    """The same under ELX_TRSM_FLAT=1 (the nb-step sweep), which the library reads
    once per process: in a spawned one."""
    monkeypatch.setenv("ELX_TRSM_FLAT", "1")
    mp.spawn(TC.dist_worker, args=(el.GPU, TC.all_sixteen(el.F64, 45, 70) + TC.all_sixteen(el.F32, 45, 70), 16, None),
             nprocs=1, join=True)


def _left(dtype, m, n, combos):
    return [(dtype, el.LEFT, uplo, orient, diag, m, n) for (uplo, orient, diag) in combos]


ALTERNATING = [(el.LOWER, el.NORMAL, el.NON_UNIT), (el.LOWER, el.TRANSPOSE, el.UNIT),
               (el.UPPER, el.NORMAL, el.UNIT), (el.UPPER, el.TRANSPOSE, el.NON_UNIT)]


def test_trsm_batched_dead_second_block():
    """nb = 80, (200, 320): batched with two workgroups per diagonal block
    (blockIdx.x = 0, 1); the last block has 40 rows, so its second workgroup has
    no live lane and only keeps the barriers."""
    TC.run_dist(el.GPU, _left(el.F64, 200, 320, ALTERNATING) + _left(el.F32, 200, 320, ALTERNATING), 80)


def test_trsm_batched_raised_lds_f32():
    """f32, nb = 300, (700, 1200): batched with 78 000 B of dynamic LDS per
    workgroup, above 64 KiB (tri_inverse_lds_ok raises the kernel's limit)."""
    TC.run_dist(el.GPU, _left(el.F32, 700, 1200, ALTERNATING), 300)


def test_trsm_unbatched_global_f64():
    """f64, nb = 296, (300, 1200): 296 x 65 x 8 B exceeds kTriInverseLdsMax, so
    nothing is batched; exec::Trsm solves the 296-row block by substitution on
    global memory (m > 256) and the ragged 4-row block by inverse and GEMM."""
    TC.run_dist(el.GPU, _left(el.F64, 300, 1200, ALTERNATING), 296)


@pytest.mark.parametrize("dtype", [el.F32, el.F64])
def test_trsm_batched_widened(dtype):
    """Default Blocksize, (2100, 1030): m >= 2048 widens the diagonal blocks to 256
    rows (eight, and a ragged 52).  f32: LOWER / UPPER x NORMAL / TRANSPOSE with
    NON_UNIT and UNIT alternating; f64: LOWER NORMAL and UPPER TRANSPOSE."""
    combos = ALTERNATING if dtype == el.F32 else [ALTERNATING[0], ALTERNATING[3]]
    TC.run_dist(el.GPU, _left(dtype, 2100, 1030, combos), 128, nb=256)


def test_gpu_trsm_distributed_f32():
    _spawn(W.trsm_worker, 1, 1, el.GPU, el.F32, 45, 23, 16, 43)


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1)])
def test_gpu_trsm_distributed_wide(world, height):
    """(45, 160), nb = 16: on 1x1 the batched path; on 1x2 each rank's [*,VR] width
    is 80 >= 4 nb, so every leaf is exec::Trsm's inverse path on a real grid."""
    _spawn(W.trsm_worker, world, height, el.GPU, el.F64, 45, 160, 16, 47)
