"""Level 2 without a GPU: the host loops behind Device::CPU through the raw-pointer C
ABI at every shape the kernels' launch constants make interesting, the distributed
drivers over gloo, the argument checks and the drop-in C++ surface.  The bounds are
stated in _level2_workers."""
import os
import random
import shutil
import socket
import subprocess

import numpy as np
import pytest
import torch.multiprocessing as mp

import _level2_workers as W
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, C, T = (int(L.lib().elx_level2_gemv_rows()), int(L.lib().elx_level2_gemv_cols()),
           int(L.lib().elx_level2_symv_tile()))
ALL_TYPES = [el.F64, el.F32, el.F16, el.BF16]
REAL_TYPES = [el.F64, el.F32]
INCS = [(1, 1), (3, 1), (1, 3), (3, 3)]
DIST_SIZES = [(37, 29), (2 * 128 + 5, 2 * 128 + 3)]  # the second is over twice the default Blocksize()


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


def split_shape(trans):
    """the shape that forces the split path of one orientation."""
    return (40 * R, 3) if trans else (17, 40 * C)


def test_constants_and_split_rule():
    assert R > 0 and C > 0 and T > 0
    assert el.Blocksize() == 128 and DIST_SIZES[1][0] > 2 * el.Blocksize()
    for trans in (False, True):
        o = el.TRANSPOSE if trans else el.NORMAL
        m, n = split_shape(trans)
        assert int(L.lib().elx_level2_gemv_splits(o, m, n)) > 1, "the split shape must take the split path"
        assert int(L.lib().elx_level2_gemv_splits(o, 65, 2)) == 1, "a small shape must take the single launch"
    # enough workgroups already: one launch
    assert int(L.lib().elx_level2_gemv_splits(el.NORMAL, 256 * R, 4 * C)) == 1
    assert int(L.lib().elx_level2_gemv_splits(el.TRANSPOSE, 4 * R, 4096)) == 1


def test_reference_meets_the_bounds():
    """The bounds are reachable: a numpy restatement of Gemv in each accumulation type,
    as a forward loop and as a pairwise sum, stays inside them at every shape the other
    tests use (Symv is the same sum on the symmetrized matrix, so its sizes are run as
    square Gemvs); the rank updates restated with three roundings stay inside theirs."""
    shapes = sorted(set(W.gemv_shapes(R, C) + [split_shape(False), split_shape(True)] + DIST_SIZES +
                        [(n, n) for n in W.symv_sizes(T)]))
    for fmt in ("f64", "f32", "f16", "bf16"):
        for (m, n) in shapes:
            A = W.rand(fmt, m, n, 3 + m + n)
            for trans in (False, True):
                k, ylen = (m, n) if trans else (n, m)
                x, y = W.rand(fmt, k, 1, 5)[:, 0], W.rand(fmt, ylen, 1, 7)[:, 0]
                ref, S = W.gemv_ref(trans, 0.75, A, x, -0.5, y)
                for pairwise in (False, True):
                    got = W.restate_gemv(fmt, trans, 0.75, A, x, -0.5, y, pairwise)
                    assert (np.abs(got - ref) <= W.gemv_bound(fmt, k, S, ref)).all(), (fmt, m, n, trans, pairwise)
    for fmt in ("f64", "f32"):
        acc = W.ACC[fmt]
        for (m, n) in [(65, 63), (2 * T + 1, 2 * T + 1)]:
            A, x, y = W.rand(fmt, m, n, 1), W.rand(fmt, m, 1, 2)[:, 0], W.rand(fmt, n, 1, 3)[:, 0]
            for terms in (0, 2) if m == n else (0,):
                Aref, base, _ = W.update_ref(terms, True, 0.75, x, y, A)
                u = (acc(0.75) * x.astype(acc)).astype(acc)
                got = (A.astype(acc) + np.outer(u, y.astype(acc)).astype(acc)).astype(acc)
                if terms == 2:
                    v = (acc(0.75) * y.astype(acc)).astype(acc)
                    got = (got + np.outer(v, x.astype(acc)).astype(acc)).astype(acc)
                got = np.where(W.tri_mask(True, m, n) | (terms == 0), got, A)
                assert (np.abs(got - Aref) <= 4 * W.eps_acc(fmt) * base).all(), (fmt, m, n, terms)


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("dtype", ALL_TYPES)
def test_host_gemv(dtype, trans):
    """Every edge shape, lda = m and m + 3 with the base off by one element and NaN in
    all padding, strides 1 and 3, guards around y; the split shapes; the integer cases."""
    for q, (m, n) in enumerate(W.gemv_shapes(R, C) + [split_shape(trans)]):
        incx, incy = INCS[q % 4]
        W.check_gemv(el.CPU, dtype, trans, m, n, False, incx, incy, 11 + q)
        W.check_gemv(el.CPU, dtype, trans, m, n, True, incy, incx, 13 + q)
        if q % 3 == 0 or max(m, n) > 2 * R + 3:
            W.check_gemv(el.CPU, dtype, trans, m, n, q % 2 == 0, incx, incy, 17 + q, exact=True)
    W.check_gemv_conventions(el.CPU, dtype)


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("dtype", REAL_TYPES)
def test_host_symv(dtype, lower):
    for q, n in enumerate(W.symv_sizes(T)):
        W.check_symv(el.CPU, dtype, lower, n, False, 21 + q)
        W.check_symv(el.CPU, dtype, lower, n, True, 23 + q)
        W.check_symv(el.CPU, dtype, lower, n, q % 2 == 0, 27 + q, exact=True)
    for imap in W.SYMV_MAPS:
        for (m, n) in [(T + 1, 2 * T + 1), (2 * T + 1, T - 1), (5, 3)]:
            W.check_symv_accumulate(el.CPU, dtype, lower, m, n, imap, 29)


@pytest.mark.parametrize("terms", [0, 1, 2])
@pytest.mark.parametrize("dtype", REAL_TYPES)
def test_host_updates(dtype, terms):
    """Ger on the Gemv shapes, Syr and Syr2 on the Symv sizes and both triangles: the
    other triangle and all padding compared by bits before and after."""
    if terms == 0:
        for q, (m, n) in enumerate(W.gemv_shapes(R, C)):
            W.check_update(el.CPU, dtype, 0, True, m, n, q % 2 == 1, q % 3 == 0, 31 + q, exact=q % 4 == 0)
        return
    for q, n in enumerate(W.symv_sizes(T)):
        for lower in (True, False):
            W.check_update(el.CPU, dtype, terms, lower, n, n, False, q % 2 == 0, 37 + q)
            W.check_update(el.CPU, dtype, terms, lower, n, n, True, q % 2 == 1, 41 + q, exact=q % 2 == 0)


@pytest.mark.parametrize("world,height", [(2, 1), (2, 2), (4, 2), (8, 2)])
def test_dist_level2(world, height):
    """Every driver over gloo on 1 x 2, 2 x 1, 2 x 2 and 2 x 4 grids of Device::CPU
    matrices (see level2_worker)."""
    mp.spawn(W.level2_worker, args=(world, _port(), height, el.CPU, el.F64, DIST_SIZES, 3), nprocs=world, join=True)


@pytest.mark.parametrize("dtype", [el.F16, el.BF16])
def test_dist_gemv_16bit(dtype):
    """The distributed Gemv on 2-byte elements on a 2 x 2 grid: the redistributions of
    every vector form, under the bound that allows one storage rounding per stage (see
    gemv16_worker)."""
    mp.spawn(W.gemv16_worker, args=(4, _port(), 2, el.CPU, dtype, 37, 29, 7), nprocs=4, join=True)


def test_dist_level2_f32():
    mp.spawn(W.level2_worker, args=(4, _port(), 2, el.CPU, el.F32, DIST_SIZES[:1], 5), nprocs=4, join=True)


def _dm(g, dtype, h, w, U=el.MC, V=el.MR, device=el.CPU):
    D = el.DistMatrix(g, dtype, U, V, device, height=h, width=w)
    el.Fill(D, 1.0)
    return D


def test_argument_checks():
    g, g2 = el.Grid(), el.Grid()
    A, x, y = _dm(g, el.F64, 37, 29), _dm(g, el.F64, 29, 1), _dm(g, el.F64, 37, 1)
    S, v = _dm(g, el.F64, 37, 37), _dm(g, el.F64, 37, 1)
    with pytest.raises(L.LogicError, match=r"Nonconformal Gemv: A ~ 37 x 29, x ~ 30 x 1, y ~ 37 x 1"):
        el.Gemv(el.NORMAL, 1.0, A, _dm(g, el.F64, 30, 1), 0.0, y)
    with pytest.raises(L.LogicError, match=r"Nonconformal Gemv: A ~ 37 x 29, x ~ 29 x 1, y ~ 37 x 1"):
        el.Gemv(el.TRANSPOSE, 1.0, A, x, 0.0, y)
    with pytest.raises(L.LogicError, match=r"Nonconformal Gemv: .*x ~ 29 x 2"):
        el.Gemv(el.NORMAL, 1.0, A, _dm(g, el.F64, 29, 2), 0.0, y)
    with pytest.raises(L.LogicError, match=r"Nonconformal Ger: A ~ 37 x 29, x ~ 29 x 1, y ~ 37 x 1"):
        el.Ger(1.0, x, y, A)
    with pytest.raises(L.LogicError, match=r"A must be square: A ~ 37 x 29"):
        el.Symv(el.LOWER, 1.0, A, x, 0.0, y)
    with pytest.raises(L.LogicError, match=r"A must be square: A ~ 37 x 29"):
        el.Syr(el.LOWER, 1.0, y, A)
    with pytest.raises(L.LogicError, match=r"Nonconformal Symv: A ~ 37 x 37, x ~ 29 x 1, y ~ 37 x 1"):
        el.Symv(el.LOWER, 1.0, S, x, 0.0, y)
    with pytest.raises(L.LogicError, match=r"Nonconformal Syr: A ~ 37 x 37, x ~ 29 x 1"):
        el.Syr(el.UPPER, 1.0, x, S)
    with pytest.raises(L.LogicError, match=r"Nonconformal Syr2: A ~ 37 x 37, x ~ 37 x 1, y ~ 29 x 1"):
        el.Syr2(el.UPPER, 1.0, v, x, S)
    with pytest.raises(L.LogicError, match="mixed types"):
        el.Gemv(el.NORMAL, 1.0, A, _dm(g, el.F32, 29, 1), 0.0, y)
    with pytest.raises(L.LogicError, match="different grids"):
        el.Gemv(el.NORMAL, 1.0, A, _dm(g2, el.F64, 29, 1), 0.0, y)
    with pytest.raises(L.LogicError, match="different grids"):
        el.Syr2(el.LOWER, 1.0, v, _dm(g2, el.F64, 37, 1), S)
    with pytest.raises(L.LogicError, match="bad UpperOrLower"):
        el.Symv(7, 1.0, S, v, 0.0, y)
    # the four routines other than Gemv take float and double only
    H, hv = _dm(g, el.BF16, 8, 8), _dm(g, el.BF16, 8, 1)
    for name, fn in (("Ger", lambda: el.Ger(1.0, hv, hv, H)), ("Symv", lambda: el.Symv(el.LOWER, 1.0, H, hv, 0.0, hv)),
                     ("Syr", lambda: el.Syr(el.LOWER, 1.0, hv, H)),
                     ("Syr2", lambda: el.Syr2(el.LOWER, 1.0, hv, hv, H))):
        with pytest.raises(L.LogicError, match=f"{name}: only float and double are supported"):
            fn()
    buf = np.zeros(16, np.uint16)
    with pytest.raises(L.LogicError, match="Symv: only float and double are supported"):
        L.call("elx_matrix_symv", el.F16, el.CPU, el.LOWER, 4, 1.0, buf.ctypes.data, 4, buf.ctypes.data, 1, 0.0,
               buf.ctypes.data, 1, None)
    with pytest.raises(L.LogicError, match="leading dimension 3 < 4"):
        L.call("elx_matrix_gemv", el.F64, el.CPU, el.NORMAL, 4, 4, 1.0, buf.ctypes.data, 3, buf.ctypes.data, 1, 0.0,
               buf.ctypes.data, 1, None)
    with pytest.raises(L.LogicError, match="stride 0 < 1"):
        L.call("elx_matrix_gemv", el.F64, el.CPU, el.NORMAL, 1, 1, 1.0, buf.ctypes.data, 1, buf.ctypes.data, 0, 0.0,
               buf.ctypes.data, 1, None)
    assert (buf == 0).all()


def test_local_gemv_and_resize():
    """LocalGemv on spread operands, its alignment check, and the beta-less overload."""
    g = el.Grid()
    A0, x0 = W.rand("f64", 9, 7, 1), W.rand("f64", 7, 1, 2)
    A, x = W.dist_of(el, g, el.F64, el.CPU, A0), W.dist_of(el, g, el.F64, el.CPU, x0, el.MR, el.STAR)
    y = el.DistMatrix(g, el.F64, el.MC, el.STAR, el.CPU, height=9, width=1)
    el.Fill(y, float("nan"))
    el.LocalGemv(el.NORMAL, 2.0, A, x, 0.0, y)
    assert np.allclose(y.get_local(), 2.0 * A0 @ x0, rtol=0, atol=1e-14)
    with pytest.raises(L.LogicError, match="LocalGemv: x and y must be spread"):
        el.LocalGemv(el.NORMAL, 2.0, A, W.dist_of(el, g, el.F64, el.CPU, x0), 0.0, y)
    z = el.DistMatrix(g, el.F64, el.MC, el.MR, el.CPU, height=3, width=3)
    el.Fill(z, float("nan"))
    el.Gemv(el.TRANSPOSE, 1.0, A, W.dist_of(el, g, el.F64, el.CPU, W.rand("f64", 9, 1, 3)), None, z)
    assert (z.Height(), z.Width()) == (7, 1)
    assert np.allclose(z.get_local(), A0.T @ W.rand("f64", 9, 1, 3), rtol=0, atol=1e-14)


def _build_and_run(tmp_path, name, extra=(), args=()):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / name
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra, "-I",
                           os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o",
                           str(exe), "-L", libdir, "-lelemental_amd", f"-Wl,-rpath,{libdir}"])
    res = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "OK" in res.stdout


def test_cpp_level2_api(tmp_path):
    """Every new El:: overload once through include/El.hpp on Device::CPU, one known
    answer each."""
    _build_and_run(tmp_path, "test_level2_api")


def test_cpp_level2_host_shapes(tmp_path):
    """The stand-alone program over the C ABI (its own main; it can be linked against a
    sanitized host build): the host loops and the drivers' index arithmetic."""
    _build_and_run(tmp_path, "level2_host_check")
