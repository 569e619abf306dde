"""Shared pieces of the Level-2 tests (Gemv, Ger, Symv, Syr, Syr2): inputs, float64
references, the componentwise acceptance bounds, runners for the raw-pointer C ABI on
either device, and the multi-rank workers.

Bounds (k the summation length, eps the epsilon of the accumulation type, S = |alpha|
|A| |x| + |beta| |y_in| componentwise; for Symv |A| of the symmetrized triangle):
any summation order obeys |err| <= gamma_k sum |a_i x_i| with gamma_k ~ k eps / 2, plus
three roundings for alpha, beta and the final add, so the bounds carry a factor of two
over the worst case whatever tiling a kernel chooses.
  f64 / f32       |y - y_ref| <= (k + 3) eps S
  16-bit Gemv     |y - y_ref| <= eps_storage |y_ref| + 2 (k + 3) eps_f32 S + smallest subnormal
  Ger, Syr, Syr2  |A - A_ref| <= 4 eps (|A_in| + |alpha| |x| |y|^T [+ |alpha| |y| |x|^T])
"""
from __future__ import annotations

import traceback

import numpy as np

from _dist_workers import init, finish, _bits

FMT = {0: "f32", 1: "f64", 2: "f16", 3: "bf16"}  # ELX_F32, ELX_F64, ELX_F16, ELX_BF16
STORE = {"f64": np.float64, "f32": np.float32, "f16": np.float16, "bf16": np.uint16}
ACC = {"f64": np.float64, "f32": np.float32, "f16": np.float32, "bf16": np.float32}
EPS_STORE = {"f64": 2.0 ** -52, "f32": 2.0 ** -23, "f16": 2.0 ** -10, "bf16": 2.0 ** -7}
TINY = {"f16": 2.0 ** -24, "bf16": 2.0 ** -133}
EXACT_SCALARS = [(1, 1), (-1, 2), (2, 0), (1, -1)]  # (alpha, beta) of the exact integer cases
SYMV_MAPS = [(1, 2, 0, 3), (0, 3, 2, 2)]  # (i0, is, j0, js) of the SymvAccumulate cases


def eps_acc(fmt):
    return float(np.finfo(ACC[fmt]).eps)


def store(fmt, x):
    """float64 values -> the storage array of the format (one rounding)."""
    import oracle
    return oracle.convert(np.asarray(x, np.float64), "f64", fmt)


def load(fmt, a):
    """storage array -> exact float64 values."""
    import oracle
    return oracle.to_f64(np.asarray(a), fmt)


def nan_of(fmt):
    return np.uint16(0x7FC0) if fmt == "bf16" else STORE[fmt](np.nan)


def rand(fmt, m, n, seed):
    """hash_matrix values in [-1, 1] rounded to the type, as float64."""
    import oracle
    return load(fmt, oracle.hash_matrix(m, n, seed, 0.0, 1.0, "bf16" if fmt == "bf16" else STORE[fmt]))


def ints(m, n, seed):
    """entries in {-2 .. 2}: every partial sum of the tests' lengths is exact in f32."""
    import oracle
    return np.rint(2.0 * oracle.hash_matrix(m, n, seed, 0.0, 1.0, np.float64))


def gemv_shapes(R, C):
    return [(m, n) for m in (1, 2, 63, 64, 65, R - 1, R, R + 1, 2 * R + 3) for n in (1, 2, C - 1, C, C + 1, 2 * C + 3)]


def symv_sizes(T):
    return [1, 2, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3]


# ---- references and bounds -----------------------------------------------------------
def gemv_ref(trans, alpha, A, x, beta, y):
    op = A.T if trans else A
    ref = alpha * (op @ x) + (beta * y if beta != 0 else 0.0)
    S = abs(alpha) * (np.abs(op) @ np.abs(x)) + (abs(beta) * np.abs(y) if beta != 0 else 0.0)
    return ref, S


def gemv_bound(fmt, k, S, ref):
    if fmt in ("f64", "f32"):
        return (k + 3) * eps_acc(fmt) * S
    return EPS_STORE[fmt] * np.abs(ref) + 2 * (k + 3) * eps_acc(fmt) * S + TINY[fmt]


def symmetrize(uplo_lower, A):
    """the symmetric matrix an uplo triangle stands for (the other triangle ignored)."""
    T = np.tril(A) if uplo_lower else np.triu(A)
    return T + T.T - np.diag(np.diag(A))


def tri_mask(lower, m, n, i0=0, istride=1, j0=0, jstride=1, strict=False):
    gi = (i0 + istride * np.arange(m))[:, None]
    gj = (j0 + jstride * np.arange(n))[None, :]
    if lower:
        return gi > gj if strict else gi >= gj
    return gi < gj if strict else gi <= gj


def symv_accumulate_ref(lower, alpha, A, xr, xc, imap):
    """(z_row, z_col, S_row, S_col) of SymvAccumulate on zeroed z: a loop over global
    indices written as masks."""
    m, n = A.shape
    incl, strict = tri_mask(lower, m, n, *imap), tri_mask(lower, m, n, *imap, strict=True)
    Ai, As = np.where(incl, A, 0.0), np.where(strict, A, 0.0)
    return (alpha * (Ai @ xc), alpha * (As.T @ xr), abs(alpha) * (np.abs(Ai) @ np.abs(xc)),
            abs(alpha) * (np.abs(As).T @ np.abs(xr)))


def update_ref(terms, lower, alpha, x, y, A):
    """(A_ref, bound base, mask) of Ger (terms 0) / Syr (1) / Syr2 (2)."""
    m, n = A.shape
    mask = np.ones((m, n), bool) if terms == 0 else tri_mask(lower, m, n)
    upd = alpha * np.outer(x, y)
    base = np.abs(A) + abs(alpha) * np.outer(np.abs(x), np.abs(y))
    if terms == 2:
        upd = upd + alpha * np.outer(y, x)
        base = base + abs(alpha) * np.outer(np.abs(y), np.abs(x))
    return np.where(mask, A + upd, A), base, mask


def restate_sum(fmt, P, pairwise):
    """row sums of the products P (already rounded to the accumulation type), added in
    the accumulation type as a forward loop or as a pairwise tree."""
    acc = ACC[fmt]
    P = P.astype(acc)
    if not pairwise:
        s = np.zeros(P.shape[0], acc)
        for j in range(P.shape[1]):
            s = (s + P[:, j]).astype(acc)
        return s
    while P.shape[1] > 1:
        if P.shape[1] % 2:
            P = np.concatenate([P, np.zeros((P.shape[0], 1), acc)], axis=1)
        P = (P[:, 0::2] + P[:, 1::2]).astype(acc)
    return P[:, 0] if P.shape[1] else np.zeros(P.shape[0], acc)


def restate_gemv(fmt, trans, alpha, A, x, beta, y, pairwise):
    """Gemv restated in numpy in the accumulation type, rounded to the storage type once."""
    acc = ACC[fmt]
    op = (A.T if trans else A).astype(acc)
    s = restate_sum(fmt, (op * x.astype(acc)[None, :]).astype(acc), pairwise)
    v = (acc(alpha) * s).astype(acc)
    if beta != 0:
        v = (v + (acc(beta) * y.astype(acc)).astype(acc)).astype(acc)
    return load(fmt, store(fmt, v.astype(np.float64)))


# ---- the raw-pointer C ABI on either device ----------------------------------------------
class Operand:
    """A strided vector or a column-major matrix inside a flat storage buffer: `off`
    elements of padding in front (1: the base is not 16-byte aligned), NaN in every gap
    and a guard word at either end."""

    def __init__(self, fmt, values, ld=None, inc=1, off=0):
        self.fmt, self.off, self.inc = fmt, off, inc
        v = np.asarray(values, np.float64)
        self.shape = v.shape
        if v.ndim == 2:
            m, n = v.shape
            self.ld = ld if ld is not None else max(m, 1)
            self.idx = (off + 1 + np.arange(m)[:, None] + self.ld * np.arange(n)[None, :]).ravel()
            size = off + 1 + self.ld * max(n, 1) + 1
        else:
            self.ld = None
            self.idx = off + 1 + inc * np.arange(v.shape[0])
            size = off + 1 + inc * max(v.shape[0], 1) + 1
        self.buf = np.full(size, nan_of(fmt), STORE[fmt])
        self.buf[self.idx] = store(fmt, v.ravel())
        self.before = self.buf.copy()

    @property
    def elem_offset(self):
        return self.off + 1

    def values(self):
        return load(self.fmt, self.buf[self.idx]).reshape(self.shape)

    def set_nan(self, mask=None):
        idx = self.idx if mask is None else self.idx[np.asarray(mask).ravel()]
        self.buf[idx] = nan_of(self.fmt)
        self.before = self.buf.copy()

    def untouched_outside(self, written_mask=None):
        """every element outside the operand (padding, gaps, guards) and every element
        of it outside written_mask kept its bits."""
        keep = np.ones(self.buf.size, bool)
        keep[self.idx if written_mask is None else self.idx[np.asarray(written_mask).ravel()]] = False
        return np.array_equal(_bits(self.buf[keep]), _bits(self.before[keep]))

    def unchanged(self):
        return np.array_equal(_bits(self.buf), _bits(self.before))


def run(device, name, ops, make_args):
    """Call the C-ABI function `name`; make_args(ptrs) builds its arguments from each
    operand's first-element address.  On the GPU the buffers are staged through torch."""
    from elemental_amd import _lib as L
    if device == 0:
        L.call(name, *make_args([o.buf.ctypes.data + o.elem_offset * o.buf.itemsize for o in ops]))
        return
    import torch
    ts = [torch.from_numpy(o.buf.view(np.uint8).copy()).cuda() for o in ops]
    L.call(name, *make_args([t.data_ptr() + o.elem_offset * o.buf.itemsize for t, o in zip(ts, ops)]))
    L.call("elx_device_synchronize")
    for t, o in zip(ts, ops):
        o.buf[...] = t.cpu().numpy().view(o.buf.dtype)


def matrix_gemv(device, dtype, trans, alpha, A, x, beta, y):
    from elemental_amd import el
    m, n = A.shape
    run(device, "elx_matrix_gemv", [A, x, y],
        lambda p: (dtype, device, el.TRANSPOSE if trans else el.NORMAL, m, n, float(alpha), p[0], A.ld, p[1], x.inc,
                   float(beta), p[2], y.inc, None))


def matrix_symv(device, dtype, lower, alpha, A, x, beta, y):
    from elemental_amd import el
    run(device, "elx_matrix_symv", [A, x, y],
        lambda p: (dtype, device, el.LOWER if lower else el.UPPER, A.shape[0], float(alpha), p[0], A.ld, p[1], x.inc,
                   float(beta), p[2], y.inc, None))


def matrix_symv_accumulate(device, dtype, lower, alpha, A, xr, xc, zr, zc, imap):
    from elemental_amd import el
    m, n = A.shape
    run(device, "elx_matrix_symv_accumulate", [A, xr, xc, zr, zc],
        lambda p: (dtype, device, el.LOWER if lower else el.UPPER, m, n, float(alpha), p[0], A.ld, p[1], xr.inc, p[2],
                   xc.inc, p[3], zr.inc, p[4], zc.inc, imap[0], imap[1], imap[2], imap[3], None))


def matrix_update(device, dtype, terms, lower, alpha, x, y, A):
    from elemental_amd import el
    m, n = A.shape
    uplo = el.LOWER if lower else el.UPPER
    if terms == 0:
        run(device, "elx_matrix_ger", [x, y, A],
            lambda p: (dtype, device, m, n, float(alpha), p[0], x.inc, p[1], y.inc, p[2], A.ld, None))
    elif terms == 1:
        run(device, "elx_matrix_syr", [x, A], lambda p: (dtype, device, uplo, n, float(alpha), p[0], x.inc, p[1], A.ld,
                                                        None))
    else:
        run(device, "elx_matrix_syr2", [x, y, A],
            lambda p: (dtype, device, uplo, n, float(alpha), p[0], x.inc, p[1], y.inc, p[2], A.ld, None))


# ---- the local checks, shared by the CPU (host loops) and the GPU (kernels) tests ----------
def check_gemv(device, dtype, trans, m, n, pad, incx, incy, seed, exact=False):
    fmt = FMT[dtype]
    k, ylen = (m, n) if trans else (n, m)
    gen = (lambda a, b, s: ints(a, b, s)) if exact else (lambda a, b, s: rand(fmt, a, b, s))
    A0, x0, y0 = gen(m, n, seed), gen(k, 1, seed + 1)[:, 0], gen(ylen, 1, seed + 2)[:, 0]
    for (alpha, beta) in (EXACT_SCALARS if exact else [(0.75, -0.5)]):
        A = Operand(fmt, A0, ld=m + 3 if pad else None, off=1 if pad else 0)
        x, y = Operand(fmt, x0, inc=incx, off=1 if pad else 0), Operand(fmt, y0, inc=incy, off=1 if pad else 0)
        if beta == 0:
            y.set_nan()
        matrix_gemv(device, dtype, trans, alpha, A, x, beta, y)
        tag = f"gemv {fmt} {'T' if trans else 'N'} {m}x{n} pad={pad} inc=({incx},{incy}) alpha={alpha} beta={beta}"
        assert A.unchanged() and x.unchanged(), tag + ": an input changed"
        assert y.untouched_outside(np.ones(ylen, bool)), tag + ": written outside y"
        got = y.values()
        ref, S = gemv_ref(trans, alpha, A0, x0, beta, y0)
        if exact:
            assert np.array_equal(_bits(store(fmt, got)), _bits(store(fmt, ref))), tag + ": exact case differs"
        else:
            err, bound = np.abs(got - ref), gemv_bound(fmt, k, S, ref)
            assert (err <= bound).all(), f"{tag}: err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}"
        # bit-identical rerun
        y2 = Operand(fmt, y0, inc=incy, off=1 if pad else 0)
        if beta == 0:
            y2.set_nan()
        matrix_gemv(device, dtype, trans, alpha, A, x, beta, y2)
        assert np.array_equal(_bits(y2.buf[y2.idx]), _bits(y.buf[y.idx])), tag + ": two runs differ"


def check_gemv_conventions(device, dtype):
    """alpha = 0 with NaN in A and x; a zero-length x; zero-size outputs."""
    fmt = FMT[dtype]
    for trans in (False, True):
        m, n = 37, 29
        ylen = n if trans else m
        y0 = rand(fmt, ylen, 1, 5)[:, 0]
        A, x = Operand(fmt, np.zeros((m, n))), Operand(fmt, np.zeros(m if trans else n))
        A.set_nan()
        x.set_nan()
        y = Operand(fmt, y0, inc=3)
        matrix_gemv(device, dtype, trans, 0.0, A, x, 0.5, y)
        assert np.array_equal(y.values(), load(fmt, store(fmt, 0.5 * y0))), "alpha = 0 must not read A or x"
        assert y.untouched_outside(np.ones(ylen, bool))
        y = Operand(fmt, y0)
        y.set_nan()
        matrix_gemv(device, dtype, trans, 0.0, A, x, 0.0, y)
        assert (y.values() == 0).all(), "alpha = 0, beta = 0 over a NaN y"
        # a zero-length x: y := beta y
        mz, nz = (0, ylen) if trans else (ylen, 0)
        Az, xz, y = Operand(fmt, np.zeros((mz, nz)), ld=max(mz, 1)), Operand(fmt, np.zeros(0)), Operand(fmt, y0)
        matrix_gemv(device, dtype, trans, 2.0, Az, xz, -1.0, y)
        assert np.array_equal(y.values(), -y0), "zero-length x must give beta y"
        # zero-size output: nothing happens
        mz, nz = (5, 0) if trans else (0, 5)
        Az, xz, yz = Operand(fmt, np.zeros((mz, nz)), ld=max(mz, 1)), Operand(fmt, np.ones(5)), Operand(fmt, np.zeros(0))
        matrix_gemv(device, dtype, trans, 1.0, Az, xz, 1.0, yz)
        assert yz.unchanged()


def check_symv(device, dtype, lower, n, pad, seed, exact=False):
    fmt = FMT[dtype]
    gen = (lambda a, b, s: ints(a, b, s)) if exact else (lambda a, b, s: rand(fmt, a, b, s))
    A0, x0, y0 = gen(n, n, seed), gen(n, 1, seed + 1)[:, 0], gen(n, 1, seed + 2)[:, 0]
    Asym = symmetrize(lower, A0)
    other = ~tri_mask(lower, n, n)
    for (alpha, beta) in (EXACT_SCALARS if exact else [(0.75, -0.5), (1.25, 0.0)]):
        A = Operand(fmt, A0, ld=n + 3 if pad else None, off=1 if pad else 0)
        A.set_nan(other)  # every element of the other strict triangle is NaN
        incx, incy = (3, 1) if pad else (1, 3)
        x, y = Operand(fmt, x0, inc=incx, off=1 if pad else 0), Operand(fmt, y0, inc=incy)
        if beta == 0:
            y.set_nan()
        matrix_symv(device, dtype, lower, alpha, A, x, beta, y)
        tag = f"symv {fmt} {'L' if lower else 'U'} n={n} pad={pad} alpha={alpha} beta={beta}"
        assert A.unchanged() and x.unchanged(), tag + ": an input changed"
        assert y.untouched_outside(np.ones(n, bool)), tag + ": written outside y"
        got = y.values()
        ref, S = gemv_ref(False, alpha, Asym, x0, beta, y0)
        assert not np.isnan(got).any(), tag + ": the other triangle was read"
        if exact:
            assert np.array_equal(_bits(store(fmt, got)), _bits(store(fmt, ref))), tag + ": exact case differs"
        else:
            err, bound = np.abs(got - ref), gemv_bound(fmt, n, S, ref)
            assert (err <= bound).all(), f"{tag}: err/bound {np.max(err / np.maximum(bound, 1e-300)):.3g}"
            # the same product through Gemv on the symmetrized matrix, within the bound
            yg = Operand(fmt, y0)
            matrix_gemv(device, dtype, False, alpha, Operand(fmt, Asym), Operand(fmt, x0), beta, yg)
            # both results lie within `bound` of the same float64 reference, so they lie
            # within twice it of each other: that, not 1 x bound, is what the bound implies
            assert (np.abs(got - yg.values()) <= 2 * bound).all(), tag + ": differs from Gemv"
        y2 = Operand(fmt, y0, inc=incy)
        if beta == 0:
            y2.set_nan()
        matrix_symv(device, dtype, lower, alpha, A, x, beta, y2)
        assert np.array_equal(_bits(y2.buf[y2.idx]), _bits(y.buf[y.idx])), tag + ": two runs differ"


def check_symv_accumulate(device, dtype, lower, m, n, imap, seed):
    fmt = FMT[dtype]
    A0, xr0, xc0 = rand(fmt, m, n, seed), rand(fmt, m, 1, seed + 1)[:, 0], rand(fmt, n, 1, seed + 2)[:, 0]
    zr0, zc0 = rand(fmt, m, 1, seed + 3)[:, 0], rand(fmt, n, 1, seed + 4)[:, 0]
    A = Operand(fmt, A0, ld=m + 3, off=1)
    A.set_nan(~tri_mask(lower, m, n, *imap))
    xr, xc, zr, zc = Operand(fmt, xr0), Operand(fmt, xc0, inc=3), Operand(fmt, zr0, inc=3), Operand(fmt, zc0)
    matrix_symv_accumulate(device, dtype, lower, 0.75, A, xr, xc, zr, zc, imap)
    rr, rc, Sr, Sc = symv_accumulate_ref(lower, 0.75, A0, xr0, xc0, imap)
    tag = f"symv_accumulate {fmt} {'L' if lower else 'U'} {m}x{n} map={imap}"
    assert A.unchanged() and zr.untouched_outside(np.ones(m, bool)) and zc.untouched_outside(np.ones(n, bool)), tag
    for got, ref, S, z0, k in ((zr.values(), rr, Sr, zr0, n), (zc.values(), rc, Sc, zc0, m)):
        assert not np.isnan(got).any(), tag + ": an element across the diagonal was read"
        bound = gemv_bound(fmt, k, S + np.abs(z0), ref + z0)
        assert (np.abs(got - (ref + z0)) <= bound).all(), tag


def check_update(device, dtype, terms, lower, m, n, pad, rows, seed, exact=False):
    """Ger (terms 0), Syr (1), Syr2 (2); rows: the vectors are rows of a matrix (stride 3)."""
    fmt = FMT[dtype]
    gen = (lambda a, b, s: ints(a, b, s)) if exact else (lambda a, b, s: rand(fmt, a, b, s))
    A0, x0 = gen(m, n, seed), gen(m, 1, seed + 1)[:, 0]
    y0 = gen(n, 1, seed + 2)[:, 0] if terms != 1 else x0
    for alpha in ([1, -1, 2] if exact else [0.75]):
        Aref, base, mask = update_ref(terms, lower, alpha, x0, y0, A0)
        A = Operand(fmt, A0, ld=m + 3 if pad else None, off=1 if pad else 0)
        if terms != 0:
            A.set_nan(~mask)  # the other triangle is neither read nor written
        inc = 3 if rows else 1
        x, y = Operand(fmt, x0, inc=inc, off=1 if pad else 0), Operand(fmt, y0, inc=inc)
        matrix_update(device, dtype, terms, lower, alpha, x, y, A)
        tag = f"{('ger', 'syr', 'syr2')[terms]} {fmt} {'L' if lower else 'U'} {m}x{n} pad={pad} rows={rows} alpha={alpha}"
        assert x.unchanged() and y.unchanged(), tag + ": an input changed"
        assert A.untouched_outside(mask), tag + ": the other triangle or the padding changed"
        got = A.values()[mask]
        assert not np.isnan(got).any(), tag + ": the other triangle was read"
        if exact:
            assert np.array_equal(got, Aref[mask]), tag + ": exact case differs"
        else:
            assert (np.abs(got - Aref[mask]) <= 4 * eps_acc(fmt) * base[mask]).all(), tag
    # alpha = 0 reads and writes nothing
    A = Operand(fmt, A0)
    x = Operand(fmt, x0)
    x.set_nan()
    matrix_update(device, dtype, terms, lower, 0.0, x, x if terms == 1 else Operand(fmt, y0), A)
    assert A.unchanged()


# ---- distributed -----------------------------------------------------------------------------
def full_matrix(el, D):
    S = D.like(el.STAR, el.STAR)
    S.assign(D)
    return S.get_local()


def dist_of(el, g, dtype, device, G, U=None, V=None, ca=0, ra=0):
    """the global array G as a [U,V] DistMatrix with the given alignments."""
    import oracle
    U = el.MC if U is None else U
    V = el.MR if V is None else V
    D = el.DistMatrix(g, dtype, U, V, device)
    D.Align(ca % oracle.lib().orc_dist_stride(U, g.height, g.width),
            ra % oracle.lib().orc_dist_stride(V, g.height, g.width))
    D.Resize(G.shape[0], G.shape[1])
    i = D.info()
    D.set_local(oracle.local_block(np.asfortranarray(G), U, V, g.height, g.width, g.vc_rank, i["col_align"],
                                   i["row_align"]))
    return D


def vector_forms(el):
    """(name, row vector?, U, V): [MC,MR] column, [MC,MR] row, [VC,*] column."""
    return [("col[MC,MR]", False, el.MC, el.MR), ("row[MC,MR]", True, el.MC, el.MR), ("col[VC,*]", False, el.VC, el.STAR)]


def level2_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, sizes, seed: int):
    """Every routine on a height x (world / height) grid: Gemv and Ger at each (m, n) of
    `sizes`, Symv, Syr and Syr2 at n = m; x and y as [MC,MR] columns, [MC,MR] rows and
    [VC,*] columns; A with non-zero alignments; each result gathered and compared with
    numpy within the bounds (k the global length), the integer cases bit for bit, and
    LocalColAccumulate against its numpy restatement on every rank."""
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        fmt = FMT[dtype]
        npdt = STORE[fmt]
        real = fmt in ("f64", "f32")

        def mk(G, U=None, V=None, ca=0, ra=0):
            return dist_of(el, g, dtype, device, np.asarray(store(fmt, G)), U, V, ca, ra)

        def vec(v, form, ca=0):
            _, row, U, V = form
            return mk(v[None, :] if row else v[:, None], U, V, ca, ca)

        def back(D, row):
            out = load(fmt, full_matrix(el, D))
            return out[0, :] if row else out[:, 0]

        forms = vector_forms(el)
        for (m, n) in sizes:
            for exact in (False, True):
                gen = (lambda a, b, s: ints(a, b, s)) if exact else (lambda a, b, s: rand(fmt, a, b, s))
                A0 = gen(m, n, seed + m)
                alpha, beta = (2, -1) if exact else (0.75, -0.5)
                for fi, xform in enumerate(forms):
                    yform = forms[(fi + 1) % 3]
                    for trans in (False, True):
                        k, ylen = (m, n) if trans else (n, m)
                        x0, y0 = gen(k, 1, seed + 1)[:, 0], gen(ylen, 1, seed + 2)[:, 0]
                        A, x, y = mk(A0, ca=1, ra=1), vec(x0, xform, 1), vec(y0, yform)
                        el.Gemv(el.TRANSPOSE if trans else el.NORMAL, alpha, A, x, beta, y)
                        got = back(y, yform[1])
                        ref, S = gemv_ref(trans, alpha, A0, x0, beta, y0)
                        tag = f"Gemv {fmt} {'T' if trans else 'N'} {m}x{n} x {xform[0]} y {yform[0]} exact={exact}"
                        if exact:
                            assert np.array_equal(_bits(store(fmt, got)), _bits(store(fmt, ref))), tag
                        else:
                            assert (np.abs(got - ref) <= gemv_bound(fmt, k, S, ref)).all(), tag
                    if not real:
                        continue
                    x0, y0 = gen(m, 1, seed + 3)[:, 0], gen(n, 1, seed + 4)[:, 0]
                    A = mk(A0, ca=1, ra=1)
                    el.Ger(alpha, vec(x0, xform, 1), vec(y0, yform), A)
                    Aref, base, _ = update_ref(0, True, alpha, x0, y0, A0)
                    got = load(fmt, full_matrix(el, A))
                    tag = f"Ger {fmt} {m}x{n} x {xform[0]} y {yform[0]} exact={exact}"
                    assert np.array_equal(got, Aref) if exact else (np.abs(got - Aref) <= 4 * eps_acc(fmt) * base).all(), tag
                    # the triangle routines at n = m
                    S0 = gen(m, m, seed + 5)
                    y1 = gen(m, 1, seed + 6)[:, 0]
                    for lower in (True, False):
                        uplo = el.LOWER if lower else el.UPPER
                        mask = tri_mask(lower, m, m)
                        Asym = symmetrize(lower, S0)
                        poisoned = np.where(mask, S0, np.nan)
                        A = dist_of(el, g, dtype, device, np.where(mask, store(fmt, S0), nan_of(fmt)).astype(npdt),
                                    ca=1, ra=1)
                        y = vec(y1, yform)
                        el.Symv(uplo, alpha, A, vec(x0, xform, 1), beta, y)
                        got = back(y, yform[1])
                        ref, S = gemv_ref(False, alpha, Asym, x0, beta, y1)
                        tag = f"Symv {fmt} {'L' if lower else 'U'} n={m} x {xform[0]} y {yform[0]} exact={exact}"
                        assert not np.isnan(got).any(), tag + ": the other triangle was read"
                        if exact:
                            assert np.array_equal(got, ref), tag
                        else:
                            assert (np.abs(got - ref) <= gemv_bound(fmt, m, S, ref)).all(), tag
                        for terms in (1, 2):
                            yv = x0 if terms == 1 else y1
                            A = dist_of(el, g, dtype, device,
                                        np.where(mask, store(fmt, S0), nan_of(fmt)).astype(npdt), ca=1, ra=1)
                            if terms == 1:
                                el.Syr(uplo, alpha, vec(x0, xform, 1), A)
                            else:
                                el.Syr2(uplo, alpha, vec(x0, xform, 1), vec(y1, yform), A)
                            Aref, base, _ = update_ref(terms, lower, alpha, x0, yv, S0)
                            gotA = full_matrix(el, A)
                            tag = f"Syr{'' if terms == 1 else '2'} {fmt} {'L' if lower else 'U'} n={m} exact={exact}"
                            want_nan = np.where(mask, store(fmt, S0), nan_of(fmt)).astype(npdt)
                            assert np.array_equal(_bits(gotA[~mask]), _bits(want_nan[~mask])), tag + ": other triangle"
                            gv = load(fmt, gotA)[mask]
                            if exact:
                                assert np.array_equal(gv, Aref[mask]), tag
                            else:
                                assert (np.abs(gv - Aref[mask]) <= 4 * eps_acc(fmt) * base[mask]).all(), tag
                        del poisoned
            if real and m == n or real and (m, n) == sizes[0]:
                # LocalColAccumulate against its restatement on this rank's block
                nn = m
                S0, x0 = rand(fmt, nn, nn, seed + 7), rand(fmt, nn, 1, seed + 8)[:, 0]
                for lower in (True, False):
                    A = mk(S0, ca=1, ra=1)
                    x_mc, x_mr = mk(x0[:, None], el.MC, el.STAR, 1, 0), mk(x0[:, None], el.MR, el.STAR, 1, 0)
                    z_mc, z_mr = mk(np.zeros((nn, 1)), el.MC, el.STAR, 1, 0), mk(np.zeros((nn, 1)), el.MR, el.STAR, 1, 0)
                    el.SymvLocalColAccumulate(el.LOWER if lower else el.UPPER, 0.75, A, x_mc, x_mr, z_mc, z_mr)
                    i = A.info()
                    imap = (i["col_shift"], i["col_stride"], i["row_shift"], i["row_stride"])
                    Al = load(fmt, A.get_local())
                    xr, xc = load(fmt, x_mc.get_local())[:, 0], load(fmt, x_mr.get_local())[:, 0]
                    rr, rc, Sr, Sc = symv_accumulate_ref(lower, 0.75, Al, xr, xc, imap)
                    gr, gc = load(fmt, z_mc.get_local())[:, 0], load(fmt, z_mr.get_local())[:, 0]
                    assert (np.abs(gr - rr) <= gemv_bound(fmt, nn, Sr, rr)).all(), "LocalColAccumulate z[MC,*]"
                    assert (np.abs(gc - rc) <= gemv_bound(fmt, nn, Sc, rc)).all(), "LocalColAccumulate z[MR,*]"
        finish()
    except Exception:
        traceback.print_exc()
        raise


def gemv16_bound(fmt, k, world, S):
    """The distributed Gemv keeps z in the storage type, as the reference does, so it
    rounds to 16 bits once per stage instead of once: each rank's local z (P <= world
    ranks contribute, their magnitudes sum to at most S), each of the P adds of the
    contraction (every partial sum is at most S), beta y, the transposed copy's add for a
    row vector, and the final add.  That is at most P + 4 roundings of values bounded by
    S, each of half a storage epsilon relative; with the same factor of two as the local
    bound, (world + 4) eps_storage S, plus the f32 accumulation term of the local bound
    and one smallest subnormal per rounding."""
    return (world + 4) * EPS_STORE[fmt] * S + 2 * (k + 3) * eps_acc(fmt) * S + (world + 4) * TINY[fmt]


def gemv16_worker(rank: int, world: int, port: int, height: int, device: int, dtype: int, m: int, n: int, seed: int):
    """El::Gemv on f16 / bf16 DistMatrices: both orientations, x and y as [MC,MR] columns,
    [MC,MR] rows and [VC,*] columns, A with non-zero alignments, against float64 numpy
    within gemv16_bound."""
    el, comm = init(rank, world, port)
    try:
        g = el.Grid(comm, height)
        fmt = FMT[dtype]

        def mk(G, U=None, V=None, ca=0, ra=0):
            return dist_of(el, g, dtype, device, np.asarray(store(fmt, G)), U, V, ca, ra)

        forms = vector_forms(el)
        A0 = rand(fmt, m, n, seed)
        for fi, xform in enumerate(forms):
            yform = forms[(fi + 1) % 3]
            for trans in (False, True):
                k, ylen = (m, n) if trans else (n, m)
                x0, y0 = rand(fmt, k, 1, seed + 1)[:, 0], rand(fmt, ylen, 1, seed + 2)[:, 0]
                x = mk(x0[None, :] if xform[1] else x0[:, None], xform[2], xform[3], 1, 1)
                y = mk(y0[None, :] if yform[1] else y0[:, None], yform[2], yform[3])
                el.Gemv(el.TRANSPOSE if trans else el.NORMAL, 0.75, mk(A0, ca=1, ra=1), x, -0.5, y)
                out = load(fmt, full_matrix(el, y))
                got = out[0, :] if yform[1] else out[:, 0]
                ref, S = gemv_ref(trans, 0.75, A0, x0, -0.5, y0)
                err, bound = np.abs(got - ref), gemv16_bound(fmt, k, world, S)
                assert (err <= bound).all(), (f"Gemv {fmt} {'T' if trans else 'N'} x {xform[0]} y {yform[0]}: "
                                              f"err/bound {np.max(err / bound):.3g}")
        finish()
    except Exception:
        traceback.print_exc()
        raise
