"""The host loops behind Device::CPU, bit for bit, in all four element types.

Every operation runs through el.py on a 1x1 grid, on matrices attached to numpy buffers
whose leading dimension exceeds the height; the padding rows hold a sentinel that must
survive.  The expected values follow the documented rule: compute in float32 (float64
for F64), round once to nearest-even into the storage type.  They are compared as bit
patterns, except that a NaN only has to be a NaN (the one test on NaN bits says which
pattern an f16 store writes).  exp, log, sigmoid and tanh depend on the machine's libm
and are held to one unit in the last place of the storage type.

The inputs hold +-0, +-Inf, a NaN, the largest finite value of the type, an f16
subnormal, and values whose product with 1.5 lies exactly halfway between two 16-bit
neighbours (1 + 2^-10 for f16, 1 + 2^-7 for bf16), so a rounding that is not
ties-to-even shows."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from elemental_amd import _lib as L
from elemental_amd import el

F64, F32, F16, BF16 = el.F64, el.F32, el.F16, el.BF16
TYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32"), pytest.param(F16, id="f16"),
         pytest.param(BF16, id="bf16")]
SHAPES = [pytest.param((5, 3), id="5x3"), pytest.param((1, 1), id="1x1")]
COMPUTE = {F64: np.float64, F32: np.float32, F16: np.float32, BF16: np.float32}
UINT = {F64: np.uint64, F32: np.uint32, F16: np.uint16, BF16: np.uint16}
MAXF = {F64: float(np.finfo(np.float64).max), F32: float(np.finfo(np.float32).max), F16: 65504.0,
        BF16: float.fromhex("0x1.fep127")}
PAD = 3  # rows of padding below every matrix
INF, NAN = math.inf, math.nan
SUB16 = 3 * 2.0 ** -24  # an f16 subnormal
TIE16, TIEB16 = 1 + 2.0 ** -10, 1 + 2.0 ** -7  # times 1.5: halfway between two f16 / bf16 values


@pytest.fixture(autouse=True)
def _quiet_numpy():
    with np.errstate(all="ignore"):
        yield


@functools.lru_cache(maxsize=None)
def grid():
    return el.Grid()


# ---- the number formats: compute-type arrays <-> storage bit patterns
def bf16_round(f32):
    """float32 -> bf16 bits, to nearest-even."""
    u = np.asarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f32), np.uint16(0x7fc0), r)


def enc(t, c):
    """A compute-type array rounded once into the storage type, as bit patterns."""
    c = np.asarray(c, COMPUTE[t])
    if t == BF16:
        return bf16_round(c)
    if t == F16:
        return c.astype(np.float16).view(np.uint16)
    return c.view(UINT[t])


def dec(t, bits):
    """Storage bit patterns as a compute-type array (exact)."""
    bits = np.asarray(bits, UINT[t])
    if t == BF16:
        return (bits.astype(np.uint32) << 16).view(np.float32)
    if t == F16:
        return bits.view(np.float16).astype(np.float32)
    return bits.view(COMPUTE[t])


def is_nan(t, bits):
    return np.isnan(dec(t, bits))


def same(t, got, want):
    """Bit for bit, except that a NaN only has to be a NaN."""
    got, want = np.asarray(got, UINT[t]), np.asarray(want, UINT[t])
    gn, wn = is_nan(t, got), is_nan(t, want)
    assert np.array_equal(gn, wn), (dec(t, got), dec(t, want))
    assert np.array_equal(got[~wn], want[~wn]), (dec(t, got), dec(t, want))


def ordered(t, bits):
    """Bit patterns as integers in the order of the values (for distances in ulps)."""
    bits = np.asarray(bits, UINT[t])
    top = np.uint64(1) << np.uint64(8 * bits.itemsize - 1)
    b = bits.astype(np.uint64)
    mag = (b & (top - np.uint64(1))).astype(np.int64)
    return np.where((b & top) != 0, -mag, mag)


def within_one_ulp(t, got, want):
    got, want = np.asarray(got, UINT[t]), np.asarray(want, UINT[t])
    gn, wn = is_nan(t, got), is_nan(t, want)
    assert np.array_equal(gn, wn), (dec(t, got), dec(t, want))
    d = np.abs(ordered(t, got)[~wn] - ordered(t, want)[~wn])
    assert d.max(initial=0) <= 1, (dec(t, got), dec(t, want))


# ---- inputs
def values_a(t):
    return [0.0, -0.0, INF, -INF, NAN, MAXF[t], -MAXF[t], SUB16, TIE16, TIEB16, 0.1, -2.5, 3.0, 1e-3, -7.0]


def values_b(t):
    return [2.0, INF, 0.0, INF, 1.0, 2.0, MAXF[t], -0.0, 1.5, 1.5, -0.1, 0.5, NAN, 1e3, SUB16]


def arrange(t, vals, shape):
    """The 15 values as a 5x3 matrix of type t; 1x1: the entry that makes the type's tie."""
    m = enc(t, np.array(vals, np.float64).astype(COMPUTE[t])).reshape((5, 3), order="F")
    if shape == (1, 1):
        i = 9 if t == BF16 else 8
        return m[i % 5:i % 5 + 1, i // 5:i // 5 + 1].copy()
    return m


FINITE = [0.1, -2.5, 3.0, 1e-3, -7.0, TIE16, TIEB16, 0.0, SUB16, 1.5, -0.75, 2.0, 0.3, -1.1, 5.0, 0.7, -0.2, 11.0, 0.05,
          -3.5]


def finite(t, h, w, start):
    """An h x w matrix of type t of ordinary values."""
    v = [FINITE[(start + q) % len(FINITE)] for q in range(h * w)]
    return enc(t, np.array(v, np.float64).astype(COMPUTE[t])).reshape((h, w), order="F")


class Host:
    """An h x w matrix [U,V] on Device::CPU, attached to a numpy buffer of leading
    dimension h + PAD whose padding rows hold a sentinel."""

    def __init__(self, t, bits=None, shape=None, U=el.MC, V=el.MR):
        self.t = t
        self.h, self.w = shape if bits is None else bits.shape
        self.sentinel = np.frombuffer(b"\x5a" * np.dtype(UINT[t]).itemsize, UINT[t])[0]
        self.buf = np.full((self.h + PAD, self.w), self.sentinel, dtype=UINT[t], order="F")
        if bits is not None:
            self.buf[:self.h] = bits
        self.dm = el.DistMatrix(grid(), t, U, V, el.CPU).attach(self.h, self.w, 0, 0, self.buf.ctypes.data,
                                                                self.h + PAD)

    def bits(self):
        assert (self.buf[self.h:] == self.sentinel).all(), "the padding below the matrix was written"
        assert self.dm.LDim() == self.h + PAD
        return self.buf[:self.h].copy()


# ---- elementwise
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_fill(t, shape):
    # 1 + 2^-11 and 1 + 2^-8 are ties for f16 and bf16, 65520 is the tie between the largest f16 and 2^16,
    # 1e39 overflows float32, 1e-8 underflows f16
    for v in [0.1, 1 + 2.0 ** -11, 1 + 2.0 ** -8, -0.0, INF, -INF, NAN, 1e39, SUB16, 65520.0, 1e-8, MAXF[t]]:
        A = Host(t, arrange(t, values_a(t), shape))
        el.Fill(A.dm, v)
        same(t, A.bits(), enc(t, np.full(shape, np.float64(v)).astype(COMPUTE[t])))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_scale(t, shape):
    x = arrange(t, values_a(t), shape)
    for alpha in [0.0, 1.0, 1.5, -2.0, 2.0 ** -14, 1e30]:
        A = Host(t, x)
        el.Scale(alpha, A.dm)
        if alpha == 0.0:  # El::Scale: zero, whatever was there
            assert (A.bits() == 0).all()
        elif alpha == 1.0:  # untouched, a NaN's payload included
            assert np.array_equal(A.bits(), x)
        else:
            same(t, A.bits(), enc(t, COMPUTE[t](alpha) * dec(t, x)))


def test_scale_f16_stores_the_canonical_nan():
    """The host f16 store writes sign | 0x7e00 for every NaN, whatever payload came in."""
    x = np.array([[0x7c01, 0xfe55, 0x7e00], [0x7dff, 0xfc01, 0x3c00]], np.uint16)
    A = Host(F16, x)
    el.Scale(1.5, A.dm)
    got = A.bits()
    assert set(got[is_nan(F16, x)].tolist()) <= {0x7e00, 0xfe00}, [hex(v) for v in got.ravel()]
    assert got[1, 2] == 0x3e00  # 1.5


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_axpy(t, shape):
    x, y = arrange(t, values_a(t), shape), arrange(t, values_b(t), shape)
    for alpha in [1.5, -1.0, 0.0, 2.0 ** -12]:
        X, Y = Host(t, x), Host(t, y)
        el.Axpy(alpha, X.dm, Y.dm)
        same(t, Y.bits(), enc(t, dec(t, y) + COMPUTE[t](alpha) * dec(t, x)))
        assert np.array_equal(X.bits(), x)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_hadamard(t, shape):
    a, b = arrange(t, values_a(t), shape), arrange(t, values_b(t), shape)
    A, B, C = Host(t, a), Host(t, b), Host(t, shape=shape)
    el.Hadamard(A.dm, B.dm, C.dm)
    same(t, C.bits(), enc(t, dec(t, a) * dec(t, b)))
    assert np.array_equal(A.bits(), a) and np.array_equal(B.bits(), b)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_scale_trapezoid(t, shape):
    x = arrange(t, values_a(t), shape)
    i, j = np.indices(shape)
    for uplo in (el.LOWER, el.UPPER):
        for offset in (-1, 0, 1):
            for alpha in (1.5, 0.0, 1.0):
                A = Host(t, x)
                el.ScaleTrapezoid(alpha, uplo, A.dm, offset)
                inside = (j - i <= offset) if uplo == el.LOWER else (j - i >= offset)
                if alpha == 1.0:
                    inside = np.zeros(shape, bool)
                got = A.bits()
                assert np.array_equal(got[~inside], x[~inside])  # outside: untouched bits
                same(t, got[inside], enc(t, COMPUTE[t](alpha) * dec(t, x))[inside])


EXACT_MAPS = {
    L.MAP_IDENTITY: lambda x: x,
    L.MAP_NEGATE: lambda x: -x,
    L.MAP_ABS: np.abs,
    L.MAP_SQUARE: lambda x: x * x,
    L.MAP_SQRT: np.sqrt,
    L.MAP_RELU: lambda x: np.where(x > 0, x, x.dtype.type(0)),
    L.MAP_RECIP: lambda x: x.dtype.type(1) / x,
}
def libm(f, x):
    """numpy's f in float64, rounded to the compute type: numpy's own float32 exp and log
    are several ulps off, the machine's libm is held to less than one."""
    return f(x.astype(np.float64)).astype(x.dtype)


LIBM_MAPS = {
    L.MAP_EXP: lambda x: libm(np.exp, x),
    L.MAP_LOG: lambda x: libm(np.log, x),
    L.MAP_SIGMOID: lambda x: x.dtype.type(1) / (x.dtype.type(1) + libm(np.exp, -x)),
    L.MAP_TANH: lambda x: libm(np.tanh, x),
}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_entrywise_map_exact(t, shape):
    for vals in (values_a(t), values_b(t)):
        a = arrange(t, vals, shape)
        for fn, f in EXACT_MAPS.items():
            A, B = Host(t, a), Host(t, shape=shape)
            el.EntrywiseMap(fn, A.dm, B.dm)
            same(t, B.bits(), enc(t, f(dec(t, a))))
            assert np.array_equal(A.bits(), a)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_entrywise_map_libm(t, shape):
    for vals in (values_a(t), values_b(t)):
        a = arrange(t, vals, shape)
        for fn, f in LIBM_MAPS.items():
            A, B = Host(t, a), Host(t, shape=shape)
            el.EntrywiseMap(fn, A.dm, B.dm)
            within_one_ulp(t, B.bits(), enc(t, f(dec(t, a))))


COMBINES = {  # B := f(A, B)
    L.COMBINE_ADD: lambda a, b: a + b,
    L.COMBINE_SUB: lambda a, b: b - a,
    L.COMBINE_MUL: lambda a, b: a * b,
    L.COMBINE_DIV: lambda a, b: b / a,
    L.COMBINE_MAX: lambda a, b: np.where(a > b, a, b),
    L.COMBINE_MIN: lambda a, b: np.where(a < b, a, b),
    L.COMBINE_RELU_GRAD: lambda a, b: np.where(a > 0, b, b.dtype.type(0)),
}


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_combine(t, shape):
    assert len(COMBINES) == 7
    for va, vb in ((values_a(t), values_b(t)), (values_b(t), values_a(t))):
        a, b = arrange(t, va, shape), arrange(t, vb, shape)
        for fn, f in COMBINES.items():
            A, B = Host(t, a), Host(t, b)
            el.Combine(fn, A.dm, B.dm)
            same(t, B.bits(), enc(t, f(dec(t, a), dec(t, b))))
            assert np.array_equal(A.bits(), a)


# ---- FrobeniusNorm: max |a| (a NaN wins), then the scaled sum of squares in double, column by column
def ref_frobenius(x):
    vals = [float(v) for v in x.flatten(order="F")]
    amax = 0.0
    for v in vals:
        amax = amax if amax != amax else abs(v) if v != v else max(amax, abs(v))
    if amax == 0.0 or not math.isfinite(amax):
        return amax
    s = 0.0
    for v in vals:
        s += (v / amax) * (v / amax)
    return amax * math.sqrt(s)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_frobenius_norm(t, shape):
    va = values_a(t)
    no_nan = [1.0 if v != v else v for v in va]
    for bits in (arrange(t, va, shape), arrange(t, no_nan, shape), finite(t, *shape, 0), finite(t, *shape, 7),
                 np.zeros(shape, UINT[t])):
        A = Host(t, bits)
        got, want = el.FrobeniusNorm(A.dm), ref_frobenius(dec(t, bits))
        assert (got != got and want != want) or got == want, (got, want)
        assert np.array_equal(A.bits(), bits)


# ---- local Gemm: per column of C the sum over l in order, a zero B(l,j) skips its term
# (so it hides an Inf or NaN in A), then alpha * sum, plus beta * C unless beta is zero
def ref_gemm(t, ta, alpha, a, b, beta, c):
    Cm = COMPUTE[t]
    A, B, C = dec(t, a), dec(t, b), dec(t, c)
    opA = A.T if ta else A
    m, k = opA.shape
    out = np.empty(C.shape, Cm)
    for j in range(C.shape[1]):
        acc = np.zeros(m, Cm)
        for l in range(k):
            if B[l, j] == 0:
                continue
            acc = acc + opA[:, l] * B[l, j]
        v = Cm(alpha) * acc
        out[:, j] = v if beta == 0.0 else v + Cm(beta) * C[:, j]
    return enc(t, out)


@pytest.mark.parametrize("mnk", [pytest.param((5, 3, 4), id="5x3x4"), pytest.param((1, 1, 1), id="1x1x1")])
@pytest.mark.parametrize("t", TYPES)
def test_local_gemm(t, mnk):
    m, n, k = mnk
    for ta in (False, True):
        a = finite(t, *((k, m) if ta else (m, k)), 0)
        b = finite(t, k, n, 5)
        c = finite(t, m, n, 11)
        if k > 1:
            # an Inf in A's column 1 (of op(A)): hidden in column 0 of C by a zero in B, seen elsewhere
            a[(1, 2) if ta else (2, 1)] = enc(t, [INF])[0]
            b[1, 0] = 0
            c[0, 1] = enc(t, [NAN])[0]  # beta == 0 must not read it
        for alpha, beta in ((1.0, 0.0), (0.5, -2.0), (-1.5, 1.0)):
            A = Host(t, a, U=el.STAR if ta else el.MC, V=el.MC if ta else el.STAR)
            B, C = Host(t, b, U=el.STAR, V=el.MR), Host(t, c)
            el.LocalGemm(el.TRANSPOSE if ta else el.NORMAL, el.NORMAL, alpha, A.dm, B.dm, beta, C.dm)
            same(t, C.bits(), ref_gemm(t, ta, alpha, a, b, beta, c))
            assert np.array_equal(A.bits(), a) and np.array_equal(B.bits(), b)


# ---- local Gemv: the sum in order, then alpha * sum, plus beta * y unless beta is zero;
# alpha == 0 only scales y (beta == 0 writes zeros)
def ref_gemv(t, trans, alpha, a, x, beta, y):
    Cm = COMPUTE[t]
    A, X, Y = dec(t, a), dec(t, x)[:, 0], dec(t, y)[:, 0]
    if alpha == 0.0:
        out = Y if beta == 1.0 else np.zeros_like(Y) if beta == 0.0 else Cm(beta) * Y
        return enc(t, out.reshape(-1, 1))
    m, n = A.shape
    if trans:
        acc = np.zeros(n, Cm)
        for i in range(m):
            acc = acc + A[i, :] * X[i]
    else:
        acc = np.zeros(m, Cm)
        for j in range(n):
            acc = acc + A[:, j] * X[j]
    v = Cm(alpha) * acc
    return enc(t, (v if beta == 0.0 else v + Cm(beta) * Y).reshape(-1, 1))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("t", TYPES)
def test_local_gemv(t, shape):
    m, n = shape
    a = finite(t, m, n, 3)
    for trans in (False, True):
        xlen, ylen = (m, n) if trans else (n, m)
        x = finite(t, xlen, 1, 9)
        y = finite(t, ylen, 1, 14)
        y[0, 0] = enc(t, [NAN])[0]  # beta == 0 must not read it
        for alpha, beta in ((1.0, 0.0), (0.5, -2.0), (-1.5, 1.0), (0.0, 0.5), (0.0, 0.0)):
            A = Host(t, a)
            X = Host(t, x, U=el.MC if trans else el.MR, V=el.STAR)
            Y = Host(t, y, U=el.MR if trans else el.MC, V=el.STAR)
            el.LocalGemv(el.TRANSPOSE if trans else el.NORMAL, alpha, A.dm, X.dm, beta, Y.dm)
            same(t, Y.bits(), ref_gemv(t, trans, alpha, a, x, beta, y))
            assert np.array_equal(A.bits(), a) and np.array_equal(X.bits(), x)


# ---- Copy between element types (El::Copy reaches exec::Convert2D when the types differ):
# the exact source value rounded once, to nearest-even, into the target type
def bf16_from_f64(x):
    """float64 -> bf16 bits, the nearest by rational arithmetic, ties to the even pattern."""
    grid16 = dec(BF16, np.arange(0x7f80, dtype=np.uint16)).astype(np.float64)  # the finite values >= 0, ascending
    out = np.empty(x.shape, np.uint16)
    for idx, v in np.ndenumerate(x):
        v = float(v)
        sign, a = (0x8000 if math.copysign(1.0, v) < 0 else 0), abs(v)
        if a != a or a == INF:
            out[idx] = 0x7fc0 if a != a else sign | 0x7f80
            continue
        i = int(np.searchsorted(grid16, a, side="right")) - 1
        lo = Fraction(float(grid16[i]))
        hi = Fraction(float(grid16[i + 1])) if i + 1 < len(grid16) else Fraction(2) ** 128
        d = (Fraction(a) - lo) - (hi - Fraction(a))
        out[idx] = sign | (i + 1 if d > 0 or (d == 0 and i & 1) else i)
    return out


def ref_convert(ts, td, bits):
    exact = dec(ts, bits).astype(np.float64)
    if td == BF16:
        return bf16_from_f64(exact)
    if td == F16:
        return exact.astype(np.float16).view(np.uint16)
    return exact.astype(COMPUTE[td]).view(UINT[td])


def convert_values(t):
    # just above the f16 / bf16 ties of 1 (a rounding through float32 first would land on the tie),
    # the ties themselves, the overflow ties of f16 and bf16, subnormals of f16, bf16 and float32
    return [0.0, -0.0, INF, -INF, NAN, MAXF[t], -MAXF[t], 1 + 2.0 ** -11 + 2.0 ** -40, 1 + 2.0 ** -8 + 2.0 ** -40,
            1 + 2.0 ** -11, 1 + 2.0 ** -8, 65520.0, float.fromhex("0x1.ffp127"), SUB16, -(2.0 ** -134 + 2.0 ** -149)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("td", TYPES)
@pytest.mark.parametrize("ts", TYPES)
def test_copy_converts_with_one_rounding(ts, td, shape):
    for vals in (convert_values(ts), values_a(ts), [0.1 * (q - 7) for q in range(15)]):
        a = enc(ts, np.array(vals, np.float64).astype(COMPUTE[ts])).reshape((5, 3), order="F")
        if shape == (1, 1):
            a = a[2:3, 1:2].copy()  # entry 7
        A, B = Host(ts, a), Host(td, shape=shape)
        el.Copy(A.dm, B.dm)
        if ts == td:
            assert np.array_equal(B.bits(), a)  # a plain copy: every bit, a NaN's payload too
        else:
            same(td, B.bits(), ref_convert(ts, td, a))
        assert np.array_equal(A.bits(), a)


def test_bf16_rounding_restatements_agree():
    """The two bf16 roundings of this file (bit arithmetic from float32, rationals from
    float64) agree on every float32 they are both given."""
    rng = np.random.default_rng(5)
    u = rng.integers(0, 2 ** 32, 4000, dtype=np.uint64).astype(np.uint32)
    u = np.concatenate([u, np.array([0x3f808000, 0x3f818000, 0x7f7f8000, 0x7f7f7fff, 0x00008000, 0x00018000], np.uint32)])
    f = u.view(np.float32)
    f = f[~np.isnan(f)]
    assert np.array_equal(bf16_round(f), bf16_from_f64(f.astype(np.float64)))
