"""Inputs, oracle and runners shared by the Trsm tests (test_gpu_trsm, test_trsm_cpu).

The exact family: triangular systems whose solution, and every intermediate of
any correct algorithm (substitution in any order, block inverse plus GEMM, the
blocked sweep with GEMM updates), is a dyadic rational that float32 holds, so a
correct solve reproduces X bit for bit in f32 and f64.

  S    a random half of the indices
  Nt   strictly lower, integers in [-2, 2] at (r, c) only where c in S and r not
       in S, so Nt^2 = 0 and (I + Nt)^-1 = I - Nt
  Nf   a forest: row r >= 1 has one entry +-1 at column r - d, d from {1, 17, 64}
       (d <= r): (I - Nf)^-1 has entries in {0, +-1}, and the dependency chains
       run the full depth across the kernel's 8-row batch, the wave and 64 rows
  L    = (I + Nt)(I - Nf), unit lower, integer, with an integer inverse
  T    = L diag(2^e), e in {-1, 0, 1} (NON_UNIT); T = L (UNIT)

The stored A is T for LOWER and T^T for UPPER, so op(A) is T or T^T; B holds
integers in [-4, 4] and alpha = 2.  T's entries are multiples of 1/2, X is
integer, an inverse's entries are multiples of 1/2 and every product or partial
sum a multiple of 1/4: exact in float32 while it stays below 2^22, which
`bounds` asserts from the float64 reference alone before anything is launched.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np

from _trmm_workers import masked_triangle
from elemental_amd import _lib as L
from elemental_amd import el

ALPHA = 2.0
LIMIT = float(2 ** 22)
NPDT = {el.F64: np.float64, el.F32: np.float32}

# (m, n) -> the path of the f64 solve, the path of the f32 solve ("invert" /
# "subst", "LDS" / "global"): what kernels.hpp trsm_plan must name for the case
PATHS = {
    (1, 1): ("subst LDS",) * 2,
    (1, 4): ("invert LDS",) * 2,
    (9, 3): ("subst LDS",) * 2,        # one 8-row batch
    (16, 16): ("subst LDS",) * 2,      # batches without a remainder at some steps
    (17, 5): ("subst LDS",) * 2,       # two batches and a remainder
    (17, 70): ("invert LDS",) * 2,     # the identity as right-hand sides: one wave, 17 of its 64 lanes live
    (64, 65): ("subst LDS",) * 2,      # two waves, 63 dead lanes in the second
    (126, 9): ("subst LDS",) * 2,      # f64: 65 520 B of LDS
    (127, 9): ("subst LDS",) * 2,      # f64: 66 040 B, above 64 KiB
    (129, 130): ("subst LDS",) * 2,    # f64: 67 080 B, the last LDS size
    (129, 516): ("invert LDS",) * 2,
    (130, 7): ("subst global", "subst LDS"),
    (130, 520): ("invert global", "invert LDS"),
    (256, 1024): ("invert global", "invert LDS"),
    (257, 1030): ("subst global", "subst LDS"),
    (259, 5): ("subst global", "subst LDS"),   # f32: 67 340 B, the last LDS size
    (260, 5): ("subst global",) * 2,
    (300, 1): ("subst global",) * 2,
}
KERNEL_SHAPES = list(PATHS)
CPU_SHAPES = [(1, 1), (1, 4), (9, 3), (17, 70), (64, 65), (129, 70), (130, 520), (256, 40), (300, 9)]
RIGHT_SHAPES = [(33, 129), (130, 17)]


def _substitute(T, R):
    """X with T X = R by forward substitution in float64 (T lower triangular)."""
    X = np.array(R, dtype=np.float64)
    k = T.shape[0]
    for b0 in range(0, k, 64):  # 64 rows at a time, so that most of the work is one product per block
        b1 = min(k, b0 + 64)
        if b0:
            X[b0:b1] -= T[b0:b1, :b0] @ X[:b0]
        for i in range(b0, b1):
            if i > b0:
                X[i] -= T[i, b0:i] @ X[b0:i]
            X[i] /= T[i, i]
    return X


@functools.lru_cache(maxsize=None)
def family(k, nrhs, unit):
    """(T, B, X_lower, X_upper): the k x k lower triangular T of the exact family,
    the k x nrhs right-hand sides, and the float64 solutions of T X = alpha B and
    T^T X = alpha B, each verified by an exact float64 product.  Read-only."""
    rng = np.random.default_rng(7919 * k + 31 * nrhs + int(unit))
    r, c = np.indices((k, k))
    S = rng.permutation(k) < k // 2
    Nt = rng.integers(-2, 3, (k, k)).astype(np.float64) * ((r > c) & S[None, :] & ~S[:, None])
    assert not Nt[S, :].any() and not Nt[:, ~S].any()  # rows outside S, columns inside: Nt^2 = 0
    Nf, NtNf = np.zeros((k, k)), np.zeros((k, k))
    for i in range(1, k):
        d = rng.choice([d for d in (1, 17, 64) if d <= i])
        sign = rng.choice([-1.0, 1.0])
        Nf[i, i - d] = sign
        NtNf[:, i - d] += Nt[:, i] * sign
    Lm = np.eye(k) + Nt - Nf - NtNf  # (I + Nt)(I - Nf)
    assert np.array_equal(np.tril(Lm), Lm) and (np.diag(Lm) == 1).all()
    T = Lm if unit else Lm * np.exp2(rng.integers(-1, 2, k))[None, :]
    B = rng.integers(-4, 5, (k, nrhs)).astype(np.float64)
    Xl = _substitute(T, ALPHA * B)
    # T^T X = alpha B, backwards (a contiguous copy: numpy multiplies reversed views without BLAS)
    Xu = np.ascontiguousarray(_substitute(np.ascontiguousarray(T[::-1, ::-1].T), ALPHA * B[::-1])[::-1])
    assert np.array_equal(T @ Xl, ALPHA * B) and np.array_equal(T.T @ Xu, ALPHA * B)
    assert np.array_equal(Xl, np.rint(Xl)) and np.array_equal(Xu, np.rint(Xu))
    for a in (T, B, Xl, Xu):
        a.setflags(write=False)
    return T, B, Xl, Xu


@functools.lru_cache(maxsize=None)
def bounds(k, nrhs, unit, block):
    """The largest magnitude any correct algorithm can meet on family(k, nrhs,
    unit) when the diagonal blocks of `block` rows may be inverted, from the
    float64 reference alone (conditions on the inputs, not measurements):
      max(|alpha B| + |T||X|)      substitution and the GEMM updates between blocks
      max(|T_bb||W_bb|)            inverting a block by substitution on the identity
      max(|W_bb| |T_bb X_b|)       applying the inverse to the block's updated rows
    for op(A) = T and T^T; asserted below 2^22."""
    T, B, Xl, Xu = family(k, nrhs, unit)
    aT = np.abs(T)
    worst = [max((np.abs(ALPHA * B) + aT @ np.abs(Xl)).max(), (np.abs(ALPHA * B) + aT.T @ np.abs(Xu)).max()), 0.0, 0.0]
    for b0 in range(0, k, block):
        b1 = min(k, b0 + block)
        Tbb = T[b0:b1, b0:b1]
        W = _substitute(Tbb, np.eye(b1 - b0))
        assert np.array_equal(Tbb @ W, np.eye(b1 - b0)) and np.array_equal(4 * W, np.rint(4 * W))
        aW, aTbb = np.abs(W), np.abs(Tbb)
        worst[1] = max(worst[1], (aTbb @ aW).max(), (aW @ aTbb).max())
        worst[2] = max(worst[2], (aW @ np.abs(Tbb @ Xl[b0:b1])).max(), (aW.T @ np.abs(Tbb.T @ Xu[b0:b1])).max())
    assert max(worst) < LIMIT, (k, nrhs, unit, block, worst)
    return tuple(worst)


def system(side, uplo, orient, diag, m, n, block=None):
    """(A, B, X) in float64 for B := alpha op(A)^-1 B (LEFT) / alpha B op(A)^-1
    (RIGHT): A masked with NaN wherever the solve must not read, B m x n, X the
    exact result.  block: the rows of a diagonal block the path may invert
    (default: the whole triangle)."""
    left = side == el.LEFT
    k, nrhs = (m, n) if left else (n, m)
    unit = diag == el.UNIT
    T, B, Xl, Xu = family(k, nrhs, unit)
    bounds(k, nrhs, unit, min(block or k, k))
    lower, trans = uplo == el.LOWER, orient != el.NORMAL
    A = masked_triangle(T if lower else T.T, uplo, diag)
    # LEFT solves op(A) X = alpha B; RIGHT solves op(A)^T X^T = alpha B^T
    op_is_T = (lower != trans) if left else (lower == trans)
    X = Xl if op_is_T else Xu
    return (A, B, X) if left else (A, B.T, X.T)


def plan(dtype, m, n):
    """kernels.hpp trsm_plan through the C ABI: (path name, LDS bytes)."""
    inv, lds, nbytes = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    L.call("elx_trsm_plan", dtype, m, n, ctypes.byref(inv), ctypes.byref(lds), ctypes.byref(nbytes))
    return ("invert" if inv.value else "subst") + (" LDS" if lds.value else " global"), nbytes.value


def _stage(X, ld, off, device):
    """The column-major X with leading dimension ld, `off` elements into a buffer
    whose padding is NaN (any read of it shows in the result).  Returns (host
    image, the object that owns the memory the library sees, pointer to X(0,0))."""
    rows, cols = X.shape
    buf = np.full(off + ld * cols, np.nan, X.dtype)
    buf[off:].reshape(cols, ld)[:, :rows] = X.T
    if device == el.GPU:
        import torch
        t = torch.from_numpy(buf.copy()).cuda()
        return buf, t, t.data_ptr() + off * X.dtype.itemsize
    work = buf.copy()
    return buf, work, work.ctypes.data + off * X.dtype.itemsize


def _image(owner, device):
    return owner.cpu().numpy() if device == el.GPU else owner


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def matrix_case(device, dtype, side, uplo, orient, diag, m, n, pad):
    """One elx_matrix_trsm call on the exact family.  Returns None or what went
    wrong: the result differs from X in any bit, A or B's padding changed, or (GPU,
    LEFT) the launch was not the one the plan names for the shape."""
    npdt = NPDT[dtype]
    A, B, X = system(side, uplo, orient, diag, m, n)
    k = A.shape[0]
    lda, ldb, off = (k + 3, m + 1, 1) if pad else (k, m, 0)
    A0, ownA, pA = _stage(A.astype(npdt), lda, off, device)
    B0, ownB, pB = _stage(B.astype(npdt), ldb, off, device)
    if device == el.GPU:
        import torch
        torch.cuda.synchronize()
    L.call("elx_matrix_trsm", dtype, device, side, uplo, orient, diag, m, n, ALPHA, pA, lda, pB, ldb, None)
    if device == el.GPU:
        L.call("elx_device_synchronize")
    why = []
    if device == el.GPU and side == el.LEFT:
        want = PATHS[(m, n)][0 if dtype == el.F64 else 1]
        named, _ = plan(dtype, m, n)
        ran = L.lib().elx_trsm_last_launch()
        if named != want:
            why.append(f"the plan names '{named}', the table '{want}'")
        if ran != (1 if want.startswith("invert") else 0) | (2 if want.endswith("LDS") else 0):
            why.append(f"launch code {ran} is not '{want}'")
    A1, B1 = _image(ownA, device), _image(ownB, device)
    if not np.array_equal(_bits(A1), _bits(A0)):
        why.append("A was written")
    got = B1[off:].reshape(n, ldb)[:, :m].T
    if not np.array_equal(got, X.astype(npdt)):
        bad = got != X.astype(npdt)
        why.append(f"{int(bad.sum())} of {m * n} entries differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}")
    B0v, B1v = B0.copy(), B1.copy()
    B0v[off:].reshape(n, ldb)[:, :m] = 0
    B1v[off:].reshape(n, ldb)[:, :m] = 0
    if not np.array_equal(_bits(B1v), _bits(B0v)):
        why.append("B's padding was written")
    return "; ".join(why) or None


def run_matrix(device, side, shapes, dtypes=(el.F64, el.F32), uplos=(el.LOWER, el.UPPER)):
    """Every orientation x diag x shape x (aligned, padded) of the given types and
    triangles; one assertion over the collected failures."""
    bad = []
    for dtype in dtypes:
        for uplo in uplos:
            for orient in (el.NORMAL, el.TRANSPOSE):
                for diag in (el.NON_UNIT, el.UNIT):
                    for (m, n) in shapes:
                        for pad in (False, True):
                            why = matrix_case(device, dtype, side, uplo, orient, diag, m, n, pad)
                            if why:
                                bad.append((("f32", "f64")[dtype], "LU"[uplo], "NT"[orient], "NU"[diag], m, n,
                                            "padded" if pad else "aligned", why))
    assert not bad, f"{len(bad)} cases: {bad[:20]}"


def dist_case(g, device, dtype, side, uplo, orient, diag, m, n, nb):
    """One El::Trsm call on a 1x1 grid on the exact family (the caller has set the
    Blocksize; nb: the rows of the diagonal blocks it leads to).  None or what went wrong."""
    npdt = NPDT[dtype]
    A, B, X = system(side, uplo, orient, diag, m, n, nb)
    k = A.shape[0]
    Ad = el.DistMatrix(g, dtype, el.MC, el.MR, device, height=k, width=k)
    Bd = el.DistMatrix(g, dtype, el.MC, el.MR, device, height=m, width=n)
    Ad.set_local(A.astype(npdt))
    Bd.set_local(B.astype(npdt))
    el.Trsm(side, uplo, orient, diag, ALPHA, Ad, Bd)
    got = Bd.get_local()
    if not np.array_equal(_bits(np.ascontiguousarray(Ad.get_local())), _bits(np.ascontiguousarray(A.astype(npdt)))):
        return "A was written"
    if not np.array_equal(got, X.astype(npdt)):
        bad = got != X.astype(npdt)
        return f"{int(bad.sum())} of {m * n} entries differ, first at {tuple(int(v) for v in np.argwhere(bad)[0])}"
    return None


def run_dist(device, cases, blocksize, nb=None):
    """cases: (dtype, side, uplo, orient, diag, m, n) through El::Trsm on a 1x1 grid
    with the given Blocksize (restored afterwards); nb: the block rows the driver
    uses when it widens the Blocksize itself."""
    g = el.Grid()
    old = el.Blocksize()
    el.SetBlocksize(blocksize)
    bad = []
    try:
        for (dtype, side, uplo, orient, diag, m, n) in cases:
            why = dist_case(g, device, dtype, side, uplo, orient, diag, m, n, nb or blocksize)
            if why:
                bad.append((("f32", "f64")[dtype], "LR"[side], "LU"[uplo], "NT"[orient], "NU"[diag], m, n, why))
    finally:
        el.SetBlocksize(old)
    assert not bad, f"{len(bad)} cases: {bad}"


def all_sixteen(dtype, m, n):
    return [(dtype, side, uplo, orient, diag, m, n) for side in (el.LEFT, el.RIGHT) for uplo in (el.LOWER, el.UPPER)
            for orient in (el.NORMAL, el.TRANSPOSE) for diag in (el.NON_UNIT, el.UNIT)]


def dist_worker(rank, device, cases, blocksize, nb):
    """run_dist in a fresh process (mp.spawn, one rank): for knobs the library
    reads once per process, set in the parent's environment before the spawn."""
    import traceback
    try:
        run_dist(device, cases, blocksize, nb)
    except Exception:
        traceback.print_exc()
        raise
