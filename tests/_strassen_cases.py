"""Exact cases shared by the Strassen-Winograd tests (CPU and GPU).

Operands are integers in [-2, 2] and alpha, beta powers of two: with k <= 512
every operand sum (|.| <= 6), product and partial sum (< 2^24 at two levels as
well) is exact in fp32 and fp64, so the result equals numpy's float64 product bit
for bit whatever the schedule.  The references are computed once and kept.
"""
from __future__ import annotations

import functools

import numpy as np

PAIRS = [(1.0, 0.0), (-1.0, 1.0), (0.5, -0.5)]
FORCE_MIN = "128"


@functools.lru_cache(maxsize=None)
def case(m: int, n: int, k: int, ta: str, tb: str, pad: int = 0):
    """(A, B, C0, product) in float64; A, B in stored layout with `pad` extra
    rows (leading dimension > row count), product = op(A) op(B)."""
    rng = np.random.default_rng(1000 * m + 10 * n + k + (ta == "T") + 2 * (tb == "T"))
    sa = (m, k) if ta == "N" else (k, m)
    sb = (k, n) if tb == "N" else (n, k)

    def ints(shape):
        full = np.asfortranarray(rng.integers(-2, 3, (shape[0] + pad, shape[1])).astype(np.float64))
        return full

    A, B, C = ints(sa), ints(sb), ints((m, n))
    Av, Bv = A[:sa[0]], B[:sb[0]]
    P = (Av if ta == "N" else Av.T) @ (Bv if tb == "N" else Bv.T)
    for x in (A, B, C, P):
        x.setflags(write=False)
    return A, B, C, P


def expected(C0: np.ndarray, P: np.ndarray, m: int, alpha: float, beta: float) -> np.ndarray:
    """What the padded C must hold afterwards: rows beyond m untouched."""
    want = C0.copy()
    want[:m] = alpha * P + (beta * C0[:m] if beta != 0.0 else 0.0)
    return want


def start_c(C0: np.ndarray, m: int, beta: float, dtype) -> np.ndarray:
    """C on entry: NaN in the m x n block where beta == 0 (it must never be read)."""
    C = np.asfortranarray(C0.astype(dtype))
    if beta == 0.0:
        C[:m] = np.nan
    return C
