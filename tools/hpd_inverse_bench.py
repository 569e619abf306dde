"""El::HPDInverse on one MI355X (Grid 1x1, DistMatrix API): its stages, the vendor
route, and the El::HPDSolve-against-an-identity route it replaces.

  python tools/hpd_inverse_bench.py [n] [reps]
  python tools/hpd_inverse_bench.py [n] --profile

A = G G^T + n I (G uniform in [-1, 1]); n^3 algorithmic FLOPs for the inverse
(n^3/3 per stage).  In one process, for f64 and f32 and LOWER / UPPER, interleaved
per repetition:
  (a) el.HPDInverse on a DistMatrix attached to the work buffer;
  (b) its three stages one after the other on the same buffer: el.Cholesky,
      el.TriangularInverse, el.Trtrmm;
  (c) the vendor route: torch.cholesky_inverse(torch.linalg.cholesky(A)), and
      torch.linalg.solve_triangular(L, I) beside stage two.  If either raises,
      the line says "vendor route unavailable" and the run continues;
  (d) what a caller had to do before: El::HPDSolve against an identity (a copy of
      A, el.Cholesky on it, el.CholeskySolveAfter on B = I: 7 n^3 / 3 FLOPs and a
      second n x n matrix).
The input is restored from a saved copy outside the timed region.  One warm-up,
then the median (min .. max) of `reps` timed repetitions each.  Last, f64 LOWER
(a) with ELX_INVERSE_SWEEP=0 (every panel of the two new stages a Trsm / Syrk /
Trmm call on views; Cholesky keeps its own sweep) against the default local sweeps.

--profile: one small warm-up (n = 256) and one f64 LOWER el.HPDInverse at n, on a
matrix made without a GEMM, with the wall time printed: under a kernel trace the
sum of kernel time beside it is the GPU share, the rest is host time.  Run it
once as it is and once with ELX_INVERSE_SWEEP=0 in the environment.
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elemental_amd import el
from elemental_amd import _lib as L


def sync():
    torch.cuda.synchronize()
    L.call("elx_device_synchronize")


def timed(fn):
    sync()
    t = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t


def hpd(n, tdt, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    G = torch.rand(n, n, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
    A = G @ G.T
    A.diagonal().add_(n)
    return A.to(tdt)


def stats(ts):
    return f"median {statistics.median(ts)*1e3:8.2f} ms (min {min(ts)*1e3:.2f} max {max(ts)*1e3:.2f})"


def spread(ts):
    return max(ts) - min(ts)


def attach(g, dt, W, n):
    D = el.DistMatrix(g, dt, height=0, width=0)
    D.attach(n, n, 0, 0, W.data_ptr(), n)
    return D


def profile(n):
    g = el.Grid()
    el.SetBlocksize(128)
    for m in (256, n):
        gen = torch.Generator(device="cuda").manual_seed(3)
        R = torch.rand(m, m, dtype=torch.float64, device="cuda", generator=gen) - 0.5
        W = R + R.T  # |off-diagonal| < 1: strictly diagonally dominant below, so HPD
        del R
        W.diagonal().add_(2.0 * m)
        D = attach(g, el.F64, W, m)
        t = timed(lambda: el.HPDInverse(el.LOWER, D))
        print(f"profile f64 L n={m} ELX_INVERSE_SWEEP={os.environ.get('ELX_INVERSE_SWEEP', 'default')} "
              f"el.HPDInverse wall {t*1e3:.2f} ms", flush=True)
        del D, W


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    if "--profile" in sys.argv:
        return profile(n)
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    g = el.Grid()
    el.SetBlocksize(128)
    for dt, tdt, name in ((el.F64, torch.float64, "f64"), (el.F32, torch.float32, "f32")):
        A0 = hpd(n, tdt, 1)
        W = A0.clone()
        B = torch.empty_like(A0)
        eye = torch.eye(n, dtype=tdt, device="cuda")
        D, DB = attach(g, dt, W, n), attach(g, dt, B, n)
        for uplo in (el.LOWER, el.UPPER):
            keys = ("a", "chol", "trtri", "trtrmm", "potri", "vtrtri", "d")
            ts = {k: [] for k in keys}
            vendor_err = None

            def solve_identity():
                W.copy_(A0)
                B.copy_(eye)
                el.Cholesky(uplo, D)
                el.CholeskySolveAfter(uplo, el.NORMAL, D, DB)

            for rep in range(reps + 1):
                got = {}
                W.copy_(A0)
                got["a"] = timed(lambda: el.HPDInverse(uplo, D))
                W.copy_(A0)
                got["chol"] = timed(lambda: el.Cholesky(uplo, D))
                F = W.clone()  # the factor, for the vendor's triangular inverse
                got["trtri"] = timed(lambda: el.TriangularInverse(uplo, el.NON_UNIT, D))
                got["trtrmm"] = timed(lambda: el.Trtrmm(uplo, D))
                if vendor_err is None:
                    try:
                        up = uplo == el.UPPER
                        got["potri"] = timed(
                            lambda: torch.cholesky_inverse(torch.linalg.cholesky(A0, upper=up), upper=up))
                        T = F.T.triu() if up else F.T.tril()  # F is column-major: F.T is the matrix torch sees
                        got["vtrtri"] = timed(lambda: torch.linalg.solve_triangular(T, eye, upper=up))
                        del T
                    except Exception as e:  # noqa: BLE001
                        vendor_err = e
                del F
                got["d"] = timed(solve_identity)
                if rep:
                    for k, v in got.items():
                        ts[k].append(v)
            case = f"{name} {'LU'[uplo]} n={n}"
            md = {k: statistics.median(v) for k, v in ts.items() if v}
            fl = n ** 3
            print(f"{case} (a) el.HPDInverse:         {stats(ts['a'])}  {fl/md['a']/1e12:6.2f} TFLOP/s", flush=True)
            for k, what in (("chol", "el.Cholesky"), ("trtri", "el.TriangularInverse"), ("trtrmm", "el.Trtrmm")):
                print(f"{case} (b) {what:22s} {stats(ts[k])}  {fl/3/md[k]/1e12:6.2f} TFLOP/s  "
                      f"{100*md[k]/md['a']:.0f} % of (a)", flush=True)
            if vendor_err is not None or not ts["potri"] or not ts["vtrtri"]:
                print(f"{case} (c) vendor route unavailable ({vendor_err})", flush=True)
            else:
                print(f"{case} (c) torch cholesky+cholesky_inverse: {stats(ts['potri'])}  "
                      f"{fl/md['potri']/1e12:6.2f} TFLOP/s  el/vendor {md['a']/md['potri']:.3f}", flush=True)
                print(f"{case} (c) torch solve_triangular(L, I):    {stats(ts['vtrtri'])}  "
                      f"el.TriangularInverse/vendor {md['trtri']/md['vtrtri']:.3f}", flush=True)
            gain = md["d"] - md["a"]
            verdict = "faster" if gain > spread(ts["a"]) + spread(ts["d"]) else "NOT FASTER"
            print(f"{case} (d) HPDSolve against I:        {stats(ts['d'])}  (a)/(d) {md['a']/md['d']:.3f}  "
                  f"(a) is {verdict} beyond both spreads", flush=True)
        if dt == el.F64:
            variants = (("0", "ELX_INVERSE_SWEEP=0 (views)"), (None, "local sweeps (default)"))
            vt = {v: [] for v, _ in variants}
            for rep in range(reps + 1):
                for v, _ in variants:
                    if v is None:
                        os.environ.pop("ELX_INVERSE_SWEEP", None)
                    else:
                        os.environ["ELX_INVERSE_SWEEP"] = v
                    W.copy_(A0)
                    t = timed(lambda: el.HPDInverse(el.LOWER, D))
                    if rep:
                        vt[v].append(t)
            for v, what in variants:
                print(f"f64 L n={n} (a) {what:28s}: {stats(vt[v])}", flush=True)
        del D, DB, W, B, A0, eye


if __name__ == "__main__":
    main()
