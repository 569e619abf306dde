"""El::Cholesky on one MI355X (Grid 1x1, DistMatrix API) against the vendor route.

  python tools/cholesky_bench.py [n] [reps]

A = G G^T + n I (G uniform in [-1, 1]), n^3 / 3 algorithmic FLOPs.  In one
process, for f64 and f32 and LOWER / UPPER, interleaved per repetition:
  (a) el.Cholesky on a DistMatrix attached to the work buffer;
  (b) torch.linalg.cholesky on the same matrix: the vendor solver, the route the
      reference's GPU build takes for its diagonal blocks.  If it raises, the
      line says "vendor route unavailable" and the run continues.
The input is restored from a saved copy outside the timed region.  One warm-up,
then the median (min .. max) of `reps` timed repetitions each.
  (c) the leaf alone: elx_matrix_cholesky at n = kPotrfMax (one potrf_kernel
      launch plus the status read-back the entry point needs), beside the same
      call at n = 1 (the launch + read-back floor), and the leaf time times
      n / kPotrfMax as a share of (a).
Last, f64 LOWER in the reference's flat nb-step order (ELX_CHOLESKY_FLAT=1) and in
the recursive split down to single leaves (ELX_CHOLESKY_SWEEP=0), both as Trsm and
Syrk calls on views, against the recursive split with the local leaf-by-leaf
sweep of blocks of 512 .. 4096 rows (the default is 1024).
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elemental_amd import el
from elemental_amd import _lib as L


SWEEPS = (512, 1024, 2048, 4096)


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


def leaf_us(dt, tdt, n, reps=200):
    """Median wall time of elx_matrix_cholesky on one n x n leaf, in microseconds."""
    A0 = hpd(n, tdt, 5)
    A = A0.clone()
    ts = []
    for rep in range(reps + 5):
        A.copy_(A0)
        t = timed(lambda: L.call("elx_matrix_cholesky", dt, el.GPU, el.LOWER, n, A.data_ptr(), n, None))
        if rep >= 5:
            ts.append(t)
    return statistics.median(ts) * 1e6


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    g = el.Grid()
    el.SetBlocksize(128)
    nb = int(L.lib().elx_cholesky_leaf_max())
    os.environ["ELX_CHOLESKY_FLAT"] = "0"
    for dt, tdt, name in ((el.F64, torch.float64, "f64"), (el.F32, torch.float32, "f32")):
        A0 = hpd(n, tdt, 1)
        W = A0.clone()
        D = el.DistMatrix(g, dt, height=0, width=0)
        D.attach(n, n, 0, 0, W.data_ptr(), n)
        med = {}
        for uplo in (el.LOWER, el.UPPER):
            t_el, t_vendor, vendor_err = [], [], None
            for rep in range(reps + 1):
                W.copy_(A0)
                t = timed(lambda: el.Cholesky(uplo, D))
                if rep:
                    t_el.append(t)
                if vendor_err is None:
                    try:
                        t = timed(lambda: torch.linalg.cholesky(A0, upper=uplo == el.UPPER))
                        if rep:
                            t_vendor.append(t)
                    except Exception as e:  # noqa: BLE001
                        vendor_err = e
            case = f"{name} {'LU'[uplo]} n={n}"
            md = statistics.median(t_el)
            med[uplo] = md
            print(f"{case} el.Cholesky:           {stats(t_el)}  {n**3/3/md/1e12:6.2f} TFLOP/s", flush=True)
            if vendor_err is not None or not t_vendor:
                print(f"{case} torch.linalg.cholesky: vendor route unavailable ({vendor_err})", flush=True)
            else:
                vm = statistics.median(t_vendor)
                spreads = (max(t_el) - min(t_el)) + (max(t_vendor) - min(t_vendor))
                print(f"{case} torch.linalg.cholesky: {stats(t_vendor)}  {n**3/3/vm/1e12:6.2f} TFLOP/s  "
                      f"el/vendor {md/vm:.3f}  {'wins' if vm - md > spreads else 'NO WIN'} beyond the spreads",
                      flush=True)
        leaf = leaf_us(dt, tdt, nb)
        floor = leaf_us(dt, tdt, 1)
        share = leaf * 1e-6 * (n / nb) / med[el.LOWER]
        print(f"{name} leaf alone n={nb}: {leaf:.1f} us per call (n=1: {floor:.1f} us, launch + status read-back); "
              f"x {n // nb} leaves = {leaf*1e-3*(n/nb):.2f} ms = {100*share:.1f} % of el.Cholesky L "
              f"({100*max(leaf-floor, 0)*1e-6*(n/nb)/med[el.LOWER]:.1f} % without the floor)", flush=True)
        if dt == el.F64:
            # (flat, sweep rows): the reference's flat order and the pure recursion, both
            # as Trsm / Syrk calls on views, then the local sweep at several block sizes
            variants = [("1", "0"), ("0", "0")] + [("0", str(r)) for r in SWEEPS]
            ts = {v: [] for v in variants}
            for rep in range(reps + 1):
                for v in variants:
                    os.environ["ELX_CHOLESKY_FLAT"], os.environ["ELX_CHOLESKY_SWEEP"] = v
                    W.copy_(A0)
                    t = timed(lambda: el.Cholesky(el.LOWER, D))
                    if rep:
                        ts[v].append(t)
            os.environ["ELX_CHOLESKY_FLAT"] = "0"
            del os.environ["ELX_CHOLESKY_SWEEP"]
            for v in variants:
                what = "flat nb-step order on views" if v[0] == "1" else \
                    "recursive split down to leaves" if v[1] == "0" else f"recursive split, sweep {v[1]:>5s}"
                print(f"f64 L n={n} {what:31s}: {stats(ts[v])}", flush=True)
        del D, W, A0


if __name__ == "__main__":
    main()
