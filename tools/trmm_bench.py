"""El::Trmm on one MI355X (Grid 1x1, DistMatrix API) against the route without it.

  python tools/trmm_bench.py [m] [n] [reps] [leaf ...]

LEFT B := op(tri(A)) B with A m x m and B m x n: m^2 n algorithmic FLOPs.  In
one process, interleaved per repetition, for f64 and f32 and every (uplo,
orientation):
  (a) el.Trmm, once per leaf size (ELX_TRMM_LEAF, read per call; 0 keeps the
      128-row blocksize as the leaf; -1 sets the blocksize to m: one leaf, the
      triangle-aware kernel alone on the whole matrix);
  (b) el.Gemm with a copy of A whose other triangle is zeroed, into a second
      matrix; the zeroing and the copy back are not timed, so (b) is a floor
      for that route.
One warm-up, then the median (min .. max) of `reps` timed repetitions each.
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from elemental_amd import el
from elemental_amd import _lib as L


def timed(fn):
    L.call("elx_device_synchronize")
    t = time.perf_counter()
    fn()
    L.call("elx_device_synchronize")
    return time.perf_counter() - t


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 16384
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    leaves = [int(x) for x in sys.argv[4:]] or [1024]
    g = el.Grid()
    el.SetBlocksize(128)
    for dt, name in ((el.F64, "f64"), (el.F32, "f32")):
        A = el.DistMatrix(g, dt, height=m, width=m).fill_hash(1, -1.0, 1.0)
        Az = el.DistMatrix(g, dt, height=m, width=m)
        B0 = el.DistMatrix(g, dt, height=m, width=n).fill_hash(2, -1.0, 1.0)
        B = el.DistMatrix(g, dt, height=m, width=n)
        C = el.DistMatrix(g, dt, height=m, width=n)
        for uplo in (el.LOWER, el.UPPER):
            Az.assign(A)
            # zero the strict other triangle: upper is gi <= gj - 1, lower gi >= gj + 1
            el.ScaleTrapezoid(0.0, el.UPPER if uplo == el.LOWER else el.LOWER, Az, 1 if uplo == el.LOWER else -1)
            for orient in (el.NORMAL, el.TRANSPOSE):
                t_trmm = {leaf: [] for leaf in leaves}
                t_gemm = []
                for rep in range(reps + 1):
                    for leaf in leaves:
                        os.environ["ELX_TRMM_LEAF"] = str(max(leaf, 0))
                        el.SetBlocksize(m if leaf < 0 else 128)
                        B.assign(B0)
                        t = timed(lambda: el.Trmm(el.LEFT, uplo, orient, el.NON_UNIT, 1.0, A, B))
                        if rep:
                            t_trmm[leaf].append(t)
                    el.SetBlocksize(128)
                    t = timed(lambda: el.Gemm(orient, el.NORMAL, 1.0, Az, B0, 0.0, C))
                    if rep:
                        t_gemm.append(t)
                case = f"{name} L{'LU'[uplo]}{'NT'[orient]} m={m} n={n}"
                gm = statistics.median(t_gemm)
                print(f"{case} Gemm on zeroed A: median {gm*1e3:8.2f} ms (min {min(t_gemm)*1e3:.2f} max "
                      f"{max(t_gemm)*1e3:.2f})", flush=True)
                for leaf in leaves:
                    ts = t_trmm[leaf]
                    md = statistics.median(ts)
                    spreads = (max(ts) - min(ts)) + (max(t_gemm) - min(t_gemm))
                    print(f"{case} Trmm leaf {m if leaf < 0 else leaf if leaf else 128:5d}: median {md*1e3:8.2f} ms (min "
                          f"{min(ts)*1e3:.2f} max {max(ts)*1e3:.2f})  {m*m*n/md/1e12:6.2f} TFLOP/s  "
                          f"{md/gm:.3f} x Gemm  {'wins' if gm - md > spreads else 'NO WIN'} beyond the spreads",
                          flush=True)
        del A, Az, B0, B, C


if __name__ == "__main__":
    main()
