"""El::LU on one MI355X (Grid 1x1, DistMatrix API) against the vendor route.

  python tools/lu_bench.py [n ...] [--reps R]     the timing table
  python tools/lu_bench.py --trace n              one warm-up and one f64 run (for rocprofv3)
  python tools/lu_bench.py --stages kernel_stats.csv   the per-stage split of such a trace

A is uniform in [-1, 1], 2 n^3 / 3 algorithmic FLOPs.  In one process, for f64 and
f32, interleaved per repetition:
  (a) el.LU on a DistMatrix attached to the work buffer;
  (b) torch.linalg.lu_factor on the same matrix: the vendor solver.  If it raises,
      the line says "vendor route unavailable" and the run continues;
  (c) this library's own GEMM at the same n (elx_gemm, NN, 2 n^3 FLOPs): the rate
      the Level-3 part of the factorization could reach.
The input is restored from a saved copy outside the timed region.  One warm-up,
then the median (min .. max) of `reps` timed repetitions each.
"""
import csv
import os
import statistics
import sys
import time

STAGES = (("leaf steps", ("getrf_step",)), ("leaf finish", ("getrf_finish",)), ("laswp", ("laswp",)),
          ("trsm substitution / inverse", ("trsm", "tri_inverse")), ("gemm (updates and Trsm's products)", ("gemm",)),
          ("copies", ("copy2d", "Copy")))


def stages(path):
    """Group a rocprofv3 kernel_stats.csv by the stage each kernel belongs to."""
    tot = {name: [0, 0] for name, _ in STAGES}
    tot["other"] = [0, 0]
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for name, keys in STAGES:
                if any(k in row["Name"] for k in keys):
                    break
            else:
                name = "other"
            tot[name][0] += int(row["Calls"])
            tot[name][1] += int(float(row["TotalDurationNs"]))
    total = sum(v[1] for v in tot.values()) or 1
    for name, (calls, ns) in tot.items():
        print(f"{name:38s} {calls:8d} launches {ns / 1e6:10.2f} ms  {100 * ns / total:5.1f} %")
    print(f"{'all kernels':38s} {sum(v[0] for v in tot.values()):8d} launches {total / 1e6:10.2f} ms")


def main():
    args = sys.argv[1:]
    if args[:1] == ["--stages"]:
        return stages(args[1])
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

    def stats(ts):
        return f"median {statistics.median(ts)*1e3:8.2f} ms (min {min(ts)*1e3:.2f} max {max(ts)*1e3:.2f})"

    def uniform(n, tdt, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        return (torch.rand(n, n, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1).to(tdt)

    g = el.Grid()
    el.SetBlocksize(128)
    if args[:1] == ["--trace"]:
        n = int(args[1])
        A0 = uniform(n, torch.float64, 1)
        W = A0.clone()
        D = el.DistMatrix(g, el.F64, height=0, width=0)
        D.attach(n, n, 0, 0, W.data_ptr(), n)
        for _ in range(2):
            W.copy_(A0)
            print(f"el.LU f64 n={n}: {timed(lambda: el.LU(D))*1e3:.2f} ms", flush=True)
        return
    reps = 5
    if "--reps" in args:
        i = args.index("--reps")
        reps = int(args[i + 1])
        del args[i:i + 2]
    sizes = [int(a) for a in args] or [4096, 8192, 16384]
    for n in sizes:
        for dt, tdt, name, gemm in ((el.F64, torch.float64, "f64", "elx_gemm_f64"),
                                    (el.F32, torch.float32, "f32", "elx_gemm_f32")):
            A0 = uniform(n, tdt, 1)
            W = A0.clone()
            C = torch.empty_like(A0)
            D = el.DistMatrix(g, dt, height=0, width=0)
            D.attach(n, n, 0, 0, W.data_ptr(), n)  # the buffer as a column-major matrix: torch sees its transpose
            t_el, t_vendor, t_gemm, vendor_err = [], [], [], None
            for rep in range(reps + 1):
                W.copy_(A0)
                t = timed(lambda: el.LU(D))
                if rep:
                    t_el.append(t)
                if vendor_err is None:
                    try:
                        t = timed(lambda: torch.linalg.lu_factor(A0.T))
                        if rep:
                            t_vendor.append(t)
                    except Exception as e:  # noqa: BLE001
                        vendor_err = e
                t = timed(lambda: L.call(gemm, el.NORMAL, el.NORMAL, n, n, n, 1.0, A0.data_ptr(), n, W.data_ptr(), n,
                                         0.0, C.data_ptr(), n, None))
                if rep:
                    t_gemm.append(t)
            case = f"{name} n={n}"
            md, gm = statistics.median(t_el), statistics.median(t_gemm)
            rate, grate = 2 * n**3 / 3 / md / 1e12, 2 * n**3 / gm / 1e12
            print(f"{case} el.LU:                  {stats(t_el)}  {rate:6.2f} TFLOP/s  "
                  f"({rate / grate:.3f} of El::Gemm's {grate:.1f} TFLOP/s, {stats(t_gemm)})", flush=True)
            if vendor_err is not None or not t_vendor:
                print(f"{case} torch.linalg.lu_factor: vendor route unavailable ({vendor_err})", flush=True)
            else:
                vm = statistics.median(t_vendor)
                spreads = (max(t_el) - min(t_el)) + (max(t_vendor) - min(t_vendor))
                verdict = "wins" if vm - md > spreads else "loses" if md - vm > spreads else "ties"
                print(f"{case} torch.linalg.lu_factor: {stats(t_vendor)}  {2*n**3/3/vm/1e12:6.2f} TFLOP/s  "
                      f"el/vendor {md/vm:.3f}  el.LU {verdict} beyond the spreads", flush=True)
            del D, W, A0, C


if __name__ == "__main__":
    main()
