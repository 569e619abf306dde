"""El::QR on one MI355X (Grid 1x1, DistMatrix API) against the vendor route.

  python tools/qr_bench.py [m[xn] ...] [--reps R]   the timing table
  python tools/qr_bench.py --trace m[xn]            one warm-up and one f64 run (for rocprofv3)
  python tools/qr_bench.py --stages kernel_stats.csv   the per-stage split of such a trace

A is uniform in [-1, 1], 2 m n^2 - 2 n^3 / 3 algorithmic FLOPs (m >= n).  In one
process, for f64 and f32, interleaved per repetition:
  (a) el.QR on a DistMatrix attached to the work buffer;
  (b) torch.geqrf on the same matrix: the vendor solver.  If it raises, the line
      says "vendor route unavailable" and the run continues.
The input is restored from a saved copy outside the timed region.  One warm-up,
then the median (min .. max) of `reps` timed repetitions each.
"""
import csv
import os
import statistics
import sys
import time

# the U^T U product that forms T is a GEMM like the others and is counted with them
STAGES = (("leaf steps", ("geqrf_step",)), ("T forming (explicit U, fix-up)", ("qr_explicit_u", "qr_fix_t")),
          ("signature scaling", ("row_scale",)), ("trsm substitution / inverse", ("trsm", "tri_inverse")),
          ("gemm (U^T U, U^T B, B -= U Z, Trsm's products)", ("gemm",)), ("copies", ("copy2d", "Copy")))


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
        print(f"{name:48s} {calls:8d} launches {ns / 1e6:10.2f} ms  {100 * ns / total:5.1f} %")
    print(f"{'all kernels':48s} {sum(v[0] for v in tot.values()):8d} launches {total / 1e6:10.2f} ms")


def shape(arg):
    m, _, n = arg.partition("x")
    return int(m), int(n or m)


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

    def uniform(m, n, tdt, seed):
        """The column-major m x n matrix as the row-major (n, m) tensor that shares its memory."""
        gen = torch.Generator(device="cuda").manual_seed(seed)
        return (torch.rand(n, m, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1).to(tdt)

    g = el.Grid()
    el.SetBlocksize(128)
    if args[:1] == ["--trace"]:
        m, n = shape(args[1])
        A0 = uniform(m, n, torch.float64, 1)
        W = A0.clone()
        D = el.DistMatrix(g, el.F64, height=0, width=0)
        D.attach(m, n, 0, 0, W.data_ptr(), m)
        for _ in range(2):
            W.copy_(A0)
            print(f"el.QR f64 {m}x{n}: {timed(lambda: el.QR(D))*1e3:.2f} ms", flush=True)
        return
    reps = 5
    if "--reps" in args:
        i = args.index("--reps")
        reps = int(args[i + 1])
        del args[i:i + 2]
    shapes = [shape(a) for a in args] or [(4096, 4096), (8192, 8192), (16384, 16384), (65536, 1024)]
    for (m, n) in shapes:
        flops = 2 * m * n**2 - 2 * n**3 / 3
        for dt, tdt, name in ((el.F64, torch.float64, "f64"), (el.F32, torch.float32, "f32")):
            A0 = uniform(m, n, tdt, 1)
            W = A0.clone()
            D = el.DistMatrix(g, dt, height=0, width=0)
            D.attach(m, n, 0, 0, W.data_ptr(), m)
            t_el, t_vendor, vendor_err = [], [], None
            for rep in range(reps + 1):
                W.copy_(A0)
                t = timed(lambda: el.QR(D))
                if rep:
                    t_el.append(t)
                if vendor_err is None:
                    try:
                        t = timed(lambda: torch.geqrf(A0.T))
                        if rep:
                            t_vendor.append(t)
                    except Exception as e:  # noqa: BLE001
                        vendor_err = e
            case = f"{name} {m}x{n}"
            md = statistics.median(t_el)
            print(f"{case} el.QR:       {stats(t_el)}  {flops / md / 1e12:6.2f} TFLOP/s", flush=True)
            if vendor_err is not None or not t_vendor:
                print(f"{case} torch.geqrf: vendor route unavailable ({vendor_err})", flush=True)
            else:
                vm = statistics.median(t_vendor)
                spreads = (max(t_el) - min(t_el)) + (max(t_vendor) - min(t_vendor))
                verdict = "wins" if vm - md > spreads else "loses" if md - vm > spreads else "ties"
                print(f"{case} torch.geqrf: {stats(t_vendor)}  {flops / vm / 1e12:6.2f} TFLOP/s  "
                      f"el/vendor {md / vm:.3f}  el.QR {verdict} beyond the spreads", flush=True)
            del D, W, A0


if __name__ == "__main__":
    main()
