"""El::HermitianTridiag on one MI355X (elx_matrix_hermitian_tridiag on a device buffer).

  python tools/tridiag_bench.py [n ...] [--reps R] [--widths 32,64] [--eigvalsh]   the timing table
  python tools/tridiag_bench.py --trace n          one warm-up and one f64 LOWER run (for rocprofv3)
  python tools/tridiag_bench.py --stages kernel_stats.csv   the per-stage split of such a trace

A is symmetric, uniform in [-1, 1]; 4 n^3 / 3 algorithmic FLOPs.  In one process, for
f64 and f32, LOWER and UPPER and each panel width, the fused panel kernels and the
panel composed from the Level-2 routines (ELX_TRIDIAG_PANEL=level2) alternate per
repetition on the same input, restored from a saved copy outside the timed region.
One warm-up each, then the median (min .. max) of `reps` timed repetitions.

Beside each time: the HBM floor of the trailing Symv products, sum over the columns
of the triangle's bytes ~ n^3 / 6 elements, over the 8 TB/s peak and over the rate
profiles/level2_bench.log records for Symv at 16384 (f64 3.06 TB/s, f32 2.38 TB/s),
which is what this kernel set can reach without touching symv_kernel.

--eigvalsh: torch.linalg.eigvalsh on the same f64 matrix at the largest n, once, as
context only: it does strictly more work (the whole eigenvalue computation), so it
brackets from above and is not a like-for-like baseline.
"""
import csv
import os
import statistics
import sys
import time

PEAK_TBS = 8.0
SYMV_TBS = {"f64": 3.06, "f32": 2.38}  # profiles/level2_bench.log, Symv L 16384
STAGES = (("symv_kernel", ("symv_kernel",)), ("level2 reduce", ("level2_reduce",)),
          ("fused panel kernels (sytrd_*)", ("sytrd_",)), ("rank-2k update: gemm", ("gemm",)),
          ("rank-2k update: masked leaves", ("trapezoid", "Trapezoid")), ("copies", ("copy2d", "Copy")))


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
        print(f"{name:40s} {calls:8d} launches {ns / 1e6:10.2f} ms  {100 * ns / total:5.1f} %")
    print(f"{'all kernels':40s} {sum(v[0] for v in tot.values()):8d} launches {total / 1e6:10.2f} ms")


def symv_bytes(n, es):
    """The bytes the trailing products read: column k's triangle has (n-1-k)(n-k)/2 elements."""
    return es * sum((n - 1 - k) * (n - k) // 2 for k in range(n - 1))


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
        return f"median {statistics.median(ts)*1e3:9.2f} ms (min {min(ts)*1e3:.2f} max {max(ts)*1e3:.2f})"

    def symmetric(n, tdt, seed):
        gen = torch.Generator(device="cuda").manual_seed(seed)
        G = torch.rand(n, n, dtype=torch.float64, device="cuda", generator=gen) * 2 - 1
        return (torch.tril(G) + torch.tril(G, -1).T).to(tdt).contiguous()

    def run(dt, uplo, n, W, tau, panel, width):
        if panel == "level2":
            os.environ["ELX_TRIDIAG_PANEL"] = "level2"
        else:
            os.environ.pop("ELX_TRIDIAG_PANEL", None)
        L.call("elx_set_tridiag_panel_cols", width)
        L.call("elx_matrix_hermitian_tridiag", dt, el.GPU, uplo, n, W.data_ptr(), n, tau.data_ptr(), None)

    if args[:1] == ["--trace"]:
        n = int(args[1])
        A0 = symmetric(n, torch.float64, 1)
        W, tau = A0.clone(), torch.zeros(n, dtype=torch.float64, device="cuda")
        for _ in range(2):
            W.copy_(A0)
            t = timed(lambda: run(el.F64, el.LOWER, n, W, tau, "fused", int(L.lib().elx_tridiag_panel_cols())))
            print(f"HermitianTridiag f64 L {n}: {t*1e3:.2f} ms", flush=True)
        return
    reps, widths, eig = 5, [32, 64], "--eigvalsh" in args
    if eig:
        args.remove("--eigvalsh")
    if "--reps" in args:
        i = args.index("--reps")
        reps = int(args[i + 1])
        del args[i:i + 2]
    if "--widths" in args:
        i = args.index("--widths")
        widths = [int(x) for x in args[i + 1].split(",")]
        del args[i:i + 2]
    sizes = [int(a) for a in args] or [4096, 8192, 16384]
    for n in sizes:
        flops = 4 * n**3 / 3
        for dt, tdt, name in ((el.F64, torch.float64, "f64"), (el.F32, torch.float32, "f32")):
            A0 = symmetric(n, tdt, 1)
            W, tau = A0.clone(), torch.zeros(n, dtype=tdt, device="cuda")
            nbytes = symv_bytes(n, A0.element_size())
            print(f"{name} n={n}: Symv reads {nbytes / 2**30:.1f} GiB; HBM floor {nbytes / PEAK_TBS / 1e9:.1f} ms at "
                  f"{PEAK_TBS} TB/s, {nbytes / SYMV_TBS[name] / 1e9:.1f} ms at symv_kernel's recorded "
                  f"{SYMV_TBS[name]} TB/s", flush=True)
            for uplo, un in ((el.LOWER, "L"), (el.UPPER, "U")):
                for width in widths:
                    ts = {"fused": [], "level2": []}
                    for rep in range(reps + 1):
                        for panel in ("fused", "level2"):
                            W.copy_(A0)
                            t = timed(lambda: run(dt, uplo, n, W, tau, panel, width))
                            if rep:
                                ts[panel].append(t)
                    mf, ml = statistics.median(ts["fused"]), statistics.median(ts["level2"])
                    spreads = sum(max(v) - min(v) for v in ts.values())
                    verdict = "fused wins" if ml - mf > spreads else "level2 wins" if mf - ml > spreads else "tie"
                    case = f"{name} {un} n={n} w={width}"
                    print(f"{case} fused:  {stats(ts['fused'])}  {flops / mf / 1e12:6.3f} TFLOP/s", flush=True)
                    print(f"{case} level2: {stats(ts['level2'])}  {flops / ml / 1e12:6.3f} TFLOP/s  "
                          f"fused/level2 {mf / ml:.3f}  {verdict} beyond the spreads", flush=True)
            if eig and name == "f64" and n == max(sizes):
                try:
                    timed(lambda: torch.linalg.eigvalsh(A0))
                    print(f"context only: torch.linalg.eigvalsh f64 n={n}: "
                          f"{timed(lambda: torch.linalg.eigvalsh(A0))*1e3:.2f} ms (all eigenvalues: strictly more "
                          f"work, an upper bracket, not a baseline)", flush=True)
                except Exception as e:  # noqa: BLE001
                    print(f"context only: torch.linalg.eigvalsh unavailable ({e})", flush=True)
            del W, A0
    os.environ.pop("ELX_TRIDIAG_PANEL", None)
    L.call("elx_set_tridiag_panel_cols", 0)


if __name__ == "__main__":
    main()
