"""The Level-2 kernels on one MI355X against the vendor's torch.mv / torch.addr.

  python tools/level2_bench.py [--quick]    the timing table
  python tools/level2_bench.py --trace      a few calls of every kernel (for rocprofv3
                                            --kernel-trace --stats: the reduce launches' share)

One process.  Every case is warmed, then timed `REPS` times with device events around
enough back-to-back calls to fill about 0.2 s, ours and the vendor's alternated.  The
operands of one call are larger than the 256 MiB Infinity Cache, or the calls rotate
among copies that together hold 2 GiB, eight times the cache, so none stays resident.
Algorithmic bytes: m n elements for
Gemv, n (n + 1) / 2 for Symv, twice that for the updates (read and write), plus the
vectors.  torch has no symv: its line is torch.mv on the full matrix, and the claim to
check is that reading half the bytes takes about half that time.  Streaming yardsticks
recorded elsewhere: Axpy / Hadamard at 5.69 / 5.86 TB/s (BENCH_r05.json).
"""
import math
import os
import statistics
import sys

REPS = 5
FILL = 0.2  # seconds of back-to-back calls per timed sample
RESIDENT = 2 << 30  # rotate among copies until this many bytes are swept


def main():
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from elemental_amd import el
    from elemental_amd import _lib as L

    quick, trace = "--quick" in sys.argv, "--trace" in sys.argv
    # a stream of torch's own, made current: the library's calls and torch.mv queue on it,
    # and so do the timing events (a null stream would mean the library's compute stream)
    side = torch.cuda.Stream()
    torch.cuda.set_stream(side)
    stream = side.cuda_stream
    tdt = {el.F64: torch.float64, el.F32: torch.float32, el.BF16: torch.bfloat16}
    names = {el.F64: "f64", el.F32: "f32", el.BF16: "bf16"}

    def sample(fn, inner):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for q in range(inner):
            fn(q)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / inner

    def measure(ours, vendor):
        """medians and spreads of REPS alternated samples; vendor may be None."""
        for fn in (ours, vendor):
            if fn is not None:
                fn(0)
        torch.cuda.synchronize()
        inner = max(1, min(200, math.ceil(FILL / max(sample(ours, 1), 1e-6))))
        t_o, t_v = [], []
        for _ in range(REPS):
            t_o.append(sample(ours, inner))
            if vendor is not None:
                t_v.append(sample(vendor, inner))
        return t_o, t_v

    def report(case, nbytes, t_o, t_v, vendor_name):
        mo = statistics.median(t_o)
        line = (f"{case:34s} {mo * 1e6:9.1f} us (min {min(t_o) * 1e6:.1f} max {max(t_o) * 1e6:.1f})  "
                f"{nbytes / 2**20:8.1f} MiB  {nbytes / mo / 1e12:5.2f} TB/s")
        if t_v:
            mv = statistics.median(t_v)
            spreads = (max(t_o) - min(t_o)) + (max(t_v) - min(t_v))
            verdict = "faster" if mv - mo > spreads else "slower" if mo - mv > spreads else "even"
            line += (f"  | {vendor_name} {mv * 1e6:9.1f} us (min {min(t_v) * 1e6:.1f} max {max(t_v) * 1e6:.1f})  "
                     f"ours/vendor {mo / mv:.3f} ({verdict} beyond the spreads)")
        print(line, flush=True)

    def run_shape(dt, m, n):
        es = torch.empty((), dtype=tdt[dt]).element_size()
        copies = max(1, math.ceil(RESIDENT / (m * n * es))) if m * n * es < RESIDENT else 1
        gen = torch.Generator(device="cuda").manual_seed(1)
        # the column-major m x n matrix as the row-major (n, m) tensor that shares its memory
        As = [(torch.rand(n, m, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1).to(tdt[dt])
              for _ in range(copies)]
        xm = (torch.rand(m, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1).to(tdt[dt])
        xn = (torch.rand(n, dtype=torch.float32, device="cuda", generator=gen) * 2 - 1).to(tdt[dt])
        ym, yn = torch.zeros_like(xm), torch.zeros_like(xn)
        tag = f"{names[dt]} {m}x{n}"

        def gemv(trans):
            x, y = (xm, yn) if trans else (xn, ym)
            return lambda q: L.call("elx_matrix_gemv", dt, el.GPU, el.TRANSPOSE if trans else el.NORMAL, m, n, 1.0,
                                    As[q % copies].data_ptr(), m, x.data_ptr(), 1, 0.0, y.data_ptr(), 1, stream)

        if trace:
            for fn in (gemv(False), gemv(True)):
                fn(0), fn(1)
        else:
            vec_bytes = (m + n) * es
            t_o, t_v = measure(gemv(False), lambda q: torch.mv(As[q % copies].T, xn, out=ym))
            report(f"Gemv N {tag}", m * n * es + vec_bytes, t_o, t_v, "torch.mv")
            t_o, t_v = measure(gemv(True), lambda q: torch.mv(As[q % copies], xm, out=yn))
            report(f"Gemv T {tag}", m * n * es + vec_bytes, t_o, t_v, "torch.mv")
        if dt == el.BF16:
            return

        def ger(q):
            L.call("elx_matrix_ger", dt, el.GPU, m, n, 1e-3, xm.data_ptr(), 1, xn.data_ptr(), 1,
                   As[q % copies].data_ptr(), m, stream)

        if trace:
            ger(0), ger(1)
        else:
            t_o, t_v = measure(ger, lambda q: As[q % copies].addr_(xn, xm, alpha=1e-3))
            report(f"Ger    {tag}", 2 * m * n * es + (m + n) * es, t_o, t_v, "torch.addr")
        if m != n:
            return
        tri = n * (n + 1) // 2 * es
        for uplo, u in ((el.LOWER, "L"), (el.UPPER, "U")):
            def symv(q, uplo=uplo):
                L.call("elx_matrix_symv", dt, el.GPU, uplo, n, 1.0, As[q % copies].data_ptr(), n, xn.data_ptr(), 1, 0.0,
                       yn.data_ptr(), 1, stream)
            if trace:
                symv(0), symv(1)
                continue
            t_o, t_v = measure(symv, lambda q: torch.mv(As[q % copies].T, xn, out=ym))
            report(f"Symv {u} {tag}", tri + 2 * n * es, t_o, t_v, "torch.mv (full matrix)")

        def syr2(q):
            L.call("elx_matrix_syr2", dt, el.GPU, el.LOWER, n, 1e-3, xn.data_ptr(), 1, xm.data_ptr(), 1,
                   As[q % copies].data_ptr(), n, stream)

        if trace:
            syr2(0), syr2(1)
        else:
            t_o, _ = measure(syr2, None)
            report(f"Syr2 L {tag}", 2 * tri + 2 * n * es, t_o, [], "")

    big = 4096 if quick or trace else 16384
    long_ = 16384 if quick or trace else 65536
    for dt in (el.F64, el.F32):
        for (m, n) in ((big, big), (long_, 1024), (1024, long_)):
            run_shape(dt, m, n)
    run_shape(el.BF16, 2 * big, 2 * big)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
