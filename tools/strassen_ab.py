"""Plain kernel against one and two Strassen-Winograd levels, in one process.

  python tools/strassen_ab.py [dt,ta,tb,m,n,k ...]

elx_gemm_{f64,f32} on device buffers, Uniform(-0.5, 0.5) operands, alpha = 0.5, beta =
-0.5.  The knobs are read at every call, so the three variants alternate on the
same buffers: ELX_GEMM_STRASSEN=0, then 1 and 2 with ELX_GEMM_STRASSEN_MIN at the
shape's smallest dimension (2: its half for the inner level).  Best of 3 timings
each; rates are effective (2mnk / time).  The default shapes are the cubes
around the crossover and the large shapes of bench.py's points.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from elemental_amd import _lib as L
from gemm_bench import TD, timeit

DEFAULT = ["f64,0,0,4096,4096,4096", "f64,0,0,8192,8192,8192", "f64,0,0,12288,12288,12288",
           "f64,0,0,16384,16384,16384", "f64,0,0,32768,32768,32768", "f64,0,0,32768,32768,8192",
           "f64,1,0,16384,16384,16384", "f32,0,0,8192,8192,8192", "f32,0,0,16384,16384,16384",
           "f32,0,0,32768,32768,8192"]


def run(dt, ta, tb, m, n, k):
    tdt = TD[dt]
    lda, ldb = (k if ta else m), (n if tb else k)
    A = torch.rand(lda * (m if ta else k), dtype=torch.float32, device="cuda").sub_(0.5).to(tdt)
    B = torch.rand(ldb * (k if tb else n), dtype=torch.float32, device="cuda").sub_(0.5).to(tdt)
    C = torch.rand(m * n, dtype=torch.float32, device="cuda").sub_(0.5).to(tdt)
    fn = L.lib().elx_gemm_f64 if dt == "f64" else L.lib().elx_gemm_f32
    go = lambda: L.check(fn(ta, tb, m, n, k, 0.5, A.data_ptr(), lda, B.data_ptr(), ldb, -0.5, C.data_ptr(), m, None))
    small = min(m, n, k)
    line = f"{dt} {'T' if ta else 'N'}{'T' if tb else 'N'} {m}x{n}x{k}:"
    for levels in (0, 1, 2):
        os.environ["ELX_GEMM_STRASSEN"] = str(levels)
        os.environ["ELX_GEMM_STRASSEN_MIN"] = str(small if levels < 2 else small // 2)
        t = timeit(go, 3)
        used = L.lib().elx_gemm_last_levels()
        line += f"  levels {used}: {2 * m * n * k / t / 1e12:7.2f} TF ({t * 1e3:9.3f} ms)"
    print(line, flush=True)


if __name__ == "__main__":
    for spec in sys.argv[1:] or DEFAULT:
        d, ta, tb, m, n, k = spec.split(",")
        run(d, int(ta), int(tb), int(m), int(n), int(k))
