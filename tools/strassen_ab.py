"""Plain kernel, one Strassen-Winograd level and the library's default, in one process.

  python tools/strassen_ab.py [dt,ta,tb,m,n,k ...]

elx_gemm_{f64,f32} on device buffers, Uniform(-0.5, 0.5) operands, alpha = 0.5, beta =
-0.5.  The knobs are read at every call, so the three forms alternate on the
same buffers: ELX_GEMM_STRASSEN=0; =1 with ELX_GEMM_STRASSEN_MIN at the shape's
smallest dimension where that is below the default (so the crossover shows);
and no knob at all, which is up to two levels under the default thresholds.
Three timings each: the best, and the spread of the three in brackets, which is
what a difference between two forms has to exceed; rates are effective (2mnk /
time).  A shape whose default comes out at one level must match the one-level
form: the rule does not over-split.  The default shapes are the cubes around
the crossover, the large shapes of bench.py's points and the thin-k panels the
multi-GPU runs launch.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from elemental_amd import _lib as L
from gemm_bench import TD, timeit

DEFAULT = ["f64,0,0,4096,4096,4096", "f64,0,0,8192,8192,8192", "f64,0,0,12288,12288,12288",
           "f64,0,0,16384,16384,16384", "f64,0,0,32768,32768,32768", "f64,0,0,32768,32768,8192",
           "f64,0,0,65536,65536,8192", "f64,0,0,32768,16384,8192",
           "f64,1,0,16384,16384,16384", "f32,0,0,8192,8192,8192", "f32,0,0,16384,16384,16384",
           "f32,0,0,32768,32768,8192", "f32,1,0,8192,8192,524288"]
KNOBS = ("ELX_GEMM_STRASSEN", "ELX_GEMM_STRASSEN_MIN", "ELX_GEMM_STRASSEN_MIN2")


def run(dt, ta, tb, m, n, k):
    tdt = TD[dt]
    lda, ldb = (k if ta else m), (n if tb else k)
    A = torch.rand(lda * (m if ta else k), dtype=torch.float32, device="cuda").sub_(0.5).to(tdt)
    B = torch.rand(ldb * (k if tb else n), dtype=torch.float32, device="cuda").sub_(0.5).to(tdt)
    C = torch.rand(m * n, dtype=torch.float32, device="cuda").sub_(0.5).to(tdt)
    fn = L.lib().elx_gemm_f64 if dt == "f64" else L.lib().elx_gemm_f32
    go = lambda: L.check(fn(ta, tb, m, n, k, 0.5, A.data_ptr(), lda, B.data_ptr(), ldb, -0.5, C.data_ptr(), m, None))
    small = min(m, n, k)
    forms = [("plain", {"ELX_GEMM_STRASSEN": "0"}),
             ("one", {"ELX_GEMM_STRASSEN": "1", "ELX_GEMM_STRASSEN_MIN": str(min(small, 8192))}),
             ("default", {})]
    line = f"{dt} {'T' if ta else 'N'}{'T' if tb else 'N'} {m}x{n}x{k}:"
    for name, env in forms:
        for key in KNOBS:
            os.environ.pop(key, None)
        os.environ.update(env)
        ts = [timeit(go, 1) for _ in range(3)]
        used = L.lib().elx_gemm_last_levels()
        t = min(ts)
        line += (f"  {name} (levels {used}): {2 * m * n * k / t / 1e12:7.2f} TF "
                 f"({t * 1e3:9.3f} ms, spread {(max(ts) - t) * 1e3:6.3f})")
    print(line, flush=True)


if __name__ == "__main__":
    for spec in sys.argv[1:] or DEFAULT:
        d, ta, tb, m, n, k = spec.split(",")
        run(d, int(ta), int(tb), int(m), int(n), int(k))
