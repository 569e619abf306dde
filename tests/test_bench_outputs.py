"""bench.py --dump-outputs and the plain / --full split of the line.

On CPU: the sampled tiles are a function of the shape alone, and dump_outputs
writes exactly the matrix (whole, or those tiles) for every storage type, here
from CPU-device DistMatrices.  On the GPU: one plain run of bench.py itself at a
small size, whose line carries the headline fields and none of the --full
stages, and whose C.npy is the C of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

T = bench.DUMP_TILE


def test_dump_tiles_depend_on_the_shape_alone():
    m, n = 5000, 3001
    tiles = bench.dump_tiles(m, n)
    assert tiles == bench.dump_tiles(m, n)
    assert len(tiles) == bench.DUMP_TILES and tiles[0] == (0, 0) and tiles[1] == (m - T, n - T)
    assert all(0 <= i <= m - T and 0 <= j <= n - T for i, j in tiles)
    assert len(set(tiles)) > bench.DUMP_TILES // 2
    assert bench.DUMP_TILES * T * T * 8 <= 64 << 20 and bench.DUMP_WHOLE_BYTES <= 64 << 20


# whole (<= 32 MiB) and sampled (> 32 MiB) outputs; heights and widths that are
# no multiple of the tile
@pytest.mark.parametrize("dtype,fmt,m,n", [(el.F64, "f64", 300, 257), (el.F64, "f64", 2300, 2100),
                                           (el.F32, "f32", 3000, 2900), (el.BF16, "bf16", 700, 300),
                                           (el.F16, "f16", 200, 100)])
def test_dump_outputs_writes_the_matrix(tmp_path, dtype, fmt, m, n):
    g = el.Grid()
    C = el.DistMatrix(g, dtype, el.MC, el.MR, el.CPU, height=m, width=n).fill_hash(3, 0.0, 0.1)
    want = C.get_local()
    want = oracle.bf16_bits_to_f32(want) if fmt == "bf16" else want
    bench.dump_outputs(el, g, dtype, C, str(tmp_path / "out"))
    got = np.load(tmp_path / "out" / "C.npy")
    assert got.dtype == (np.float64 if fmt == "f64" else np.float32)
    assert got.nbytes <= 64 << 20
    if m * n * got.dtype.itemsize <= bench.DUMP_WHOLE_BYTES:
        assert got.shape == (m, n) and np.array_equal(got, want.astype(got.dtype))
    else:
        assert got.shape == (bench.DUMP_TILES, T, T)
        for tile, (i, j) in zip(got, bench.dump_tiles(m, n)):
            assert np.array_equal(tile, want[i:i + T, j:j + T].astype(got.dtype)), (i, j)


N, STEPS, WARMUP = 2320, 1, 1  # 2320^2 doubles > 32 MiB: the sampled path; no multiple of 128


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("bench_out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--n", str(N), "--steps",
                        str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=200)
    assert p.returncode == 0, p.stdout + p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr, out


@pytest.mark.gpu
def test_gpu_bench_plain_line(plain_run):
    """A plain run: the headline fields, `steps` timed steps, and no stage beside
    init / warmup / timed / dump / report."""
    rec, err, _ = plain_run
    assert rec["value"] > 0 and rec["unit"] == "TFLOP/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f64" and rec["metric"] == bench.METRIC and rec["steps"] == STEPS
    # value and ms_per_step are the same measurement
    assert rec["ms_per_step"] > 0
    assert abs(2.0 * N ** 3 / (rec["ms_per_step"] * 1e-3) / 1e12 - rec["value"]) <= 0.02 * rec["value"] + 1e-3
    for key in ("verify", "residual", "cpu_baseline", "c3_1gpu", "c4_1gpu", "c5_1gpu", "c1_1gpu"):
        assert key not in rec
    for name in ("verify", "cpu_baseline", "residual"):
        assert f"stage {name}" not in err


@pytest.mark.gpu
def test_gpu_bench_dump_is_the_last_timed_steps_output(plain_run):
    """C.npy holds the sampled tiles of C after WARMUP + STEPS steps of
    C := 0.5 A B - 0.5 C on the hash inputs.  Per tile the north_star ratio
    ||C - Cref||_F / (||A_rows||_F ||B_cols||_F k eps) against a float64
    product; one El::Gemm is held to 10 elsewhere in the suite, and the second
    step halves the first step's error and adds its own, hence 15."""
    _, _, out = plain_run
    got = np.load(out / "C.npy")
    assert got.dtype == np.float64 and got.shape == (bench.DUMP_TILES, T, T)
    A = oracle.hash_matrix(N, N, 1, 0.0, 0.1)
    B = oracle.hash_matrix(N, N, 2, 0.0, 0.1)
    C = oracle.hash_matrix(N, N, 3, 0.0, 0.1)
    AB = A @ B
    for _ in range(WARMUP + STEPS):
        C = 0.5 * AB - 0.5 * C
    eps = np.finfo(np.float64).eps
    worst = max(oracle.parity_ratio(tile, C[i:i + T, j:j + T], A[i:i + T, :], B[:, j:j + T], N, eps)
                for tile, (i, j) in zip(got, bench.dump_tiles(N, N)))
    print(f"worst tile parity ratio {worst:.3g}")
    assert worst <= 15
