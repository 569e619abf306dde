"""El::Trmm without a GPU: the distributed driver on Device::CPU matrices over
gloo, the kernel's k-range plan (host code), and the drop-in C++ surface."""
import os
import random
import shutil
import socket
import subprocess

import pytest
import torch.multiprocessing as mp

import _trmm_workers as TW
from elemental_amd import _lib as L
from elemental_amd import el

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    """A free rendezvous port below the kernel's ephemeral range (see test_dist_cpu)."""
    for _ in range(200):
        p = random.randrange(20000, 32000)
        s = socket.socket()
        try:
            s.bind(("127.0.0.1", p))
            return p
        except OSError:
            continue
        finally:
            s.close()
    raise RuntimeError("no free port in 20000-32000")


@pytest.mark.parametrize("world,height", [(1, 1), (2, 1), (4, 2), (8, 2)])
def test_trmm(world, height):
    """El::Trmm LEFT/RIGHT x LOWER/UPPER x N/T x NON_UNIT/UNIT, ragged blocks
    (m = 19, n = 13, nb = 4), A's unread part NaN, against numpy."""
    mp.spawn(TW.trmm_worker, args=(world, _port(), height, el.CPU, el.F64, 19, 13, 4, 31), nprocs=world, join=True)


def test_trmm_krange_plan(tmp_path):
    """trmm_tri's k range per row tile (kernels.hpp trmm_krange) covers the
    triangle, stays within a slab and a tile of it, and walks at most 0.6 of the
    full product's slabs at m = 4096: host-only code against the HIP headers."""
    gxx = shutil.which("g++")
    if gxx is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("no g++ / HIP headers")
    exe = tmp_path / "test_trmm_plan"
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-I", os.path.join(ROOT, "elemental_amd", "csrc", "kernels"),
                           os.path.join(ROOT, "tests", "cpp", "test_trmm_plan.cpp"), "-o", str(exe)])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]


def test_cpp_trmm_api(tmp_path):
    """El::Trmm on DistMatrix and Matrix and El::LocalTrmm through include/El.hpp,
    Device::CPU, against a hand-computed 3 x 3 case."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "test_trmm_api"
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.check_call([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_trmm_api.cpp"), "-o", str(exe), "-L", libdir,
                           "-lelemental_amd", f"-Wl,-rpath,{libdir}"])
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "OK" in res.stdout
