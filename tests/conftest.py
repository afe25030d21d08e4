import ctypes
import importlib
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "raytracer-2025_amd"
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (gfx950) GPU")


def pkg_module(name=""):
    return importlib.import_module(PKG + ("." + name if name else ""))


def _make(path):
    subprocess.run(["make", "-j", "4", "-C", path], check=True, stdout=subprocess.DEVNULL)


@pytest.fixture(scope="session")
def capi():
    return pkg_module("capi")


@pytest.fixture(scope="session")
def rt():
    return pkg_module("raytracer")


@pytest.fixture(scope="session")
def scenes():
    return pkg_module("scenes")


@pytest.fixture(scope="session")
def oracle(capi):
    """The TEST-ONLY CPU oracle (oracle/), as the checker."""
    so = os.path.join(ROOT, "oracle", "_build", "liboracle.so")
    _make(os.path.join(ROOT, "oracle"))
    return capi.Api(ctypes.CDLL(so), "orc_", capi.ORACLE_EXTRAS)


@pytest.fixture(scope="session")
def oracle_cr(capi):
    """The oracle with its path libm calls on rt_crmath.h (liboracle_cr.so):
    isolates everything but glibc's own misroundings."""
    so = os.path.join(ROOT, "oracle", "_build", "liboracle_cr.so")
    _make(os.path.join(ROOT, "oracle"))
    return capi.Api(ctypes.CDLL(so), "orc_", capi.ORACLE_EXTRAS)


@pytest.fixture(scope="session")
def product():
    """librt_mi355x.so through the package loader (fails loudly when missing)."""
    pkg = pkg_module()
    if not os.path.exists(pkg.LIB_PATH):
        _make(os.path.join(ROOT, PKG))
    return pkg.load()


@pytest.fixture(scope="session")
def gpu(product):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return product


@pytest.fixture(scope="session")
def rccl_standin(tmp_path_factory):
    """The test-only RCCL stand-in (tests/cpp/fake_rccl.cpp: librccl's
    point-to-point subset over hipMemcpyPeerAsync, any number of ranks per
    device), built for this run (host code, g++ against the HIP runtime).
    Returns (path of the .so, counts()) -- counts() = (copies, bytes) so far
    in this process.  Only the check build loads it (RT_RCCL_LIB)."""
    src = os.path.join(ROOT, "tests", "cpp", "fake_rccl.cpp")
    so = str(tmp_path_factory.mktemp("standin") / "libfake_rccl.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    src, "-o", so, "-L/opt/rocm/lib", "-lamdhip64", "-pthread"], check=True, timeout=120)
    lib = ctypes.CDLL(so)
    lib.fake_rccl_counts.argtypes = [ctypes.POINTER(ctypes.c_uint64)]

    def counts():
        out = (ctypes.c_uint64 * 2)()
        lib.fake_rccl_counts(out)
        return int(out[0]), int(out[1])
    return so, counts


_LIBC = ctypes.CDLL(None, use_errno=True)
ADDR_NO_RANDOMIZE = 0x0040000  # <sys/personality.h>


def no_aslr():
    """preexec_fn of a sanitized test program: address-space randomisation off
    for that child alone (personality(2), what `setarch -R` does).  Under a
    kernel with 32 bits of mmap randomisation (vm.mmap_rnd_bits) a mapping can
    land outside the ranges the sanitizer runtimes of gcc 11 lay their shadow
    over, and the program ends before main with "FATAL: ThreadSanitizer:
    unexpected memory mapping".  Where the call is not allowed the child runs
    as it is."""
    cur = _LIBC.personality(0xffffffff)
    if cur != -1:
        _LIBC.personality(cur | ADDR_NO_RANDOMIZE)


def rmse_per_channel(a, b):
    import numpy as np

    d = a.astype(np.float64) - b.astype(np.float64)
    return np.sqrt((d ** 2).reshape(-1, 3).mean(axis=0))


def divergence(g, o, rel=1e-9):
    """Fraction of (pixel, stratum row) f64 sums whose paths diverged: the GPU
    runs ray_color as a loop (beta * L) and the oracle as the reference's
    recursion, so equal paths agree to ~1e-15 relative; a sample that took
    another branch (a transcendental or contraction ulp flipping a comparison)
    moves its row sum by orders of magnitude more.  g, o: (..., 3) arrays."""
    import numpy as np

    g = np.asarray(g, dtype=np.float64).reshape(-1, 3)
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3)
    bad = np.any(np.abs(g - o) > rel * np.maximum(1.0, np.abs(o)), axis=1)
    return float(bad.mean()) if bad.size else 0.0
