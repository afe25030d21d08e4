"""The basic tier's conservative f32 sphere filter
(raytracer-2025_amd/csrc/rt_sphere_filter.h, the same source the gfx950
kernel compiles) against the exact f64 Sphere::hit (sphere.rs:77-96) on CPU:
millions of random and adversarial (ray, sphere, bound) triples -- origins on
the sphere's surface and a hair off it, tangent rays, rays aimed at the rim,
the book-1 ground sphere (r = 1000), tiny and far spheres, |d| over four
decades, bounds right at the exact root.  The filter may only reject spheres
whose exact hit is absent or beyond the bound, and may only lower the bound to
a value >= the exact hit (tests/cpp/filter_prop.cpp).  Built twice: without
FMA contraction, as the kernel is built (-ffp-contract=off; the filter's own
fmaf calls stay), and with it, so the property does not hang on that flag.
The same cases run on the device in tests/test_walk_filters_gpu.py."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")


def build(contract, rcp=""):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "filter_prop_%s%s.%d" % (contract, rcp, os.getpid()))  # one per pytest worker
    exact = os.path.join(BUILD, "sphere_exact.o")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-c", os.path.join(HERE, "cpp", "sphere_exact.cpp"),
                    "-o", exact], check=True)
    flags = ["-mfma", "-ffp-contract=fast"] if contract == "fast" else ["-ffp-contract=off"]
    if rcp:  # the hardware reciprocal of RT_RCP_F32 = 2, emulated an ulp up / down (rt_slab.h rcp_f32)
        flags += ["-DRT_RCP_F32=2", "-DRT_RCP_EMU=%d" % (1 if rcp == "up" else -1)]
    subprocess.run(["g++", "-O2", "-std=c++17", *flags, os.path.join(HERE, "cpp", "filter_prop.cpp"), exact, "-o", exe],
                   check=True)
    return exe


@pytest.mark.parametrize("rcp", ["", "up", "down"])
@pytest.mark.parametrize("contract", ["fast", "off"])
@pytest.mark.parametrize("seed", [2025, 7])
def test_filter_is_conservative(contract, seed, rcp):
    exe = build(contract, rcp)
    r = subprocess.run([exe, "1500000", str(seed)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:]
    n, rejected, lowered, bad = map(int, r.stdout.strip().split("\n")[-1].split())
    assert bad == 0
    # the filter does decide: a large share of the cases is rejected or bounded
    assert rejected > n // 10 and lowered > n // 50
