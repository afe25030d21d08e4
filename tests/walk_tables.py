"""TEST HARNESS: builds the CPU generators of the f32 walk filters
(tests/cpp/slab_prop.cpp, tests/cpp/filter_prop.cpp) with g++ and reads the
case tables their --dump mode writes.  The host build is the header's default
(RT_RCP_F32 = 2 with the correctly rounded quotient, no contraction)."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off"]
# doubles per dumped case; the first IN_W are rt_walk_selftest's input
SLAB_W, SLAB_IN = 17, 14
FILTER_W, FILTER_IN = 15, 12


def build(kind, outdir):
    """kind 'slab' or 'filter'; returns the generator's path."""
    exe = os.path.join(str(outdir), kind + "_prop")
    src = [os.path.join(HERE, "cpp", kind + "_prop.cpp")]
    if kind == "filter":
        obj = os.path.join(str(outdir), "sphere_exact.o")
        subprocess.run([*CXX, "-c", os.path.join(HERE, "cpp", "sphere_exact.cpp"), "-o", obj], check=True, timeout=120)
        src.append(obj)
    subprocess.run([*CXX, *src, "-o", exe], check=True, timeout=120)
    return exe


def run(exe, n, seed, dump=None):
    """The four numbers a run prints, and the dumped table (or None)."""
    cmd = [exe, str(n), str(seed)] + (["--dump", dump] if dump else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    counts = tuple(map(int, r.stdout.strip().split("\n")[-1].split()))
    table = None
    if dump:
        w = SLAB_W if os.path.basename(exe).startswith("slab") else FILTER_W
        table = np.fromfile(dump, dtype=np.float64).reshape(-1, w)
        os.remove(dump)
    return counts, table


def slab_counts(t):
    """(exact hits, host hits, violations) of a slab table."""
    ex, hit = t[:, 14] == 1, t[:, 15] == 1
    return int(ex.sum()), int(hit.sum()), int((ex & ~hit).sum())


def filter_verdict(t, keep, cf2):
    """(rejected, lowered, violations) of filter results on the table's cases:
    the three conditions of filter_prop.cpp."""
    cf, tx = t[:, 11], t[:, 12]
    ok = (cf2 <= cf) | (np.isnan(cf) & np.isnan(cf2))
    rej = keep == 0
    ok &= ~rej | (tx < 0) | (tx > cf)
    low = cf2 < cf
    ok &= ~low | ((tx >= 0) & (tx <= cf2))
    return int(rej.sum()), int(low.sum()), ~ok
