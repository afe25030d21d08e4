"""The basic tier's sign-ordered f32 box test on CPU (raytracer-2025_amd/csrc/
rt_slab.h: RaySF, make_raysf, slab_sorted_f, the same text the gfx950 kernel's
visit4_rows compiles): the ray orders each axis' two planes once, by the sign
of 1/d, and a node visit computes the six plane distances of slab_f without
its per-axis min / max.  tests/cpp/slab_sorted_prop.cpp holds, with the
hardware reciprocal emulated as the correctly rounded quotient and as that
quotient moved one ulp up and down (RT_RCP_EMU 0, +1, -1):

(a) conservative: every box hit that aabb.rs:62-78 in long double admits on
    the exact box within [t_min, c] is admitted;
(b) agreement with slab_f on the same ray: the same verdict in every case and,
    on a hit, the same entry distance bit for bit -- so the walk visits the
    same nodes in the same order.

Over 4 M random and adversarial cases a build: direction components +0, -0,
1e-40 and 1e-300, flat boxes, origins inside the box and on a face, edge or
corner, boxes wholly behind the origin, c finite, infinite and at the entry.
Built plain and with AddressSanitizer + UBSan (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import no_aslr

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")
CASES = 4000000


def _build(emu, sanitize):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "slab_sorted_prop_%d%s.%d" % (emu, "_asan" if sanitize else "", os.getpid()))
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] \
        if sanitize else ["-O2"]
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-DRT_SLAB_FOLD=1", "-DRT_RCP_F32=2",
                    "-DRT_RCP_EMU=%d" % emu, os.path.join(HERE, "cpp", "slab_sorted_prop.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("emu,sanitize,seed", [(0, False, 2025), (1, False, 2025), (-1, False, 2025), (0, False, 7),
                                               (0, True, 11)])
def test_sorted_slab_is_conservative_and_agrees_with_slab_f(emu, sanitize, seed):
    exe = _build(emu, sanitize)
    r = subprocess.run([exe, str(CASES), str(seed)], capture_output=True, text=True, timeout=300, preexec_fn=no_aslr)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    n, hits, fhits, inverted, not_conservative, disagreeing = map(int, r.stdout.strip().split("\n")[-1].split())
    # n counts the cases that ran both tests (a draw the program skips -- a
    # direction with no component normal in f32 -- is drawn again)
    assert n >= 4000000 and n == CASES
    assert not_conservative == 0 and disagreeing == 0
    assert hits > n // 5 and fhits >= hits
    # the pairing slab_f's min / max would have swapped does occur (slabs
    # behind the origin), so (b) is held where the two forms differ
    assert inverted > n // 1000
