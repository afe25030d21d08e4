"""The path kernel's work queue on CPU (raytracer-2025_amd/csrc/rt_queue.h, the
same text the gfx950 kernels compile: QueuePool, pool_take, pool_entry,
guided_chunk, queue_entry).  A wave keeps its pool of queue entries in scalar
registers, sizes a chunk only on the pass that takes one and decodes a pass
that lies in one region of the queue with that region's constants; none of
that may move an entry.  tests/cpp/pool_prop.cpp holds, on small frames (S of
1, 4 and 22 samples a stratum row; whole rows only, with parts, with fine
parts; 8, 64, 65 and several thousand entries; with and without the waves'
first pools taken without the counter; the launcher's chunk floor and cap and
small ones):

(a) 1 to 64 simulated waves with random need masks against one shared counter
    until all lanes have left: every entry below queue_total is handed out
    exactly once and none at or beyond it, each within the bounds its pass
    reports -- and each lane takes the entry, and the counter every add, that
    the per-lane hand-out before this change gave (kept in the program);
(b) queue_entry over all q tiles each item's [0, S) exactly once, in the order
    of the frame plan (rt_plan.h row_parts), under any bounds of the pass;
(c) guided_chunk equals its per-lane predecessor on a grid of (pool_end, avail,
    n) across every region border.

Built plain and with AddressSanitizer + UBSan (a stand-alone host program)."""
import os
import subprocess

import pytest

from conftest import no_aslr

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "_build")


def _build(sanitize):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "pool_prop%s.%d" % ("_asan" if sanitize else "", os.getpid()))
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] \
        if sanitize else ["-O2"]
    # (rt_plan.h reaches the HIP runtime's header through rt_layout.h: host declarations only)
    subprocess.run(["g++", *flags, "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(HERE, "cpp", "pool_prop.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("sanitize,seed", [(False, 2025), (False, 7), (True, 11)])
def test_every_entry_goes_out_once_in_the_order_it_did(sanitize, seed):
    exe = _build(sanitize)
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=300, preexec_fn=no_aslr)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    frames, passes, entries, chunk_cases = map(int, r.stdout.strip().split("\n")[-1].split())
    # 14 frame shapes x 6 wave counts x with / without static pools, every entry of each handed out
    assert frames == 14 * 6 * 2
    assert entries > 300000 and passes > 10000 and chunk_cases > 100000
