#!/usr/bin/env python3
"""Static ISA attribution of the basic tier's path kernel (C2) by phase.

Compiles csrc/rt_kernel_path.hip for tier 0 as the product does (gfx950, -O3, no
contraction, machine LICM off) with -DRT_ISA_MARKS -- an assembler comment at
each phase boundary of the loop (RT_ISA_MARK: fields, walk / walk_visit /
walk_sphere / walk_tail, park, miss, refill, draws, shade, camera) -- and
counts the instructions of rt_path_kernel<0, false> after each marker, in
layout order, by class: VALU (f64 / f32 / integer+other), SALU, vector
memory, LDS, scalar memory, branches, waits.  It also compiles the unmarked
kernel and reports both totals (the markers' effect on code generation).
A static count is the code of a phase, once; how often each runs is the
diagnostic build's business (scripts/diag.py).
  python scripts/isa_phases.py > profiles/r06/isa_phases_c2.json"""
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raytracer-2025_amd", "csrc", "rt_kernel_path.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
         "-mllvm", "-disable-machine-licm", "-DRT_TIER=0", "--offload-device-only", "-S"]
KERNEL = "_ZN3rtk14rt_path_kernelILi0ELb0EEEvPKNS_7KParamsE"


RESOURCES = {}  # of the last asm() call: kernel -> {vgprs, scratch_bytes_per_lane, waves_per_simd}


def asm(extra):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *extra, "-Rpass-analysis=kernel-resource-usage", "-o", out,
                            SRC], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        text = open(out).read()
    RESOURCES.clear()
    cur = None
    for ln in r.stderr.splitlines():  # the compiler's resource remarks, a block per kernel
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = RESOURCES.setdefault(m.group(2), {})
        elif cur is not None:
            cur[{"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
                 "Occupancy [waves/SIMD]": "waves_per_simd"}[m.group(1)]] = int(m.group(2))
    start = text.index(KERNEL + ":")
    end = text.index(".Lfunc_end", start)
    return text[start:end].splitlines()


def klass(op):
    if op.startswith(("v_cmp", "v_cndmask")) or op.startswith("v_") and op.endswith(("_f64", "_f64_e32", "_f64_e64")) is False:
        pass
    if op.startswith("v_"):
        if "_f64" in op:
            return "valu_f64"
        if "_f32" in op or "_f16" in op:
            return "valu_f32"
        return "valu_int_other"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "other"


def count(lines):
    phases = collections.OrderedDict()
    cur = "entry"
    total = 0
    for ln in lines:
        m = re.search(r";@@phase (\w+)", ln)
        if m:
            cur = m.group(1)
            continue
        t = ln.strip()
        if not t or t.startswith((";", ".")) or t.endswith(":"):
            continue
        op = t.split()[0]
        c = phases.setdefault(cur, collections.Counter())
        c[klass(op)] += 1
        c["all"] += 1
        total += 1
    return phases, total


def main():
    marked, total_m = count(asm(["-DRT_ISA_MARKS"]))
    _, total_p = count(asm([]))
    wide = KERNEL.replace("Lb0", "Lb1")  # rt_path_kernel<0, true>: trees past the batch variant's LDS node copy
    out = {
        "resources_product_build": {"rt_path_kernel<0, false>": dict(RESOURCES.get(KERNEL, {})),
                                    "rt_path_kernel<0, true>": dict(RESOURCES.get(wide, {}))},
        "kernel": "rt_path_kernel<0, false> (basic tier, 56-lane shading batches: C1 / C2)",
        "method": "static instruction counts in layout order after each RT_ISA_MARK comment (-DRT_ISA_MARKS); "
                  "a phase's count is its code once, not how often it runs",
        "total_instructions_marked_build": total_m,
        "total_instructions_product_build": total_p,
        "phases": {k: dict(v) for k, v in marked.items()},
    }
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
