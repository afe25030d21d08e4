"""Shared by tests/test_world_scatter_cpu.py and tests/test_world_scatter_gpu.py:
the oracle's scatter-query driver (tests/cpp/scatter_oracle.cpp, built once per
process and flavour as tests/radiance_query.py builds its driver, which this
one includes), the worlds and ray sets of tests/radiance_query.py on it, and
the helpers that compare records bit for bit.

The records are numpy structured arrays of raytracer.SCATTER_DTYPE on both
sides; floats are compared as integers, field by field.
"""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT, pkg_module
import radiance_query as rq

_DP = C.POINTER(C.c_double)
_UP = C.POINTER(C.c_uint32)
RAY, PDF, NO_SAMPLE, EVAL, PANIC = 1, 2, 4, 8, 16
FLOAT_FIELDS = ("emitted", "f", "pdf", "origin", "dir", "eval_f", "eval_pdf")
HIT_FLOAT_FIELDS = ("t", "p", "normal", "u", "v")


@functools.lru_cache(maxsize=None)
def driver(crmath=True):
    """capi.Api of the oracle with the Disney and Portal materials, with
    orcx_world_scatter / orcx_world_radiance / orcx_first_hit bound as
    .x_world_scatter / .x_world_radiance / .x_first_hit (-DORC_CRMATH, or
    without it: glibc's libm)."""
    capi = pkg_module("capi")
    out = os.path.join(tempfile.mkdtemp(prefix="scatter_query_"), "libscatter_oracle%s.so" % ("_cr" if crmath else ""))
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off"] + (["-DORC_CRMATH"] if crmath else []) + \
          ["-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "scatter_oracle.cpp"),
           os.path.join(ROOT, "oracle", "rt_oracle.cpp"), os.path.join(ROOT, "oracle", "rt_oracle_obj.cpp"),
           "-pthread", "-lz"]
    subprocess.run(cmd, check=True, timeout=600)
    lib = C.CDLL(out)
    api = capi.Api(lib, "orc_", capi.ORACLE_EXTRAS)
    for name in ("orc_mat_portal", "orc_mat_disney", "orc_disney_params_default"):
        assert name not in api.missing, name
    fn = lib.orcx_world_scatter
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, _DP, _DP, _UP,
                   C.c_uint64, C.c_void_p]
    api.x_world_scatter = fn
    fn = lib.orcx_world_radiance
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _DP,
                   C.c_uint64, _DP]
    api.x_world_radiance = fn
    fn = lib.orcx_first_hit
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, _DP, C.c_uint64, _DP]
    api.x_first_hit = fn
    return api


def oracle_scatter(api, scene, world, rays, *, eval_dirs=None, indices=None, seed=rq.SEED, sample=0, vertex=1,
                   first_index=0, background=None):
    """orcx_world_scatter for an (n, 8) ray array, as Scene.scatter returns it."""
    rt = pkg_module("raytracer")
    a = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
    n = a.shape[0]
    e = None if eval_dirs is None else np.ascontiguousarray(eval_dirs, dtype=np.float64).reshape(n, 3)
    i = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32).reshape(n)
    out = np.zeros(n, dtype=rt.SCATTER_DTYPE)
    api.check(api.x_world_scatter(scene.s, world.h, -1 if background is None else background.h, int(seed), int(sample),
                                  int(vertex), int(first_index), a.ctypes.data_as(_DP),
                                  None if e is None else e.ctypes.data_as(_DP),
                                  None if i is None else i.ctypes.data_as(_UP), n, out.ctypes.data))
    return out


@functools.lru_cache(maxsize=None)
def oracle_world(name, crmath=True):
    """(scene, world, lights, cam, box) of a named world of radiance_query.WORLDS on this module's driver."""
    return rq.world_case(driver(crmath), name)


def bits(a):
    """A float array as the integers of its bits."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def differing_fields(got, want, hit_mat=False):
    """The fields of two SCATTER_DTYPE arrays that differ in any bit of any
    record -- name -> indices of the records -- floats compared as integers;
    hit.mat only when asked for."""
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = {}
    for k in FLOAT_FIELDS:
        d = bits(got[k]) != bits(want[k])
        d = d.reshape(len(got), -1).any(axis=1)
        if d.any():
            bad[k] = np.nonzero(d)[0]
    for k in HIT_FLOAT_FIELDS:
        d = (bits(got["hit"][k]) != bits(want["hit"][k])).reshape(len(got), -1).any(axis=1)
        if d.any():
            bad["hit." + k] = np.nonzero(d)[0]
    for k in ("flags", "draws"):
        d = got[k] != want[k]
        if d.any():
            bad[k] = np.nonzero(d)[0]
    d = got["hit"]["flags"] != want["hit"]["flags"]
    if d.any():
        bad["hit.flags"] = np.nonzero(d)[0]
    if hit_mat:
        d = got["hit"]["mat"] != want["hit"]["mat"]
        if d.any():
            bad["hit.mat"] = np.nonzero(d)[0]
    return bad


def report(label, got, want, bad):
    """Prints what differing_fields found, a few records a field."""
    print(f"{label}: {len(got)} records, fields that differ: { {k: len(v) for k, v in bad.items()} }")
    for k, idx in bad.items():
        for i in idx[:3]:
            g, w = (got, want) if "." not in k else (got["hit"], want["hit"])
            f = k.split(".")[-1]
            print(f"  {k}[{i}]: got {g[f][i]} want {w[f][i]} (flags {got['flags'][i]} / {want['flags'][i]})")


def same_bytes(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
