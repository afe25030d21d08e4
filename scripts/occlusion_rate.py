#!/usr/bin/env python3
"""Occlusion-query throughput beside the hit query's (GPU box): for C2 and the
C4 terrain, as scripts/hit_rate.py builds them, two device-resident ray sets of
1920 x 1080 rays each --
  primary: the frame's pixel-centre rays, t_max = inf;
  ao:      from each primary hit's p (the records of one rt_world_hit_device
           call), one cosine-weighted direction about the record's normal
           (numpy.random.default_rng(2025)), t_max = inf; misses dropped and
           the set cycled up to the primary set's length
-- through rt_world_hit_device and rt_world_occluded_device in one process on
the same arrays: windows of `reps` back-to-back queries after a warm-up, timed
with HIP events, `rounds` windows each, alternating between the two calls.
Before any timing the occlusion bytes must equal the records' RT_HIT_FOUND on
every ray of every set.  Prints one JSON document: per set the tier, the
occluded fraction, ms per query of each call (all windows), Mrays/s best and
median, the ratio of the medians, and whether the occlusion query's median is
no slower than the hit query's beyond the hit query's own window spread.
python scripts/occlusion_rate.py [reps] [rounds] [terrain cells]"""
import ctypes
import importlib
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("raytracer-2025_amd")
capi = importlib.import_module("raytracer-2025_amd.capi")
rt = importlib.import_module("raytracer-2025_amd.raytracer")
scenes = importlib.import_module("raytracer-2025_amd.scenes")


def primary_rays(cam):
    """Camera::initilize's frame (camera.rs:204-245) and the ray through each pixel centre."""
    W, H = cam.image_width, cam.image_height
    lf, la, up = (np.array(v, dtype=np.float64) for v in (cam.look_from, cam.look_at, cam.vec_up))
    focus = float(cam.focus_distance)
    vh = 2.0 * math.tan(math.radians(cam.vertical_fov_in_degrees) / 2.0) * focus
    vw = vh * W / H
    w = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    du, dv = vw * u / W, -vh * v / H
    corner = lf - focus * w - vw * u / 2.0 + vh * v / 2.0
    i, j = np.meshgrid(np.arange(W), np.arange(H))
    px = corner + (i.reshape(-1, 1) + 0.5) * du + (j.reshape(-1, 1) + 0.5) * dv
    rays = np.zeros((W * H, 8))
    rays[:, 0:3] = lf
    rays[:, 3:6] = px - lf
    rays[:, 7] = np.inf
    return rays


def ao_rays(rec, n, rng):
    """One cosine-weighted direction about the normal of each hit of `rec`,
    from the hit's p; misses dropped, cycled up to n rays."""
    hit = (rec["flags"] & 1) != 0
    p, nrm = rec["p"][hit], rec["normal"][hit]
    # an orthonormal basis about the normal: the axis it is least along, crossed in
    k = np.argmin(np.abs(nrm), axis=1)
    a = np.zeros_like(nrm)
    a[np.arange(len(nrm)), k] = 1.0
    t = np.cross(a, nrm)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    r1, r2 = rng.random(len(nrm)), rng.random(len(nrm))
    phi, s = 2.0 * math.pi * r1, np.sqrt(r2)
    d = (np.cos(phi) * s)[:, None] * t + (np.sin(phi) * s)[:, None] * b + np.sqrt(1.0 - r2)[:, None] * nrm
    rays = np.zeros((len(p), 8))
    rays[:, 0:3], rays[:, 3:6], rays[:, 7] = p, d, np.inf
    return np.ascontiguousarray(rays[np.arange(n) % len(rays)])


class Bound:
    """A workload on one library: its scene, world and tier, and the two
    queries from device arrays."""

    def __init__(self, api, build):
        self.api = api
        self.scene = rt.Scene(api)
        self.world, _, self.cam = build(self.scene)
        info = capi.RtWorldInfo()
        api.check(api.world_info_get(self.scene.s, self.world.h, -1, -1, 0, ctypes.byref(info)))
        self.tier = int(info.kernel_tier)

    def hit(self, d_rays, n, d_out):
        self.scene.hit_device(self.world, d_rays.data_ptr(), n, d_out.data_ptr())

    def occluded(self, d_rays, n, d_out):
        self.scene.occluded_device(self.world, d_rays.data_ptr(), n, d_out.data_ptr())


def device_sets(bound):
    """{"primary", "ao"} -> (device rays, n, the records' FOUND as a numpy array) of a workload."""
    rays = primary_rays(bound.cam)
    n = len(rays)
    d_rec = torch.zeros(n * 80, dtype=torch.uint8, device="cuda")
    sets = {}
    for name in ("primary", "ao"):
        if name == "ao":
            rays = ao_rays(rec, n, np.random.default_rng(2025))
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
        bound.hit(d_rays, n, d_rec)  # (the first call flattens and uploads the world)
        torch.cuda.synchronize()
        rec = d_rec.cpu().numpy().view(rt.HIT_DTYPE).copy()
        sets[name] = (d_rays, n, ((rec["flags"] & 1) != 0).astype(np.uint8))
    return sets


def check_bytes(bound, d_rays, n, found):
    """The occlusion bytes of a set equal the records' RT_HIT_FOUND on every ray."""
    d_occ = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    bound.occluded(d_rays, n, d_occ)
    torch.cuda.synchronize()
    got = d_occ.cpu().numpy()
    assert np.array_equal(got, found), "%d occlusion bytes differ from the records' RT_HIT_FOUND" % int((got != found).sum())


def windows(calls, reps, rounds):
    """`rounds` windows of `reps` back-to-back calls of each of `calls`
    ({name: callable}), alternating between them; ms per call of every window."""
    for fn in calls.values():
        fn()  # warm-up: the kernel's code object
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    return ms


def rate(n, ms):
    return {"ms_per_query": [round(x, 4) for x in ms], "mrays_per_s_best": round(n / min(ms) / 1e3, 1),
            "mrays_per_s_median": round(n / float(np.median(ms)) / 1e3, 1)}


def workloads(cells):
    terrain = scenes.write_terrain_obj(tempfile.mkdtemp(prefix="occlusion_rate_"), cells)
    return [("C2 random spheres 1920x1080", lambda s: scenes.random_spheres(s, 1920, 1)),
            ("C4 OBJ terrain (%d triangles) 1920x1080" % (2 * cells * cells),
             lambda s: scenes.obj_terrain(s, terrain, 1920, 1))]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    cells = int(sys.argv[3]) if len(sys.argv) > 3 else 707
    assert torch.cuda.is_available(), "occlusion_rate.py measures on the GPU: there is no CPU fallback"
    torch.cuda.set_device(0)
    api = pkg.load()
    results = []
    for label, build in workloads(cells):
        bound = Bound(api, build)
        sets = device_sets(bound)
        for d_rays, n, found in sets.values():
            check_bytes(bound, d_rays, n, found)
        for name, (d_rays, n, found) in sets.items():
            d_rec = torch.zeros(n * 80, dtype=torch.uint8, device="cuda")
            d_occ = torch.zeros(n, dtype=torch.uint8, device="cuda")
            ms = windows({"hit": lambda: bound.hit(d_rays, n, d_rec), "occluded": lambda: bound.occluded(d_rays, n, d_occ)},
                         reps, rounds)
            hit_med, occ_med = float(np.median(ms["hit"])), float(np.median(ms["occluded"]))
            spread = max(ms["hit"]) - min(ms["hit"])
            results.append({"workload": label, "set": name, "kernel_tier": bound.tier, "rays": n,
                            "occluded_fraction": round(float(found.mean()), 4), "queries_per_window": reps,
                            "hit": rate(n, ms["hit"]), "occluded": rate(n, ms["occluded"]),
                            "median_ratio_hit_over_occluded": round(hit_med / occ_med, 3),
                            "hit_window_spread_ms": round(spread, 4),
                            "occluded_not_slower_beyond_spread": bool(occ_med <= hit_med + spread)})
            print(label, name, results[-1]["median_ratio_hit_over_occluded"], file=sys.stderr, flush=True)
    print(json.dumps({"what": "rt_world_hit_device and rt_world_occluded_device on the same device arrays, HIP events "
                              "around windows of back-to-back queries, alternating",
                      "device": torch.cuda.get_device_name(0), "results": results}, indent=1))


if __name__ == "__main__":
    main()
