#!/usr/bin/env python3
"""Hit-query throughput (GPU box): the primary rays of the C2 and C4 frames
(1920x1080, one ray a pixel through its centre, no defocus) through
rt_world_hit_device from device arrays, timed with HIP events around `reps`
back-to-back queries after a warm-up query (the first call flattens and
uploads the world; the warm-up also loads the kernel's code object).  Prints
one JSON document: per workload the kernel tier, the rays, the hit fraction and
Mrays/s (best and median of `rounds` timed windows).
python scripts/hit_rate.py [reps] [rounds] [terrain cells]"""
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

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cells = int(sys.argv[3]) if len(sys.argv) > 3 else 707
assert torch.cuda.is_available(), "hit_rate.py measures on the GPU: there is no CPU fallback"
torch.cuda.set_device(0)
api = pkg.load()


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


def measure(label, build):
    scene = rt.Scene(api)
    world, _, cam = build(scene)
    info = capi.RtWorldInfo()
    api.check(api.world_info_get(scene.s, world.h, -1, -1, 0, ctypes.byref(info)))
    rays = primary_rays(cam)
    n = len(rays)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).cuda()
    d_out = torch.zeros(n * 80, dtype=torch.uint8, device="cuda")
    scene.hit_device(world, d_rays.data_ptr(), n, d_out.data_ptr())  # warm-up: flatten, upload, code object
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            scene.hit_device(world, d_rays.data_ptr(), n, d_out.data_ptr())
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    rec = d_out.cpu().numpy().view(rt.HIT_DTYPE)
    return {"workload": label, "kernel_tier": int(info.kernel_tier), "bvh_nodes": int(info.bvh_nodes),
            "primitives": int(info.primitives), "rays": n, "hit_fraction": round(float((rec["flags"] & 1).mean()), 4),
            "queries_per_window": reps, "ms_per_query": [round(x, 4) for x in ms],
            "mrays_per_s_best": round(n / min(ms) / 1e3, 1), "mrays_per_s_median": round(n / float(np.median(ms)) / 1e3, 1)}


terrain = scenes.write_terrain_obj(tempfile.mkdtemp(prefix="hit_rate_"), cells)
out = {"what": "rt_world_hit_device, primary rays of the frame, device arrays, HIP events around the timed queries",
       "device": torch.cuda.get_device_name(0),
       "results": [measure("C2 random spheres 1920x1080", lambda s: scenes.random_spheres(s, 1920, 1)),
                   measure("C4 OBJ terrain (%d triangles) 1920x1080" % (2 * cells * cells),
                           lambda s: scenes.obj_terrain(s, terrain, 1920, 1))]}
print(json.dumps(out, indent=1))
