#!/usr/bin/env python3
"""Path-kernel rate of the Disney tier (kernel tier 5): scenes.random_spheres
at C2's camera with every sphere's material replaced by a Disney parameter
set of the same colour -- Lambertian -> the default set, Metal -> metallic 1
with roughness = fuzz, Dielectric -> spec_trans 1 with its ior -- the ground
and the three big spheres included.  Prints one JSON object and writes it to
the path given (default profiles/r17/disney.json).  New ground: the number is
recorded, not asserted.

Usage: python scripts/disney_rate.py [spp] [reps] [out.json]"""
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("raytracer-2025_amd")
capi = importlib.import_module("raytracer-2025_amd.capi")
rt = importlib.import_module("raytracer-2025_amd.raytracer")
scenes = importlib.import_module("raytracer-2025_amd.scenes")

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r17", "disney.json")


def disney_spheres(scene, image_width, samples_per_pixel):
    """scenes.random_spheres with Disney materials: (world, cam)."""
    data = scenes.load_random_spheres()
    objs = scene.Hittables()
    mats = {}
    for s in data["spheres"]:
        m = s["material"]
        key = json.dumps(m, sort_keys=True)
        if key not in mats:
            tex = scene.SolidColor(m["albedo"])
            if m["type"] == "lambertian":
                mats[key] = scene.Disney(tex)
            elif m["type"] == "metal":
                mats[key] = scene.Disney(tex, metallic=1.0, roughness=max(m["fuzz"], 0.05))
            else:
                mats[key] = scene.Disney(tex, spec_trans=1.0, ior=m["ior"], roughness=0.05)
        objs.add(scene.Sphere(s["center"], s["radius"], mats[key]))
    world = scene.Hittables()
    world.add(scene.BVH(objs))
    _, _, cam = scenes.random_spheres(scene, image_width, samples_per_pixel, spheres=1)  # C2's camera and sky
    return world, cam


torch.cuda.init()
api = pkg.load()
scene = rt.Scene(api)
world, cam = disney_spheres(scene, 1920, spp)
info = capi.RtWorldInfo()
api.check(api.world_info_get(scene.s, world.h, -1, cam.background.h, 0, ctypes.byref(info)))
assert info.kernel_tier == 5, info.kernel_tier
lin, _, st = cam.render(world, None, seed=1, want_srgb=False)  # warm-up
times, panics = [], int(st.panics)
for _ in range(reps):
    lin, _, st = cam.render(world, None, seed=1, want_srgb=False)
    times.append(st.kernel_ms)
    print("kernel_ms", st.kernel_ms, file=sys.stderr, flush=True)
res = {"workload": "random_spheres (C2 camera, 1920 x 1080), every material a Disney set", "spp": spp,
       "kernel_tier": int(info.kernel_tier), "kernel_ms": times, "kernel_ms_min": min(times),
       "msamples_per_s": cam.traced_samples() / (min(times) * 1e-3) / 1e6, "rays": int(st.rays), "panics": panics,
       "mean_radiance": float(lin.mean())}
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
