#!/usr/bin/env python3
"""Path-kernel rate of the reference's mc.obj under its own MTL -- every
material a Disney BSDF (rt_wavefront_load_flags with RT_OBJ_DISNEY, kernel
tier 5) beneath the DiffuseLight / image-ratio Mix wrappers mc.mtl gives it --
at 1920 x 1080 and 64 spp, beside the same mesh under the vanilla metals of
tests/hit_query.py::world_mc_obj.  The mesh, the camera and the sky are the
"mc" fixture of tests/obj_disney_query.py.  The metal twin runs a lower tier
(no wrappers, no textures), so the ratio only says what the materials cost.
Prints one JSON object and writes it to the path given (default
profiles/r23/obj_disney_rate.json).  New ground: recorded, not asserted.

Usage: python scripts/obj_disney_rate.py [spp] [reps] [out.json]"""
import importlib
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
pkg = importlib.import_module("raytracer-2025_amd")
rt = importlib.import_module("raytracer-2025_amd.raytracer")
import hit_query as hq  # noqa: E402
import obj_disney_query as oq  # noqa: E402

spp = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "r23", "obj_disney_rate.json")

METAL_MTL = "".join("newmtl %s\nKd %g %g %g\nPm 1.0\nPr 0.3\n" % ((name,) + kd) for name, kd in hq.MC_KD.items())


def measure(api, disney):
    scene = rt.Scene(api)
    path = oq.write_mc(tempfile.mkdtemp(prefix="obj_disney_rate_"), None if disney else METAL_MTL)
    world = scene.Hittables()
    world.add(scene.Wavefont(path, True, disney=disney))
    cam = oq.mc_camera(rt, scene)
    cam.image_width, cam.samples_per_pixel = 1920, spp
    info = oq.world_info(api, scene, world, None, cam.background)
    lin, _, st = cam.render(world, None, seed=1, want_srgb=False)  # warm-up
    times, panics = [], int(st.panics)
    for _ in range(reps):
        lin, _, st = cam.render(world, None, seed=1, want_srgb=False)
        times.append(st.kernel_ms)
        print("disney" if disney else "metal", "kernel_ms", st.kernel_ms, file=sys.stderr, flush=True)
    times.sort()
    med = times[len(times) // 2]
    return {"kernel_tier": int(info.kernel_tier), "features": int(info.features), "primitives": int(info.primitives),
            "kernel_ms": times, "kernel_ms_median": med, "msamples_per_s": cam.traced_samples() / (med * 1e-3) / 1e6,
            "rays": int(st.rays), "panics": panics, "mean_radiance": float(lin.mean())}


torch.cuda.init()
api = pkg.load()
res = {"workload": "tests/golden/ref_assets/mc.obj (stone objects left out), 1920 x 1080, sky gradient, max_depth 10",
       "spp": spp, "disney_own_mtl": measure(api, True), "metal_twin": measure(api, False)}
res["kernel_ms_ratio_disney_over_metal"] = res["disney_own_mtl"]["kernel_ms_median"] / res["metal_twin"]["kernel_ms_median"]
print(json.dumps(res, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
