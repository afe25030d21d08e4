"""The benchmark scenes of BASELINE.json `configs`, built through the
reference-mirroring API (raytracer.py).  Each builder takes a `Scene` (on any
implementation of the ABI) and returns (world, lights, camera).

  C1  random_spheres(scene, 400, 100)     book-1 final scene, reference CPU size
  C2  random_spheres(scene, 1920, 512)    the headline benchmark (484 traced spp)
  C3  cornell_smoke(scene, 800, 1024)     reference cornell_box + a smoke box
  C4  obj_terrain(scene, path, 1920, 256) synthetic 1M-triangle OBJ (write_terrain_obj)
  C5  final_scene(scene, 3840, 4096, 40)  reference final_scene, aspect 16/9

Scene-construction randomness (the reference calls Random:: while building,
src/main.rs:395-400, 491-499) is drawn from SplitMix64(seed) here so every
implementation receives identical objects.
"""
import json
import os

from .raytracer import Camera, Quaternion

DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
MASK = (1 << 64) - 1


class SplitMix64:
    def __init__(self, seed):
        self.state = seed & MASK

    def next_u64(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & MASK
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
        return z ^ (z >> 31)

    def f64(self):
        return (self.next_u64() >> 11) * (1.0 / 9007199254740992.0)

    def range(self, lo, hi):
        return lo + (hi - lo) * self.f64()


def load_random_spheres():
    with open(os.path.join(DATA, "random_spheres_seed2025.json")) as f:
        return json.load(f)


def random_spheres(scene, image_width=400, samples_per_pixel=100, max_depth=None, spheres=None):
    """Book-1 random spheres: world = Hittables{ BVH::new(spheres) }."""
    data = load_random_spheres()
    objs = scene.Hittables()
    mats = {}
    sph = data["spheres"] if spheres is None else data["spheres"][:spheres]
    for s in sph:
        m = s["material"]
        key = json.dumps(m, sort_keys=True)
        if key not in mats:
            if m["type"] == "lambertian":
                mats[key] = scene.Lambertian(scene.SolidColor(m["albedo"]))
            elif m["type"] == "metal":
                mats[key] = scene.Metal(m["albedo"], m["fuzz"])
            else:
                mats[key] = scene.Dielectric(scene.SolidColor(m["albedo"]), m["ior"])
        objs.add(scene.Sphere(s["center"], s["radius"], mats[key]))
    world = scene.Hittables()
    world.add(scene.BVH(objs))
    c = data["camera"]
    cam = Camera()
    cam.aspect_ratio = c["aspect_ratio"]
    cam.image_width = image_width
    cam.samples_per_pixel = samples_per_pixel
    cam.max_depth = c["max_depth"] if max_depth is None else max_depth
    cam.vertical_fov_in_degrees = c["vertical_fov_in_degrees"]
    cam.look_from = tuple(c["look_from"])
    cam.look_at = tuple(c["look_at"])
    cam.vec_up = tuple(c["vec_up"])
    cam.defocus_angle_in_degrees = c["defocus_angle_in_degrees"]
    cam.focus_distance = c["focus_distance"]
    cam.background = scene.SkyGradient(data["sky"]["horizon"], data["sky"]["zenith"])
    return world, None, cam


def cornell_smoke(scene, image_width=800, samples_per_pixel=1024, max_depth=10, smoke=True):
    """src/main.rs:541-639 cornell_box(), plus (C3) a 165^3 smoke box rotated
    -18 deg about y at (130,0,65) as ConstantMedium::new_with_tex(box, 0.01,
    white) (volume.rs:23-33)."""
    api = scene.api
    red = scene.Lambertian(scene.SolidColor((0.65, 0.05, 0.05)))
    white = scene.Lambertian(scene.SolidColor((0.73, 0.73, 0.73)))
    green = scene.Lambertian(scene.SolidColor((0.12, 0.45, 0.15)))
    light = scene.DiffuseLight(scene.SolidColor((15.0, 15.0, 15.0)))
    world = scene.Hittables()
    world.add(scene.Quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green))
    world.add(scene.Quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red))
    world.add(scene.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), light))
    world.add(scene.Quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white))
    world.add(scene.Quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white))
    world.add(scene.Quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white))
    box1 = scene.build_box((0, 0, 0), (165, 330, 165), white)
    box1 = scene.Transform(box1, (265, 0, 295), Quaternion.from_axis_angle(api, (0, 1, 0), 15.0), None)
    world.add(box1)
    if smoke:
        box2 = scene.build_box((0, 0, 0), (165, 165, 165), white)
        box2 = scene.Transform(box2, (130, 0, 65), Quaternion.from_axis_angle(api, (0, 1, 0), -18.0), None)
        world.add(scene.ConstantMedium(box2, 0.01, scene.SolidColor((1.0, 1.0, 1.0))))
    lights = scene.Hittables()
    lights.add(scene.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), light))
    cam = Camera()
    cam.aspect_ratio = 1.0
    cam.image_width = image_width
    cam.samples_per_pixel = samples_per_pixel
    cam.max_depth = max_depth
    cam.vertical_fov_in_degrees = 40.0
    cam.look_from = (278.0, 278.0, -800.0)
    cam.look_at = (278.0, 278.0, 0.0)
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.defocus_angle_in_degrees = 0.0
    return world, lights, cam


def final_scene(scene, image_width=800, samples_per_pixel=5000, max_depth=40, aspect_ratio=1.0, seed=2025):
    """src/main.rs:384-539 final_scene.  The earth texture file is missing from
    the mount -> ImageTexture cyan fallback (texture.rs:167-169)."""
    api = scene.api
    g = SplitMix64(seed)
    boxes1 = scene.Hittables()
    ground = scene.Lambertian(scene.SolidColor((0.48, 0.83, 0.53)))
    for i in range(20):
        for j in range(20):
            w = 100.0
            x0 = -1000.0 + i * w
            z0 = -1000.0 + j * w
            y1 = g.range(1.0, 101.0)
            boxes1.add(scene.build_box((x0, 0.0, z0), (x0 + w, y1, z0 + w), ground))
    world = scene.Hittables()
    world.add(scene.Sphere((400, 200, 400), 100, scene.Lambertian(scene.ImageTexture(None))))
    world.add(scene.BVH(boxes1))
    light_mat = scene.DiffuseLight(scene.SolidColor((7, 7, 7)))
    world.add(scene.Quad((123, 554, 147), (300, 0, 0), (0, 0, 265), light_mat))
    world.add(scene.Sphere_new_with_motion((400, 400, 200), (430, 400, 200), 50,
                                           scene.Lambertian(scene.SolidColor((0.7, 0.3, 0.1)))))
    glass = scene.Dielectric(scene.SolidColor((1, 1, 1)), 1.5)
    world.add(scene.Sphere((260, 150, 45), 50, glass))
    world.add(scene.Sphere((0, 150, 145), 50, scene.Metal((0.8, 0.8, 0.9), 1.0)))
    world.add(scene.Sphere((360, 150, 145), 70, glass))
    boundary = scene.Sphere((360, 150, 145), 70, scene.EmptyMaterial())
    world.add(scene.ConstantMedium(boundary, 0.2, scene.SolidColor((0.2, 0.4, 0.9))))
    boundary = scene.Sphere((0, 0, 0), 5000, scene.EmptyMaterial())
    world.add(scene.ConstantMedium(boundary, 0.0001, scene.SolidColor((1, 1, 1))))
    world.add(scene.Sphere((220, 280, 300), 80, scene.Lambertian(scene.NoiseTexture(0.2, seed))))
    boxes2 = scene.Hittables()
    white = scene.Lambertian(scene.SolidColor((0.73, 0.73, 0.73)))
    for _ in range(1000):
        c = (g.range(0.0, 165.0), g.range(0.0, 165.0), g.range(0.0, 165.0))
        boxes2.add(scene.Sphere(c, 10, white))
    world.add(scene.Transform(scene.BVH(boxes2), (-100, 270, 395),
                              Quaternion.from_axis_angle(api, (0, 1, 0), 15.0), None))
    lights = scene.Hittables()
    lights.add(scene.Quad((123, 554, 147), (300, 0, 0), (0, 0, 265), scene.EmptyMaterial()))
    cam = Camera()
    cam.aspect_ratio = aspect_ratio
    cam.image_width = image_width
    cam.samples_per_pixel = samples_per_pixel
    cam.max_depth = max_depth
    cam.vertical_fov_in_degrees = 40.0
    cam.look_from = (478.0, 278.0, -600.0)
    cam.look_at = (278.0, 278.0, 0.0)
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.defocus_angle_in_degrees = 0.0
    return world, lights, cam


# ---------------------------------------------------------------- C4: synthetic OBJ mesh
TERRAIN_MTL = """# two vanilla materials (obj.rs:289-298): Pm 1 -> Metal(Kd, Pr)
newmtl chrome
Kd 0.8 0.85 0.9
Pm 1.0
Pr 0.15
newmtl gold
Kd 0.9 0.7 0.3
Pm 1.0
Pr 0.45
"""


def terrain_height(x, z):
    """Displacement of the C4 terrain and its analytic gradient."""
    import numpy as np

    h = 0.35 * np.sin(1.3 * x) * np.cos(1.1 * z) + 0.12 * np.sin(3.7 * x + 1.3) * np.sin(2.9 * z) \
        + 0.04 * np.cos(9.0 * x - 7.0 * z)
    hx = 0.35 * 1.3 * np.cos(1.3 * x) * np.cos(1.1 * z) + 0.12 * 3.7 * np.cos(3.7 * x + 1.3) * np.sin(2.9 * z) \
        - 0.04 * 9.0 * np.sin(9.0 * x - 7.0 * z)
    hz = -0.35 * 1.1 * np.sin(1.3 * x) * np.sin(1.1 * z) + 0.12 * 2.9 * np.sin(3.7 * x + 1.3) * np.cos(2.9 * z) \
        + 0.04 * 7.0 * np.sin(9.0 * x - 7.0 * z)
    return h, hx, hz


def write_terrain_obj(directory, cells=707, extent=4.0):
    """Writes terrain.obj + terrain.mtl: a (cells x cells)-quad displaced grid
    over [-extent, extent]^2 (2*cells^2 triangles; cells=707 -> 999 698), every
    corner `v/vt/vn` with one shared index, analytic vertex normals, texture
    coordinates (i/cells, j/cells).  Two objects (x < 0: `chrome`, x >= 0:
    `gold`) so the loader's per-model BVHs and usemtl handling are exercised.
    Deterministic: the same cells give the same bytes."""
    import numpy as np

    os.makedirs(directory, exist_ok=True)
    n = cells + 1
    g = np.linspace(-extent, extent, n)
    X, Z = np.meshgrid(g, g, indexing="ij")  # [i, j] -> (x_i, z_j)
    H, HX, HZ = terrain_height(X, Z)
    N = np.stack([-HX, np.ones_like(HX), -HZ], axis=-1)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    U, V = np.meshgrid(np.arange(n) / cells, np.arange(n) / cells, indexing="ij")
    obj = os.path.join(directory, "terrain.obj")
    with open(os.path.join(directory, "terrain.mtl"), "w") as f:
        f.write(TERRAIN_MTL)
    with open(obj, "w") as f:
        f.write("# synthetic C4 terrain: %d x %d cells, %d triangles\nmtllib terrain.mtl\n" % (cells, cells, 2 * cells * cells))
        np.savetxt(f, np.stack([X.ravel(), H.ravel(), Z.ravel()], 1), fmt="v %.6f %.6f %.6f")
        np.savetxt(f, np.stack([U.ravel(), V.ravel()], 1), fmt="vt %.6f %.6f")
        np.savetxt(f, N.reshape(-1, 3), fmt="vn %.6f %.6f %.6f")
        idx = np.arange(n * n).reshape(n, n) + 1  # 1-based
        a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
        half = cells // 2
        for name, sl in (("chrome", slice(0, half)), ("gold", slice(half, cells))):
            f.write("o terrain_%s\nusemtl %s\n" % (name, name))
            # two counter-clockwise (seen from +y) triangles per cell
            t1 = np.stack([a[sl], d[sl], c[sl]], -1).reshape(-1, 3)
            t2 = np.stack([a[sl], c[sl], b[sl]], -1).reshape(-1, 3)
            tris = np.stack([t1, t2], 1).reshape(-1, 3)
            np.savetxt(f, np.repeat(tris, 3, axis=1), fmt="f %d/%d/%d %d/%d/%d %d/%d/%d")
    return obj


def obj_terrain(scene, obj_path, image_width=1920, samples_per_pixel=256, max_depth=50):
    """C4: world = Hittables{ Wavefont(terrain.obj) (one BVH per
    model), a glass and a diffuse sphere }, sky background."""
    world = scene.Hittables()
    world.add(scene.Wavefont(obj_path, True))
    world.add(scene.Sphere((-0.9, 1.0, 0.6), 0.45, scene.Dielectric(scene.SolidColor((1.0, 1.0, 1.0)), 1.5)))
    world.add(scene.Sphere((1.1, 0.95, -0.3), 0.4, scene.Lambertian(scene.SolidColor((0.7, 0.2, 0.15)))))
    cam = Camera()
    cam.aspect_ratio = 16.0 / 9.0
    cam.image_width = image_width
    cam.samples_per_pixel = samples_per_pixel
    cam.max_depth = max_depth
    cam.vertical_fov_in_degrees = 40.0
    cam.look_from = (0.0, 3.4, 6.8)
    cam.look_at = (0.0, 0.0, 0.0)
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.defocus_angle_in_degrees = 0.0
    cam.focus_distance = 10.0
    cam.background = scene.SkyGradient((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
    return world, None, cam


def portal_scene(scene, background=None, image_width=1920, samples_per_pixel=500, max_depth=10, quad_material=None):
    """src/main.rs:50-90 portal_scene(): a Portal(WHITE, (2, 0, 0), identity)
    quad in the y = 0 plane and a white Lambertian sphere below the place its
    offset leads to, 16:9, ACES tone map.

    The reference lights it with an EXR image texture
    (rogland_clear_night_4k.exr), which no decoder here reads, so the
    background is a parameter: any Texture, by default the sky gradient of the
    other scenes.  quad_material puts another material in the Portal's place
    (Transparent: the same kernel tier's cost without the Portal arm,
    scripts/portal_rate.py)."""
    if quad_material is None:
        quad_material = scene.Portal((1.0, 1.0, 1.0), (2.0, 0.0, 0.0), Quaternion.identity())
    world = scene.Hittables()
    world.add(scene.Quad((-1.0, 0.0, -1.0), (0.0, 0.0, 2.0), (2.0, 0.0, 0.0), quad_material))
    world.add(scene.Sphere((2.0, -1.5, 0.0), 1.0, scene.Lambertian(scene.SolidColor((1.0, 1.0, 1.0)))))
    cam = Camera()
    cam.aspect_ratio = 16.0 / 9.0
    cam.image_width = image_width
    cam.samples_per_pixel = samples_per_pixel
    cam.max_depth = max_depth
    cam.vertical_fov_in_degrees = 40.0
    cam.look_from = (0.0, 4.0, 2.0)  # Point3::new(0.0, 2.0, 1.0) * 2.0, exact
    cam.look_at = (0.0, 0.0, 0.0)
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.defocus_angle_in_degrees = 0.0
    cam.toon_map = 1  # ToonMap::ACES
    cam.background = background if background is not None else scene.SkyGradient((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))
    return world, None, cam


def _sky(scene, background):
    return background if background is not None else scene.SkyGradient((1.0, 1.0, 1.0), (0.5, 0.7, 1.0))


def disney_scene(scene, background=None, image_width=1920, samples_per_pixel=500, max_depth=10):
    """src/main.rs:92-153 disney_scene(): one unit sphere at the origin under
    Disney::builder() with base_color WHITE, roughness 0, metallic 1, ior 1.5
    and every other field spelled out at its default (main.rs:95-112), 16:9,
    ACES tone map, `camera.render(&world, None)`.

    The reference lights it with rogland_clear_night_4k.exr (main.rs:149-150),
    which no decoder here reads: the background is a parameter, as in
    portal_scene."""
    disney = scene.Disney(scene.SolidColor((1.0, 1.0, 1.0)), roughness=0.0, anisotropic=0.0, sheen=0.0, sheen_tint=0.0,
                          clearcoat=0.0, clearcoat_gloss=0.0, specular_tint=0.0, metallic=1.0, ior=1.5, flatness=0.0,
                          spec_trans=0.0, diff_trans=0.0, thin=False)  # main.rs:95-112
    world = scene.Hittables()
    world.add(scene.Sphere((0.0, 0.0, 0.0), 1.0, disney))  # main.rs:124
    cam = Camera()
    cam.aspect_ratio = 16.0 / 9.0  # main.rs:136-139
    cam.image_width = image_width
    cam.samples_per_pixel = samples_per_pixel
    cam.max_depth = max_depth
    cam.vertical_fov_in_degrees = 40.0  # main.rs:141-144
    cam.look_from = (-4.0, 2.0, 0.0)  # Point3::new(-2.0, 1.0, 0.0) * 2.0, exact
    cam.look_at = (0.0, 0.0, 0.0)
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.defocus_angle_in_degrees = 0.0  # main.rs:146-147
    cam.toon_map = 1  # ToonMap::ACES
    cam.background = _sky(scene, background)
    return world, None, cam  # main.rs:152


def background_scene(scene, background=None, image_width=1920, samples_per_pixel=100, max_depth=10):
    """src/main.rs:155-205 background_scene(): a Mix(Metal, Lambertian, 0.5)
    floor quad and a small sphere of Mix(DiffuseLight, Metal, 0.5), which is
    also the lights (`camera.render(&world, Some(&light))`, main.rs:200): the
    reference clones the sphere, an object here moves into its list, so the
    sphere is built a second time with the same material.  16:9, ACES tone
    map; the background (main.rs:197-198, the EXR) is a parameter, as in
    portal_scene."""
    metal_mat = scene.Metal((1.0, 1.0, 1.0), 0.0)  # main.rs:163
    lam_mat = scene.Lambertian(scene.SolidColor((0.8, 0.8, 0.8)))  # main.rs:164-166
    mix_mat = scene.Mix(metal_mat, lam_mat, 0.5)  # main.rs:167
    world = scene.Hittables()
    world.add(scene.Quad((-2.0, -2.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), mix_mat))  # main.rs:168-173
    light_mat = scene.DiffuseLight(scene.SolidColor((0.75 * 1.0, 1.0 * 1.0, 0.58 * 1.0)))  # main.rs:175-177
    mix_mat2 = scene.Mix(light_mat, metal_mat, 0.5)  # main.rs:178
    world.add(scene.Sphere((1.5, -1.5, 0.0), 0.2, mix_mat2))  # main.rs:179-180
    cam = Camera()
    cam.aspect_ratio = 16.0 / 9.0  # main.rs:184-187
    cam.image_width = image_width
    cam.samples_per_pixel = samples_per_pixel
    cam.max_depth = max_depth
    cam.vertical_fov_in_degrees = 40.0  # main.rs:189-192
    cam.look_from = (-4.0, 2.0, 0.0)  # Point3::new(-2.0, 1.0, 0.0) * 2.0, exact
    cam.look_at = (0.0, 0.0, 0.0)
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.defocus_angle_in_degrees = 0.0  # main.rs:194-195
    cam.toon_map = 1  # ToonMap::ACES
    cam.background = _sky(scene, background)
    lights = scene.Sphere((1.5, -1.5, 0.0), 0.2, mix_mat2)  # light.clone(), main.rs:180, 200
    return world, lights, cam


# main.rs:208-221: (file, vanilla_material) of every Wavefont::new(file, "Final", vanilla), in the order made
OBJ_SCENE_OBJS = (
    ("初音未来.obj", False), ("玻璃球.obj", False), ("外框.obj", False), ("声匣.obj", False), ("镜子门.obj", False),
    ("镜子.obj", True), ("环.obj", False), ("传送门框.obj", False), ("水下.obj", False), ("水面.obj", True),
    ("文字.obj", False), ("mc.obj", False), ("伞.obj", False), ("卒.obj", False),
)
# main.rs:312-332: the world's add order; a name is an entry of OBJ_SCENE_OBJS, a "+name" one of the built objects
_OBJ_SCENE_ORDER = ("初音未来.obj", "+light_board", "玻璃球.obj", "外框.obj", "声匣.obj", "镜子门.obj", "镜子.obj", "环.obj",
                    "传送门框.obj", "水下.obj", "水面.obj", "文字.obj", "+translucent_board", "mc.obj", "+portal", "伞.obj",
                    "+yellow_board", "+black_box", "+fog", "卒.obj")


def obj_scene(scene, asset_dir, background=None, objs=OBJ_SCENE_OBJS, fog="雾.obj", image_width=None,
              samples_per_pixel=3000, max_depth=30):
    """src/main.rs:207-382 obj_scene(), the scene the reference's main runs:
    the Wavefont::new(file, "Final", vanilla) meshes of `objs` from `asset_dir`
    (every MTL material a Disney BSDF, or with vanilla a Metal / Dielectric
    where Pm / Tf say so, obj.rs:271-293), the fog mesh as a ConstantMedium, a
    Portal quad, a thin translucent Disney board, two light boards and a black
    box, added in main.rs:312-332's order; the lights are the two boards as
    EmptyMaterial quads under their Transforms; the camera is
    asset_dir/camera.json with 3000 spp and depth 30.

    `objs`: (file, vanilla) pairs, by default all fourteen of main.rs:208-221;
    a subset keeps the world's add order.  fog=None leaves the medium out.  A
    named file that is absent raises (the reference's unwrap panics).
    image_width overrides camera.json's.  The reference's background is
    13.hdr (main.rs:339-340): a parameter here, any Texture
    (scene.ImageTexture_file reads Radiance HDR), by default the sky gradient
    of the other scenes."""
    api = scene.api
    by_name = dict(objs)
    unknown = [f for f in by_name if f not in _OBJ_SCENE_ORDER]
    if unknown:
        raise ValueError("not a mesh of obj_scene: %r" % unknown)
    for f in list(by_name) + ([fog] if fog is not None else []):
        if not os.path.exists(os.path.join(asset_dir, f)):
            raise FileNotFoundError(os.path.join(asset_dir, f))  # Wavefont::new(..).unwrap()

    def wavefont(file, vanilla):
        return scene.Wavefont(os.path.join(asset_dir, file), vanilla, disney=True)

    # main.rs:208-221, in the order made (handles number the same way on every implementation)
    meshes = {file: wavefont(file, by_name[file]) for file, _ in OBJ_SCENE_OBJS if file in by_name}
    built = {}
    if fog is not None:  # main.rs:223-228
        built["fog"] = scene.ConstantMedium(wavefont(fog, False), 0.05, scene.SolidColor((1.0, 0.936, 0.381)))

    portal_material = scene.Portal((1.0, 1.0, 1.0), (0.0, -6.3, 1.1), Quaternion.identity())  # main.rs:230-234
    portal_anchor = (-5.8035, -0.9983, -7.7198)  # main.rs:236-239
    portal_u = (-3.8206 - portal_anchor[0], -0.9983 - portal_anchor[1], -8.3722 - portal_anchor[2])
    portal_v = (-5.8035 - portal_anchor[0], 3.1159 - portal_anchor[1], -7.7198 - portal_anchor[2])
    built["portal"] = scene.Quad(portal_anchor, portal_u, portal_v, portal_material)

    # main.rs:241-247: Disney::builder().diff_trans(1.0).roughness(1.0).thin(true).build(): base_color is
    # DisneyParameters::default's (0.8, 0.8, 0.8) (disney.rs:36-55)
    translucent_material = scene.Disney(scene.SolidColor((0.8, 0.8, 0.8)), diff_trans=1.0, roughness=1.0, thin=True)

    def board(material):  # main.rs:248-253, 267-272, 285-290, 342-347, 357-362
        return scene.Quad((-1.0, 0.0, -1.0), (0.0, 0.0, 2.0), (2.0, 0.0, 0.0), material)

    def light_transform(obj):  # main.rs:273-281, 348-356
        return scene.Transform(obj, (-0.44579, 5.2955, 0.89889),
                               Quaternion.from_axis_angle(api, (0.921, 0.021, 0.389), 34.7), (3.415, 3.415, 3.415))

    def yellow_transform(obj):  # main.rs:291-299, 363-371
        return scene.Transform(obj, (-1.0053, -1.9655, -4.242),
                               Quaternion.from_axis_angle(api, (0.766, 0.483, -0.423), 85.7),
                               (1.0 * 1.499, 1.0 * 1.499, 1.0 * 1.499))

    built["translucent_board"] = scene.Transform(  # main.rs:254-262
        board(translucent_material), (2.8145, -0.23603, -19.501),
        Quaternion.from_axis_angle(api, (0.993, -0.082, 0.082), 90.4), (2.616, 1.0, 1.0))
    built["light_board"] = light_transform(board(scene.DiffuseLight(scene.SolidColor((4.0, 4.0, 4.0)))))  # :264-281
    # main.rs:282-284: 5.0 * Color::new(1.0, 0.687, 0.0)
    built["yellow_board"] = yellow_transform(board(scene.DiffuseLight(scene.SolidColor((5.0 * 1.0, 5.0 * 0.687, 5.0 * 0.0)))))
    built["black_box"] = scene.Transform(  # main.rs:301-310
        scene.build_box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), scene.DiffuseLight(scene.SolidColor((0.0, 0.0, 0.0)))),
        (-4.9891, -6.4998, -8.3939), None, (1.0 * 6.244, 1.0 * 6.244, 1.0 * 6.244))

    world = scene.Hittables()  # main.rs:312-332
    for name in _OBJ_SCENE_ORDER:
        obj = built.get(name[1:]) if name.startswith("+") else meshes.get(name)
        if obj is not None:
            world.add(obj)

    cam = Camera.from_json(api, os.path.join(asset_dir, "camera.json"))  # main.rs:334
    cam.samples_per_pixel = samples_per_pixel  # main.rs:336-337
    cam.max_depth = max_depth
    if image_width is not None:
        cam.image_width = image_width
    cam.background = _sky(scene, background)  # main.rs:339-340

    lights = scene.Hittables()  # main.rs:342-375
    lights.add(light_transform(board(scene.EmptyMaterial())))
    lights.add(yellow_transform(board(scene.EmptyMaterial())))
    return world, lights, cam
