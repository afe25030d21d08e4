"""The tree the flatten builds, through rt_world_info_get and rt_world_selftest
on CPU: the C2 world's 4-wide tree after the full-sweep SAH rebuild and the
cost-optimal collapse, and the parallel build against the serial one on worlds
on both sides of the sweep's range (RT_SAH_SWEEP_MAX = 2048 items)."""
import ctypes
import random

PARENT_C2_NODES = 241  # the C2 tree of the commit before the sweep + optimal collapse (binned SAH, greedy collapse)


def test_c2_tree_is_smaller_and_stays_in_the_basic_tier(product, rt, scenes, capi):
    s = rt.Scene(product)
    world, lights, cam = scenes.random_spheres(s, 1920, 16)
    info = capi.RtWorldInfo()
    assert product.world_info_get(s.s, world.h, -1, cam.background.h, 0, ctypes.byref(info)) == 0
    print("C2: tier", info.kernel_tier, "nodes", info.bvh_nodes, "stack need", info.stack_need)
    assert info.kernel_tier == 0
    assert info.stack_need <= 14
    # 485 leaves: at least ceil(484 / 3) = 162 nodes of up to four children
    assert 162 <= info.bvh_nodes < PARENT_C2_NODES


def _sphere_world(rt, product, n, seed):
    rng = random.Random(seed)
    s = rt.Scene(product)
    mat = s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))
    lst = s.Hittables()
    for _ in range(n):
        # a coarse grid in x and z: many equal centroids on two axes
        c = (float(rng.randrange(200)) * 0.5, rng.uniform(-1, 1), float(rng.randrange(200)) * 0.5)
        lst.add(s.Sphere(c, 0.2, mat))
    world = s.Hittables()
    world.add(s.BVH(lst))
    world.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, mat))
    return s, world


def test_parallel_flatten_equals_serial_just_past_the_sweep_range(product, rt):
    """2049 spheres and the ground: the root range is binned, every range below it swept."""
    s, world = _sphere_world(rt, product, 2049, 5)
    assert product.world_selftest(s.s, world.h, -1, -1) == 1


def test_parallel_flatten_equals_serial_70000_spheres(product, rt):
    """Past the parallel build's threshold (32768 items a node): binned ranges
    on several threads over swept ones, spliced in preorder."""
    s, world = _sphere_world(rt, product, 70000, 3)
    assert product.world_selftest(s.s, world.h, -1, -1) == 1
