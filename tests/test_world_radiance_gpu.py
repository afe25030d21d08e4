"""rt_world_radiance on the GPU: Camera::ray_color of caller-given rays against
the oracle's radiance driver on rt_crmath.h (tests/radiance_query.py,
tests/cpp/radiance_oracle.cpp), one world per kernel tier -- lights, media,
wrapper materials, Disney and Portal among them -- at 1 and 4 samples and at
depths 0, 1 and 8.

Bars, per ray where tests/test_parity_gpu.py's check has them per pixel: at
least 0.999 of the rays within 1e-5 * max(1, |oracle|) on all channels, RMSE
below 1e-5 on every channel, `rays` equal on at least 0.999 of the rays, no
panics.  What the GPU must give bit for bit is its own answer again: the same
call twice, a batch split with first_index, the host and the device variant,
any grid size (a lane then takes several rays from the counter), and every
prefix of a batch.
"""
import ctypes
import os
import tempfile

import numpy as np
import pytest

import radiance_query as rq
from conftest import rmse_per_channel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")
REC = 32   # sizeof(rt_radiance)
PAD = 256


@pytest.fixture(scope="module")
def builds(capi, gpu):
    # the check build is a build product (__graft_entry__.build() makes it): absent is a failure
    assert os.path.exists(CHECK_SO), "check build absent: make -C raytracer-2025_amd check (__graft_entry__.build())"
    chk = capi.Api(ctypes.CDLL(CHECK_SO), "rt_")
    assert not chk.missing, chk.missing
    return {"product": gpu, "check": chk}


_worlds = {}


def gpu_world(api, name, build="product"):
    """(scene, world, lights, cam) of a named world on a build of the library, made once per module."""
    key = (name, build)
    if key not in _worlds:
        _worlds[key] = rq.world_case(api, name, tempfile.mkdtemp(prefix="radiance_world_"))[:4]
    return _worlds[key]


def query(api, name, rays, build="product", **kw):
    s, w, l, cam = gpu_world(api, name, build)
    kw.setdefault("max_depth", rq.DEPTH)
    kw.setdefault("seed", rq.SEED)
    return s.radiance(w, l, rays, background=cam.background, **kw)


def check(label, got, want):
    """The bars of the module's docstring; prints every figure before it asserts."""
    (g, gr, gp), (o, orr, op) = got, want
    assert g.shape == o.shape and g.dtype == np.float64 and gr.dtype == np.uint32 and gp.dtype == np.uint32
    ok = rq.within(g, o)
    rmse = rmse_per_channel(g, o) if len(g) else np.zeros(3)
    same_rays = float(np.mean(gr == orr))
    print(f"{label}: {len(g)} rays, within 1e-5: {ok.mean():.5f}, per-channel RMSE {rmse}, rays equal {same_rays:.5f} "
          f"(gpu {int(gr.sum())} oracle {int(orr.sum())}), panics gpu {int(gp.sum())} oracle {int(op.sum())}")
    for i in np.nonzero(~ok)[0][:5]:
        print(f"  ray {i}: gpu {g[i]} ({gr[i]} calls) oracle {o[i]} ({orr[i]} calls)")
    assert np.isfinite(g).all()
    assert ok.mean() >= 0.999
    assert np.all(rmse < 1e-5), rmse
    assert same_rays >= 0.999
    assert not gp.any() and not op.any()


def same_bits(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def _tier(api, capi, name, build="product", flags=0):
    s, w, l, cam = gpu_world(api, name, build)
    info = capi.RtWorldInfo()
    bg = -1 if cam.background is None else cam.background.h
    api.check(api.world_info_get(s.s, w.h, -1 if l is None else l.h, bg, flags, ctypes.byref(info)))
    return info.kernel_tier


# ---------------------------------------------------------------- parity, one world per tier
@pytest.mark.parametrize("samples, depth", [(1, rq.DEPTH), (4, rq.DEPTH), (1, 1), (4, 1)])
@pytest.mark.parametrize("name", list(rq.WORLDS))
def test_radiance_equals_the_oracle(gpu, capi, name, samples, depth):
    assert _tier(gpu, capi, name) == rq.WORLDS[name][1]
    rays, _ = rq.world_rays(name)
    got = query(gpu, name, rays, samples=samples, max_depth=depth)
    check(f"{name} (tier {rq.WORLDS[name][1]}) samples {samples} depth {depth}", got,
          rq.reference(name, samples, depth))


@pytest.mark.parametrize("name", list(rq.WORLDS))
def test_check_build_equals_the_product(builds, capi, name):
    """Every ref the radiance kernels decode is within its array (the check
    build reports one that is not), and both builds give the same bits."""
    rays, _ = rq.world_rays(name)
    assert _tier(builds["check"], capi, name, "check") == rq.WORLDS[name][1]
    chk = query(builds["check"], name, rays, "check", samples=2)
    check(f"{name} / check build", chk, rq.reference(name, 2, rq.DEPTH))
    assert same_bits(chk, query(builds["product"], name, rays, samples=2))


@pytest.mark.parametrize("size", rq.SIZES)
@pytest.mark.parametrize("name", rq.SIZED)
def test_batch_sizes(gpu, name, size):
    """1, a wave and a block of either size, each less and more by one ray: a
    ray's answer is keyed by its index alone, so a prefix of the batch is the
    prefix of its answer, and the oracle's."""
    rays, _ = rq.world_rays(name)
    full = query(gpu, name, rays, samples=4)
    got = query(gpu, name, rays[:size], samples=4)
    assert all(len(a) == size for a in got)
    check(f"{name} first {size}", got, tuple(a[:size] for a in rq.reference(name, 4, rq.DEPTH)))
    assert same_bits(got, tuple(a[:size] for a in full))


@pytest.mark.parametrize("name", ["spheres", "media", "portal"])
def test_depth_zero_is_black(gpu, name):
    """max_depth 0: every ray_color is BLACK (camera.rs:282-284): zeros, no
    call, no panic -- without a kernel launch on the host variant, by a
    memset on the device variant, which writes nothing past out[n - 1]."""
    import torch
    rays, _ = rq.world_rays(name)
    rgb, calls, panics = query(gpu, name, rays, samples=4, max_depth=0)
    assert rgb.shape == (rq.RAYS, 3) and not rgb.any() and not calls.any() and not panics.any()
    n = 65
    s, w, l, cam = gpu_world(gpu, name)
    d_rays = _upload(rays[:n])
    d_out = torch.full((n * REC + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.radiance_device(w, l, d_rays.data_ptr(), n, d_out.data_ptr(), max_depth=0, samples=4, seed=rq.SEED,
                      background=cam.background)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert not out[:n * REC].any() and np.all(out[n * REC:] == 0xA5)


# ---------------------------------------------------------------- consistency and determinism
def _upload(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()


def _device_query(api, name, rays, stream=None, **kw):
    """rt_world_radiance_device through torch's allocations on the current
    device; the record past out[n - 1] (and PAD bytes in all) must come back
    as it was."""
    import torch
    rt = rq.pkg_module("raytracer")
    s, w, l, cam = gpu_world(api, name)
    n = len(rays)
    d_rays = _upload(rays)
    d_out = torch.full((n * REC + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.radiance_device(w, l, d_rays.data_ptr(), n, d_out.data_ptr(), background=cam.background,
                      stream=stream.cuda_stream if stream is not None else None, **kw)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[n * REC:] == 0xA5), "bytes past out[n - 1] were written"
    rec = out[:n * REC].view(rt.RADIANCE_DTYPE)
    return rec["rgb"].copy(), rec["rays"].copy(), rec["panics"].copy()


@pytest.mark.parametrize("name", list(rq.WORLDS))
def test_the_answer_is_the_same_however_it_is_asked_for(gpu, name):
    import torch
    rays, _ = rq.world_rays(name)
    kw = dict(samples=4, max_depth=rq.DEPTH, seed=rq.SEED)
    got = query(gpu, name, rays, **kw)
    # the same call twice
    assert same_bits(query(gpu, name, rays, **kw), got)
    # one batch, and the batch split at 1 000 with first_index
    lo = query(gpu, name, rays[:1000], **kw)
    hi = query(gpu, name, rays[1000:], first_index=1000, **kw)
    assert same_bits(tuple(np.concatenate([a, b]) for a, b in zip(lo, hi)), got)
    # (and first_index does key the draws)
    assert not same_bits(query(gpu, name, rays[1000:], **kw)[:1], (got[0][1000:],))
    # the device variant, on the default stream and on one of the caller's, with a sentinel past the
    # last record; a batch whose last wave holds one ray
    assert same_bits(_device_query(gpu, name, rays, **kw), got)
    assert same_bits(_device_query(gpu, name, rays[:65], stream=torch.cuda.Stream(), **kw), tuple(a[:65] for a in got))
    # fewer lanes than rays: one block, so every lane takes its further rays from the counter
    os.environ["RT_RADIANCE_GRID"] = "1"
    try:
        one_block = query(gpu, name, rays, **kw)
    finally:
        del os.environ["RT_RADIANCE_GRID"]
    assert same_bits(one_block, got)


@pytest.mark.parametrize("name", ["spheres", "mc_obj", "plain_bvh_lit", "disney"])
def test_reference_bvh_flag_agrees(gpu, capi, name):
    """RT_FLAG_REFERENCE_BVH (the reference's own tree, another traversal
    order) against the default build of the tree: the same hits, so the same
    radiance to the bars."""
    rays, _ = rq.world_rays(name)
    default = query(gpu, name, rays, samples=4)
    flagged = query(gpu, name, rays, samples=4, flags=1)
    check(f"{name} RT_FLAG_REFERENCE_BVH vs default", flagged, default)
    check(f"{name} RT_FLAG_REFERENCE_BVH vs the oracle", flagged, rq.reference(name, 4, rq.DEPTH))


def test_another_seed_is_another_answer(gpu):
    name = "plain_bvh_lit"
    rays, _ = rq.world_rays(name)
    s, w, l, cam, _ = rq._oracle_world(name, True)
    want = rq.oracle_radiance(rq.driver(True), s, w, l, rays, seed=0x1234567890ABCDEF, samples=2,
                              background=cam.background)
    got = query(gpu, name, rays, seed=0x1234567890ABCDEF, samples=2)
    check(f"{name} at a 64-bit seed", got, want)
    assert not same_bits(got[:1], query(gpu, name, rays, samples=2)[:1])


# ---------------------------------------------------------------- against rt_render
@pytest.mark.parametrize("name", ["spheres", "plain_bvh_lit", "general_bvh_lit"])
def test_radiance_of_the_camera_rays_is_the_render(gpu, rt, name):
    """A 1-spp rt_render (tiers 0, 2 and 4) against rt_world_radiance of the
    same camera's rays, made on the host (orcx_camera_rays), keyed by their
    pixel: the render's f64 sums, to the bars (the render makes its camera
    ray on the device, so not bit for bit)."""
    s, w, l, cam = gpu_world(gpu, name)
    seed = 11
    spp, depth = cam.samples_per_pixel, cam.max_depth
    cam.samples_per_pixel = 1
    try:
        part, st = cam.render_partials(w, l, seed=seed)
        so, _, _, cam_o, _ = rq._oracle_world(name, True)
        cam_o.samples_per_pixel, cam_o.max_depth = 1, depth
        rays = rq.camera_rays(rq.driver(True), so, cam_o, seed)
    finally:
        cam.samples_per_pixel = spp
    frame = part.reshape(-1, 3)
    assert len(rays) == len(frame) and st.panics == 0
    rgb, calls, panics = s.radiance(w, l, rays, max_depth=depth, samples=1, seed=seed, background=cam.background)
    ok = rq.within(rgb, frame)
    rmse = rmse_per_channel(rgb, frame)
    print(f"{name}: {len(rays)} camera rays, within 1e-5 of the render: {ok.mean():.5f}, per-channel RMSE {rmse}, "
          f"calls {int(calls.sum())} render rays {st.rays}")
    assert ok.mean() >= 0.999 and np.all(rmse < 1e-5) and not panics.any()
    assert abs(int(calls.sum()) - int(st.rays)) <= 1e-3 * st.rays


# ---------------------------------------------------------------- the world cache
def test_a_render_and_a_query_upload_one_flattening_once(gpu, rt):
    name = "uvwrap_flat_lit"
    rays, _ = rq.world_rays(name)
    want = rq.reference(name, 1, rq.DEPTH)
    # a render, then the query, then the render again: nothing flattened for the third (nor, then, for the second)
    s, w, l, cam = rq.world_case(gpu, name)[:4]
    _, _, st0 = cam.render(w, l, seed=3, want_srgb=False)
    got = s.radiance(w, l, rays[:257], max_depth=rq.DEPTH, seed=rq.SEED, background=cam.background)
    _, _, st1 = cam.render(w, l, seed=3, want_srgb=False)
    assert st0.flatten_ms > 0 and st1.flatten_ms == 0
    check("query after a render", got, tuple(a[:257] for a in want))
    # the query first, then the render of the same flattening
    s, w, l, cam = rq.world_case(gpu, name)[:4]
    got = s.radiance(w, l, rays[:257], max_depth=rq.DEPTH, seed=rq.SEED, background=cam.background)
    _, _, st2 = cam.render(w, l, seed=3, want_srgb=False)
    assert st2.flatten_ms == 0
    check("query before a render", got, tuple(a[:257] for a in want))
    # another background is another flattening
    _, _, st3 = cam.render(w, l, seed=3, want_srgb=False)
    assert st3.flatten_ms == 0
    s.radiance(w, l, rays[:64], max_depth=1, seed=rq.SEED, background=s.SkyGradient())
    _, _, st4 = cam.render(w, l, seed=3, want_srgb=False)
    assert st4.flatten_ms > 0
