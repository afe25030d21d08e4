"""rt_lights_pdf / rt_lights_sample on the GPU: lights.pdf_value and
lights.random of six light sets (tests/lights_query.py) against the oracle's
driver, bit for bit -- the f64 bit patterns, a NaN matching a NaN -- on the
product and on the check build.  The bar is bit-equality, not a tolerance: the
render evaluates these same device functions at every lit vertex and is held
to RMSE 0 against the same restatement.

Then what a batched query can get wrong on its own: prefixes round a wave's
size, samples that straddle a wave, the top of the index range, several
grid-stride trips (RT_LIGHTS_GRID=1), the device variants and the bytes past
their output, the world cache shared with renders and radiance queries, and the
panicking origin's neighbours.
"""
import ctypes
import os

import numpy as np
import pytest

import lights_query as lq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")
PAD = 256
NAMES = sorted(lq.SETS)


@pytest.fixture(scope="module")
def builds(capi, gpu):
    # the check build is a build product (__graft_entry__.build() makes it): absent is a failure
    assert os.path.exists(CHECK_SO), "check build absent: make -C raytracer-2025_amd check (__graft_entry__.build())"
    chk = capi.Api(ctypes.CDLL(CHECK_SO), "rt_")
    assert not chk.missing, chk.missing
    return {"product": gpu, "check": chk}


def _report_pdf(name, got, want):
    bad = np.nonzero(~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))))[0]
    print(f"{name}: pdf of {len(want)} points, {np.mean(want != 0):.3f} non-zero, {int(np.isnan(want).sum())} NaN, "
          f"{len(bad)} differ from the driver" + "".join(f"\n  {i}: gpu {got[i]!r} driver {want[i]!r}" for i in bad[:5]))


def _report_samples(name, got, want):
    g, w = got.reshape(-1), want.reshape(-1)
    same = np.all((g["dir"].view(np.uint64) == w["dir"].view(np.uint64)) | (np.isnan(g["dir"]) & np.isnan(w["dir"])), axis=1)
    same &= (g["pdf"].view(np.uint64) == w["pdf"].view(np.uint64)) | (np.isnan(g["pdf"]) & np.isnan(w["pdf"]))
    same &= g["flags"] == w["flags"]
    bad = np.nonzero(~same)[0]
    print(f"{name}: {len(w)} draws, {int((w['flags'] != 0).sum())} panicked, {len(bad)} differ from the driver"
          + "".join(f"\n  {i}: gpu {g[i]} driver {w[i]}" for i in bad[:5]))


@pytest.mark.parametrize("build", ["product", "check"])
@pytest.mark.parametrize("name", NAMES)
def test_lights_pdf_equals_the_oracle_bit_for_bit(builds, name, build):
    o, d, pdf, _ = lq.reference(name)
    s, w, l, _ = lq.set_case(builds[build], name)
    got = s.lights_pdf(w, l, o, d)
    assert got.shape == (lq.N,) and got.dtype == np.float64
    _report_pdf(f"{name} / {build}", got, pdf)
    assert lq.same_bits(got, pdf)
    assert lq.same_bits(s.lights_pdf(w, l, o, d, flags=1), pdf)  # RT_FLAG_REFERENCE_BVH names another flattening only


@pytest.mark.parametrize("build", ["product", "check"])
@pytest.mark.parametrize("name", NAMES)
def test_lights_sample_equals_the_oracle_bit_for_bit(builds, rt, name, build):
    o, _, _, smp = lq.reference(name)
    s, w, l, _ = lq.set_case(builds[build], name)
    got = s.lights_sample(w, l, o, samples=lq.SAMPLES, seed=lq.SEED)
    assert got.shape == (lq.N, lq.SAMPLES) and got.dtype == rt.LIGHT_SAMPLE_DTYPE
    _report_samples(f"{name} / {build}", got, smp)
    assert lq.same_samples(got, smp)
    # self-consistency on the GPU: a draw's pdf is the pdf query's value of its direction
    good = got["flags"] == 0
    og = np.repeat(o, lq.SAMPLES, axis=0)[good.reshape(-1)]
    assert lq.same_bits(s.lights_pdf(w, l, og, got["dir"][good]), got["pdf"][good])


@pytest.mark.parametrize("name", NAMES)
def test_prefixes_sample_counts_and_the_top_of_the_index_range(gpu, name):
    o, d, pdf, smp = lq.reference(name)
    drv = lq.driver()
    so, wo, lo, _ = lq.oracle_case(name)
    s, w, l, _ = lq.set_case(gpu, name)
    full_pdf = s.lights_pdf(w, l, o, d)
    full_smp = s.lights_sample(w, l, o, samples=lq.SAMPLES, seed=lq.SEED)
    # prefixes: an item's answer is keyed by its index alone
    for n in (1, 63, 64, 65, 1025):
        assert lq.same_bits(s.lights_pdf(w, l, o[:n], d[:n]), full_pdf[:n]), n
        assert lq.same_samples(s.lights_sample(w, l, o[:n], samples=lq.SAMPLES, seed=lq.SEED), full_smp[:n]), n
    # samples 1, 3, 4 at n = 65: an origin's samples straddle a wave; sample s of a call is sample s of any call
    k = lq.N - 16 - 65 if lq.SETS[name][2] is not None else 0  # (with the origins inside the sphere light, if any)
    o65 = o[k:k + 65]
    by = {m: s.lights_sample(w, l, o65, samples=m, seed=lq.SEED, first_index=k) for m in (1, 3, 4)}
    assert lq.same_samples(by[3], full_smp[k:k + 65])
    assert lq.same_samples(by[1], by[4][:, :1]) and lq.same_samples(by[3], by[4][:, :3])
    assert lq.same_samples(by[4], lq.oracle_sample(drv, so, lo, o65, 4, lq.SEED, first_index=k))
    # first_index = 2^32 - 65 with n = 65: the last index is 2^32 - 1
    top = (1 << 32) - 65
    got = s.lights_sample(w, l, o65, samples=lq.SAMPLES, seed=lq.SEED, first_index=top)
    assert lq.same_samples(got, lq.oracle_sample(drv, so, lo, o65, lq.SAMPLES, lq.SEED, first_index=top))
    # (another index is another draw: the box's first origins, none of which panics in one_sphere)
    moved = s.lights_sample(w, l, o[:65], samples=lq.SAMPLES, seed=lq.SEED, first_index=top)
    assert lq.same_samples(moved, lq.oracle_sample(drv, so, lo, o[:65], lq.SAMPLES, lq.SEED, first_index=top))
    assert not lq.same_samples(moved, full_smp[:65])
    with pytest.raises(Exception, match="2\\^32"):
        s.lights_sample(w, l, o65, samples=lq.SAMPLES, seed=lq.SEED, first_index=top + 1)


@pytest.mark.parametrize("name", ["flat", "tree"])
def test_one_block_makes_several_grid_stride_trips(gpu, name):
    """RT_LIGHTS_GRID=1: 4 096 items on 256 lanes, 16 trips a lane (48 for the draws)."""
    o, d, pdf, smp = lq.reference(name)
    s, w, l, _ = lq.set_case(gpu, name)
    os.environ["RT_LIGHTS_GRID"] = "1"
    try:
        one_pdf = s.lights_pdf(w, l, o, d)
        one_smp = s.lights_sample(w, l, o, samples=lq.SAMPLES, seed=lq.SEED)
    finally:
        del os.environ["RT_LIGHTS_GRID"]
    assert lq.same_bits(one_pdf, pdf) and lq.same_samples(one_smp, smp)
    assert lq.same_bits(s.lights_pdf(w, l, o, d), one_pdf)
    assert lq.same_samples(s.lights_sample(w, l, o, samples=lq.SAMPLES, seed=lq.SEED), one_smp)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def _device_pdf(s, w, l, o, d, **kw):
    import torch
    n = len(o)
    d_o, d_d = _dev(o), _dev(d)
    out = torch.full((n * 8 + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.lights_pdf_device(w, l, d_o.data_ptr(), d_d.data_ptr(), n, out.data_ptr(), **kw)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert np.all(raw[n * 8:] == 0xA5), "bytes past out[n - 1] were written"
    return raw[:n * 8]


def _device_sample(s, w, l, o, samples, **kw):
    import torch
    n = len(o)
    d_o = _dev(o)
    out = torch.full((n * samples * 40 + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.lights_sample_device(w, l, d_o.data_ptr(), n, out.data_ptr(), samples=samples, **kw)
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert np.all(raw[n * samples * 40:] == 0xA5), "bytes past the last record were written"
    return raw[:n * samples * 40]


@pytest.mark.parametrize("name", NAMES)
def test_device_variants_give_the_host_variants_bytes(gpu, rt, name):
    import torch
    o, d, pdf, smp = lq.reference(name)
    s, w, l, _ = lq.set_case(gpu, name)
    host_pdf = s.lights_pdf(w, l, o, d)
    host_smp = s.lights_sample(w, l, o, samples=lq.SAMPLES, seed=lq.SEED)
    assert not host_smp["reserved"].any()
    for n in (lq.N, 65):
        raw = _device_pdf(s, w, l, o[:n], d[:n])
        assert raw.tobytes() == host_pdf[:n].tobytes(), n
        assert _device_pdf(s, w, l, o[:n], d[:n]).tobytes() == raw.tobytes()  # a second identical call
        raw = _device_sample(s, w, l, o[:n], lq.SAMPLES, seed=lq.SEED)
        assert raw.tobytes() == host_smp[:n].tobytes(), n
        assert _device_sample(s, w, l, o[:n], lq.SAMPLES, seed=lq.SEED).tobytes() == raw.tobytes()
    # on a stream of the caller's
    stream = torch.cuda.Stream()
    d_o = _dev(o)
    out = torch.full((lq.N * lq.SAMPLES * 40 + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s.lights_sample_device(w, l, d_o.data_ptr(), lq.N, out.data_ptr(), samples=lq.SAMPLES, seed=lq.SEED,
                           stream=stream.cuda_stream)
    stream.synchronize()
    raw = out.cpu().numpy()
    assert np.all(raw[-PAD:] == 0xA5) and raw[:-PAD].tobytes() == host_smp.tobytes()


def test_the_panicking_origin_and_its_neighbours(gpu):
    """`one_sphere`: every draw from the light's centre has the flag and zeros;
    the origins before and after it are the driver's, untouched."""
    name = "one_sphere"
    o, _, _, smp = lq.reference(name)
    k = lq.N - 16 - 1
    assert np.array_equal(o[k], lq.SPHERE[0])
    s, w, l, _ = lq.set_case(gpu, name)
    got = s.lights_sample(w, l, o[k - 70:k + 9], samples=lq.SAMPLES, seed=lq.SEED, first_index=k - 70)
    assert np.all(got["flags"][70] == lq.PANIC) and not got["dir"][70].any() and not got["pdf"][70].any()
    assert lq.same_samples(got, smp[k - 70:k + 9])
    after = got[71:]
    assert not after["flags"].any() and np.all(after["pdf"] > 0)
    raw = _device_sample(s, w, l, o[k:k + 1], lq.SAMPLES, seed=lq.SEED, first_index=k)
    assert raw.tobytes() == got[70:71].tobytes()


@pytest.mark.parametrize("name", ["flat", "tree"])
def test_a_render_a_radiance_query_and_a_lights_query_upload_once(gpu, rt, name):
    o, d, pdf, smp = lq.reference(name)
    rays = np.zeros((64, 8))
    rays[:, 0:3], rays[:, 3:6], rays[:, 7] = o[:64], d[:64], np.inf
    # a render first: nothing is flattened for what follows
    s, w, l, cam = lq.set_case(gpu, name)
    first, _, st0 = cam.render(w, l, seed=3, want_srgb=False)
    s.radiance(w, l, rays, max_depth=4, seed=5)
    got_pdf = s.lights_pdf(w, l, o[:257], d[:257])
    second, _, st1 = cam.render(w, l, seed=3, want_srgb=False)
    got_smp = s.lights_sample(w, l, o[:257], samples=lq.SAMPLES, seed=lq.SEED)
    third, _, st2 = cam.render(w, l, seed=3, want_srgb=False)
    assert st0.flatten_ms > 0 and st1.flatten_ms == 0 and st2.flatten_ms == 0
    assert lq.same_bits(got_pdf, pdf[:257]) and lq.same_samples(got_smp, smp[:257])
    # a lights query between two renders leaves the second bit-equal to the first
    assert np.array_equal(first, second) and np.array_equal(first, third)
    # the lights query first, then the render of the same flattening
    s, w, l, cam = lq.set_case(gpu, name)
    got_pdf = s.lights_pdf(w, l, o[:257], d[:257])
    again, _, st3 = cam.render(w, l, seed=3, want_srgb=False)
    assert st3.flatten_ms == 0
    assert lq.same_bits(got_pdf, pdf[:257]) and np.array_equal(again, first)
    # another background is another flattening
    s.lights_pdf(w, l, o[:64], d[:64], background=s.SkyGradient())
    _, _, st4 = cam.render(w, l, seed=3, want_srgb=False)
    assert st4.flatten_ms > 0
