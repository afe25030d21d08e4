"""The f32 stages of the closest-hit walk as the GPU compiles them, through
rt_walk_selftest (the device functions the path kernels call: make_rayf +
slab_f, make_sphf + sphere_filter, rcp_f32, sqrt_f32, Closest::set / lower,
f32_down), against exact references:

 - the box test and the sphere filter on the case tables of the CPU generators
   (tests/cpp/slab_prop.cpp, tests/cpp/filter_prop.cpp --dump: random and
   adversarial cases with the exact verdict of each), under the conditions the
   CPU property tests (test_slab_cpu.py, test_filter_cpu.py) put on the g++
   build; how many device results differ from that build's is printed;
 - the hardware reciprocal and square root within one ulp of the correctly
   rounded result -- what the host builds emulate (RT_RCP_EMU = +-1) and what
   the sphere filter's margins assume;
 - Closest's f32 bound never below the f64 hit distance; f32_down the largest
   f32 not above its argument."""
import ctypes

import numpy as np
import pytest

import walk_tables as wt

pytestmark = pytest.mark.gpu

N = 1000000
P = ctypes.POINTER(ctypes.c_double)
OUT_W = {0: 2, 1: 2, 2: 1, 3: 1, 4: 1, 5: 1, 6: 1}


def walk(gpu, fn, inp):
    inp = np.ascontiguousarray(inp, dtype=np.float64)
    n = inp.shape[0]
    out = np.empty((n, OUT_W[fn]), dtype=np.float64)
    gpu.check(gpu.walk_selftest(fn, inp.ctypes.data_as(P), out.ctypes.data_as(P), n))
    return out


@pytest.fixture(scope="module")
def gens(tmp_path_factory):
    """The generators, built for this run with g++ (host code only)."""
    d = tmp_path_factory.mktemp("walk_filters")
    return {k: wt.build(k, d) for k in ("slab", "filter")}, str(d)


@pytest.mark.parametrize("seed", [2025, 7])
def test_device_slab_is_conservative(gpu, gens, seed):
    exes, d = gens
    (n, hits, fhits, bad), t = wt.run(exes["slab"], N, seed, dump="%s/slab_%d.bin" % (d, seed))
    out = walk(gpu, 0, t[:, :wt.SLAB_IN])
    dev_hit = out[:, 0] == 1
    ex = t[:, 14] == 1
    viol = ex & ~dev_hit
    host_hit = t[:, 15] == 1
    same_entry = (out[:, 1] == t[:, 16]) | (np.isnan(out[:, 1]) & np.isnan(t[:, 16]))
    print("slab seed %d: %d cases, %d exact hits, %d device hits, %d host hits; device != host: %d verdicts, %d entries; "
          "violations %d" % (seed, len(t), int(ex.sum()), int(dev_hit.sum()), int(host_hit.sum()),
                             int((dev_hit != host_hit).sum()), int((~same_entry).sum()), int(viol.sum())))
    assert int(ex.sum()) == hits
    assert not viol.any(), t[viol][:5].tolist()
    assert dev_hit.sum() >= ex.sum() and ex.sum() > n // 5


@pytest.mark.parametrize("seed", [2025, 7])
def test_device_sphere_filter_is_conservative(gpu, gens, seed):
    exes, d = gens
    (n, rejected, lowered, bad), t = wt.run(exes["filter"], N, seed, dump="%s/filter_%d.bin" % (d, seed))
    out = walk(gpu, 1, t[:, :wt.FILTER_IN])
    keep, cf2 = out[:, 0], out[:, 1]
    rej, low, viol = wt.filter_verdict(t, keep, cf2)
    same_cf = (cf2 == t[:, 14]) | (np.isnan(cf2) & np.isnan(t[:, 14]))
    print("filter seed %d: %d cases, device rejected %d lowered %d (host %d, %d); device != host: %d verdicts, %d bounds; "
          "violations %d" % (seed, len(t), rej, low, rejected, lowered, int((keep != t[:, 13]).sum()),
                             int((~same_cf).sum()), int(viol.sum())))
    assert len(t) == n
    assert not viol.any(), (t[viol][:5].tolist(), out[viol][:5].tolist())
    assert rej > n // 10 and low > n // 50


def _f32_samples(exponents, rng):
    """4096 random mantissas per biased f32 exponent, plus every power of two
    and its two neighbours (positive bit patterns)."""
    e = np.asarray(list(exponents), dtype=np.uint32)
    bits = (np.repeat(e, 4096) << 23) | rng.integers(0, 1 << 23, e.size * 4096, dtype=np.uint32)
    pow2 = e << 23
    return np.concatenate([bits, pow2, pow2 - 1, pow2 + 1]).astype(np.uint32)


def _ulp_report(name, x, got, want, exact):
    """Asserts got is want (the correctly rounded f32) or one of its two
    neighbours; returns the worst error in ulps of the correctly rounded
    result against the f64 value `exact`."""
    up, down = np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))
    ok = (got == want) | (got == up) | (got == down)
    ulp = (up.astype(np.float64) - want.astype(np.float64))
    err = np.abs(got.astype(np.float64) - exact) / ulp
    print("%s: %d arguments, %d not correctly rounded (%.3f %%), worst error %.4f ulp at x = %s" %
          (name, x.size, int((got != want).sum()), 100.0 * float((got != want).mean()), float(err.max()),
           float(x[np.argmax(err)]).hex()))
    assert ok.all(), (name, [float(v).hex() for v in x[~ok][:5]], [float(v).hex() for v in got[~ok][:5]])
    return float(err.max())


def test_hardware_reciprocal_within_one_ulp(gpu):
    """rcp_f32 (v_rcp_f32) wherever x and 1 / x are both normal: the correctly
    rounded quotient or a neighbour -- exactly what RT_RCP_EMU = +-1 emulates
    in the CPU property tests."""
    rng = np.random.default_rng(2025)
    pos = _f32_samples(range(1, 255), rng)
    x = np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)
    got = walk(gpu, 2, x.astype(np.float64))[:, 0]
    assert (got.astype(np.float32).astype(np.float64) == got).all()  # an f32 travels exactly
    got = got.astype(np.float32)
    tiny = np.float32(1.1754944e-38)
    with np.errstate(all="ignore"):
        want = np.float32(1) / x
    normal = (np.abs(x) >= tiny) & (np.abs(want) >= tiny) & np.isfinite(want)
    worst = _ulp_report("rcp_f32", x[normal], got[normal], want[normal], 1.0 / x[normal].astype(np.float64))
    assert worst <= 1.5  # a neighbour of the correctly rounded quotient is within 1.5 ulp of 1 / x
    # outside the normal range: reported, not asserted
    spec = np.array([0.0, -0.0, 1e-45, 1e-40, -1e-40, 1.1754942e-38, 8.6e37, 1.8e38, -3.4028235e38, np.inf, -np.inf, np.nan],
                    dtype=np.float32)
    r = walk(gpu, 2, spec.astype(np.float64))[:, 0]
    print("rcp_f32 outside the normal range: " + ", ".join("%g -> %g" % (float(a), float(b)) for a, b in zip(spec, r)))


def test_hardware_square_root_within_one_ulp(gpu):
    """sqrt_f32 (v_sqrt_f32, what make_sphf takes for ehd) over the positive
    normal range: the correctly rounded root or a neighbour.  ehd = 2^-19 |d|
    is five times the 6.2u bound it scales (rt_sphere_filter.h), so an error
    of a few ulps of the root (each 2^-23 relative at most) leaves that margin."""
    rng = np.random.default_rng(7)
    x = _f32_samples(range(1, 255), rng).view(np.float32)
    x = x[x >= np.float32(1.1754944e-38)]  # the neighbour below the smallest power of two is subnormal
    got = walk(gpu, 3, x.astype(np.float64))[:, 0]
    assert (got.astype(np.float32).astype(np.float64) == got).all()
    got = got.astype(np.float32)
    want = np.sqrt(x)
    worst = _ulp_report("sqrt_f32", x, got, want, np.sqrt(x.astype(np.float64)))
    assert worst <= 1.5
    spec = np.array([0.0, -0.0, 1e-45, 1e-40, 1.1754942e-38, -1.0, np.inf, np.nan], dtype=np.float32)
    r = walk(gpu, 3, spec.astype(np.float64))[:, 0]
    print("sqrt_f32 outside the normal range: " + ", ".join("%g -> %g" % (float(a), float(b)) for a, b in zip(spec, r)))


def _closest_inputs():
    """t over every binade from 1e-8 to 1e300 (64 random mantissas each, the
    binade's ends), and doubles just above and below f32-representable numbers."""
    rng = np.random.default_rng(2025)
    e = np.arange(-27, 997)
    t = [np.ldexp(1.0 + rng.random((e.size, 64)), e[:, None]).ravel(), np.ldexp(1.0, e),
         np.nextafter(np.ldexp(1.0, e), 0.0)]
    fb = rng.integers(0x322BCC77, 0x7F800000, 100000, dtype=np.uint32)  # f32 in [1e-8, FLT_MAX]
    f = np.concatenate([fb, [0x7F7FFFFF, 0x322BCC77, 0x3F800000]]).astype(np.uint32).view(np.float32).astype(np.float64)
    t += [f, np.nextafter(f, np.inf), np.nextafter(f, 0.0)]
    t = np.concatenate(t)
    return t[(t >= 1e-8) & (t <= 1e300)]


def test_closest_bound_is_never_below_t(gpu):
    """Closest::set: (double)c_f >= t (c_f = +inf above FLT_MAX); Closest::lower
    from a given c_f: the smaller of the old bound and set's."""
    t = _closest_inputs()
    cf = walk(gpu, 4, t[:, None])[:, 0]
    assert (cf.astype(np.float32).astype(np.float64) == cf).all()
    below = cf < t
    print("Closest::set: %d values of t, %d with c_f < t, %d with c_f = inf (t > FLT_MAX: %d)" %
          (t.size, int(below.sum()), int(np.isinf(cf).sum()), int((t > 3.4028234663852886e38).sum())))
    assert not below.any(), [(float(a).hex(), float(b).hex()) for a, b in zip(t[below][:5], cf[below][:5])]
    assert not np.isinf(cf[t < 3.4028e38 * (1 - 2.0 ** -22)]).any()  # and only inf where FLT_MAX cannot hold it
    # lower: old bounds above, at and below set's bound, and none (inf)
    rng = np.random.default_rng(7)
    with np.errstate(over="ignore"):
        scale = np.array([0.5, 1.0 - 2.0 ** -23, 1.0, 1.0 + 2.0 ** -22, 2.0])[rng.integers(0, 5, t.size)]
        old = np.where(rng.random(t.size) < 0.2, np.inf, (cf * scale).astype(np.float32).astype(np.float64))
    low = walk(gpu, 5, np.stack([t, old], axis=1))[:, 0]
    assert (low == np.minimum(old, cf)).all()


def test_f32_down_is_the_largest_f32_not_above(gpu):
    rng = np.random.default_rng(2025)
    e = np.arange(-160, 135)  # below the smallest f32 subnormal to above FLT_MAX
    x = np.ldexp(1.0 + rng.random((e.size, 64)), e[:, None]).ravel()
    fb = rng.integers(0, 0x7F800000, 100000, dtype=np.uint32).view(np.float32).astype(np.float64)  # subnormals too
    x = np.concatenate([x, fb, np.nextafter(fb, np.inf), np.nextafter(fb, -np.inf), [0.0, 1e-300, 5e-324, 1e300]])
    x = np.concatenate([x, -x])
    got = walk(gpu, 6, x[:, None])[:, 0]
    assert (got.astype(np.float32).astype(np.float64) == got).all()
    with np.errstate(over="ignore", under="ignore"):
        f = x.astype(np.float32)
    want = np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float64)
    fin = np.isfinite(want)
    with np.errstate(over="ignore"):
        above = np.nextafter(want.astype(np.float32), np.float32(np.inf)).astype(np.float64)
    assert (want <= x).all() and (above[fin] > x[fin]).all()  # the numpy reference is what the name says
    bad = (got != want) | (np.signbit(got) != np.signbit(want))
    assert not bad.any(), [(float(a).hex(), float(b).hex(), float(c).hex()) for a, b, c in
                           zip(x[bad][:5], got[bad][:5], want[bad][:5])]
