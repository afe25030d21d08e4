"""The device output stage (srgb_u8 of rt_kernel_common.hip through rt_to_rgb_device:
ACES or not, sRGB OETF with ocml's pow, round, clamp) against the exact
rational reference of tests/srgb_exact.py, on the inputs where it can go
wrong: the +-64-ulp neighbourhood of every byte threshold, the +-4-ulp
neighbourhood of the 0.0031308 knee, 4 M random f32 bit patterns in [0, 4],
and +-0, subnormals, negatives (under ACES x < -0.012 maps towards white),
values > 1, +-inf and NaN.

A decided case (the exact byte is the same for X (1 - 2^-40) and X (1 + 2^-40),
about a thousand times the f64 evaluation error of the formula) must match the
device byte exactly; an undecided one may differ by one, and at most 0.1 % of
the inputs may be undecided (measured: none, tests/test_srgb_exact_cpu.py)."""
import ctypes

import numpy as np
import pytest

import srgb_exact as sx

pytestmark = pytest.mark.gpu


def device_bytes(gpu, x, toon):
    import torch
    x = np.ascontiguousarray(x, dtype=np.float32)
    dl = torch.from_numpy(x).cuda()
    du = torch.empty(x.shape, dtype=torch.uint8, device="cuda")
    gpu.check(gpu.to_rgb_device(ctypes.c_void_p(dl.data_ptr()), ctypes.c_void_p(du.data_ptr()), x.size, toon,
                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return du.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("toon", [0, 1])
def test_to_rgb_bytes_are_exact(gpu, toon):
    x = np.concatenate([sx.boundary_inputs(toon), sx.random_inputs(4 << 20)])
    want, und = sx.expected(x, toon)
    got = device_bytes(gpu, x, toon)
    diff = np.abs(got - want)
    bad = (diff != 0) & ~und
    print("toon %d: %d inputs, %d undecided (share %.2e), %d device bytes differ (%d of them decided)" %
          (toon, x.size, int(und.sum()), float(und.mean()), int((diff != 0).sum()), int(bad.sum())))
    assert und.mean() <= 1e-3
    assert not bad.any(), [(float(v).hex(), int(g), int(w)) for v, g, w in zip(x[bad][:8], got[bad][:8], want[bad][:8])]
    assert diff.max() <= 1


@pytest.mark.parametrize("toon", [0, 1])
def test_to_rgb_edge_values(gpu, toon):
    """Negatives give 0 without ACES and the reference's value with it; +inf
    gives 255; NaN gives 0 (Rust's saturating `as u8`) -- and so does either
    infinity with ACES, where the reference's f64 arithmetic (color.rs:14-25)
    makes inf * inf / inf = NaN before the clamp."""
    fin = np.concatenate([sx.EDGES, np.array([-3.0e38, -0.0121, -0.0119, -0.5, 3.4028235e38], dtype=np.float32)])
    want, und = sx.expected(fin, toon)
    assert not und.any()
    got = device_bytes(gpu, fin, toon)
    print("toon %d finite edges: %s" % (toon, [(float(v), int(g)) for v, g in zip(fin, got)]))
    assert got.tolist() == want.tolist(), [(float(v), int(g), int(w)) for v, g, w in zip(fin, got, want) if g != w]
    if toon == 0:
        assert (got[fin <= 0] == 0).all()
    spec = np.array([np.inf, -np.inf, np.nan, -np.nan], dtype=np.float32)
    got = device_bytes(gpu, spec, toon)
    want = [sx.exact_byte_special(float(v), toon) for v in spec]
    print("toon %d specials (+inf, -inf, nan, -nan): %s" % (toon, got.tolist()))
    assert got.tolist() == want
