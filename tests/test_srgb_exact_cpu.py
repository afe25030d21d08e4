"""The exact reference of the output stage (tests/srgb_exact.py: rationals
only) against the f64 formula of Color::to_rgb in numpy, on the inputs the GPU
test (tests/test_to_rgb_gpu.py) feeds the device: every decided case must give
the same byte, an undecided one (a byte boundary within a relative 2^-40 of the
input) may differ by one, and the undecided cases stay far under the 0.1 % the
GPU test allows."""
import numpy as np
import pytest

import srgb_exact as sx


def test_exact_byte_spot_values():
    from fractions import Fraction as Fr
    assert sx.exact_byte(Fr(0), 0) == 0 and sx.exact_byte(Fr(1), 0) == 255 and sx.exact_byte(Fr(2), 0) == 255
    assert sx.exact_byte(Fr(-1), 0) == 0
    # 12.92 * 255 * X = 0.5 at X = 1 / 6589.2: the first byte boundary is linear
    assert sx.exact_byte(Fr(10, 65892), 0) == 1 and sx.exact_byte(Fr(10, 65893), 0) == 0
    # middle grey: 0.5^(1/2.4) * 1.055 - 0.055 = 0.7353569..., * 255 = 187.516...
    assert sx.exact_byte(Fr(1, 2), 0) == 188
    # ACES: 0 -> 0; large -> 2.51 / 2.43, clamped; x < -0.03 / 2.51 maps to a positive value
    assert sx.exact_byte(Fr(0), 1) == 0 and sx.exact_byte(Fr(10 ** 30), 1) == 255
    assert sx.exact_byte(Fr(-1, 100), 1) == 0 and sx.exact_byte(Fr(-1), 1) == 255
    assert sx.exact_byte_special(float("nan"), 0) == 0 and sx.exact_byte_special(float("inf"), 0) == 255
    assert sx.exact_byte_special(float("-inf"), 0) == 0 and sx.exact_byte_special(float("-inf"), 1) == 0
    assert sx.exact_byte_special(float("inf"), 1) == 0  # inf * inf / inf = NaN in the reference's f64


@pytest.mark.parametrize("toon", [0, 1])
def test_thresholds_are_the_smallest(toon):
    thr = sx.thresholds(toon)
    assert len(thr) == 255
    for k in (1, 2, 10, 11, 128, 254, 255):
        b = thr[k - 1]
        assert sx.exact_byte(sx.f32_bits_to_fraction(b), toon) == k
        assert sx.exact_byte(sx.f32_bits_to_fraction(b - 1), toon) == k - 1


@pytest.mark.parametrize("toon", [0, 1])
def test_reference_matches_f64_formula(toon):
    x = np.concatenate([sx.boundary_inputs(toon), sx.random_inputs(4 << 20)])
    want, und = sx.expected(x, toon)
    got = sx.f64_formula(x, toon)
    diff = np.abs(got - want)
    share = float(und.mean())
    print("toon %d: %d inputs, %d undecided (share %.2e), %d differ from the f64 formula (all undecided: %s)" %
          (toon, x.size, int(und.sum()), share, int((diff != 0).sum()), bool(und[diff != 0].all())))
    assert not (diff[~und] != 0).any(), (x[~und][diff[~und] != 0][:5], got[~und][diff[~und] != 0][:5])
    assert diff.max() <= 1
    assert share < 1e-4  # a tenth of what the GPU test allows
    if toon == 0:
        # without ACES the boundary neighbours and 20 000 random values agree on every case
        xb = np.concatenate([sx.boundary_inputs(0), sx.random_inputs(20000, seed=7)])
        assert (sx.f64_formula(xb, 0) == sx.expected(xb, 0)[0]).all()


def test_searchsorted_classification_equals_direct_evaluation():
    """expected()'s threshold classification against exact_byte case by case."""
    x = np.concatenate([sx.random_inputs(300, seed=3), sx.EDGES])
    for toon in (0, 1):
        want, _ = sx.expected(x, toon)
        direct = [sx.exact_byte(float(v), toon) for v in x]
        assert want.tolist() == direct
