"""TEST HARNESS: an exact reference of the output stage, Color::to_rgb
(color.rs:14-36: optional ACES fit, clamp, sRGB OETF, f64 -> u8), for f32
inputs -- the stdlib `fractions` module only, no floating point in a decision.

An f32 input is an exact rational X.  The real-valued function is
    v(X) = 255 * 12.92 * X                          for X <= 0.0031308,
    v(X) = 255 * (1.055 * X^(1/2.4) - 0.055)        above,
after X went through the ACES rational function (decimal constants, clamped to
[0, 1]) for toon_map = 1; the byte is v rounded half away from zero, clamped to
[0, 255].  "byte >= k" is v >= k - 1/2, which above the knee is
    X^5 >= (((k - 1/2) / 255 + 0.055) / 1.055)^12,
decided in rationals.  For X >= 0 both maps are monotone (the ACES derivative
is positive there), so the 255 smallest f32 values that reach each byte
(thresholds(), by bisection over f32 bit patterns) classify any number of
non-negative inputs with one searchsorted; negative inputs are evaluated
directly.  +-inf and NaN are no rationals: exact_byte_special().

A case is *decided* when the exact byte is the same for X (1 - 2^-40) and
X (1 + 2^-40): about a thousand times the f64 evaluation error of the formula
(some ten roundings plus pow's), so an f64 implementation must match a decided
case exactly and may be off by one on an undecided one."""
import functools
import struct
from fractions import Fraction as Fr

import numpy as np

KNEE = Fr("0.0031308")
LIN = 255 * Fr("12.92")
EPS = Fr(1, 2 ** 40)
# B(k)^12 of "byte >= k" above the knee, k = 1 .. 255
_B12 = [None] + [(((Fr(2 * k - 1, 2) / 255) + Fr("0.055")) / Fr("1.055")) ** 12 for k in range(1, 256)]


def f32_bits_to_fraction(bits):
    """The exact value of a finite f32 bit pattern."""
    return Fr(struct.unpack("<f", struct.pack("<I", bits))[0])


def aces(X):
    m = (X * (Fr("2.51") * X + Fr("0.03"))) / (X * (Fr("2.43") * X + Fr("0.59")) + Fr("0.14"))
    return min(max(m, Fr(0)), Fr(1))


def byte_ge(X, k):
    """byte(X) >= k for a mapped value 0 < X, 1 <= k <= 255."""
    if X <= KNEE:
        return LIN * X >= Fr(2 * k - 1, 2)
    return X ** 5 >= _B12[k]


def exact_byte(X, toon):
    """The byte of the rational X."""
    X = Fr(X)
    if toon:
        X = aces(X)
    if X <= 0:
        return 0  # v <= 0: rounds to <= 0, clamped
    if X >= 1:
        return 255  # v(1) = 255
    lo, hi = 0, 255  # the largest k with byte >= k
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if byte_ge(X, mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def exact_byte_special(x, toon):
    """+-inf and NaN, which are no rationals.  NaN is 0 (Rust's saturating
    `as u8`); without ACES -inf is 0 and +inf 255.  With ACES the reference's
    f64 arithmetic (color.rs:14-25) makes inf * inf / inf = NaN of either
    infinity, which f64::clamp keeps: 0, by the NaN rule."""
    if x != x or toon:
        return 0
    return 255 if x > 0 else 0


def is_decided(X, toon):
    X = Fr(X)
    return exact_byte(X * (1 - EPS), toon) == exact_byte(X * (1 + EPS), toon)


@functools.lru_cache(maxsize=None)
def thresholds(toon):
    """thr[k - 1] = the bit pattern of the smallest f32 X >= 0 with byte(X) >= k,
    k = 1 .. 255 (ascending)."""
    out = []
    top = 0x7F7FFFFF
    for k in range(1, 256):
        lo, hi = 0, top  # byte(lo) < k <= byte(hi)
        assert exact_byte(f32_bits_to_fraction(hi), toon) >= k
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if exact_byte(f32_bits_to_fraction(mid), toon) >= k:
                hi = mid
            else:
                lo = mid
        out.append(hi)
    assert all(a < b for a, b in zip(out, out[1:]))
    return tuple(out)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def expected(x, toon):
    """(bytes, undecided) for an f32 array x of finite values."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    thr = np.array(thresholds(toon), dtype=np.uint32)
    want = np.zeros(x.shape, dtype=np.int64)
    undecided = np.zeros(x.shape, dtype=bool)
    b = _bits(x)
    neg = (b >> 31).astype(bool) & (x != 0)
    pos = ~neg
    # non-negative values order as their bit patterns do (-0.0 counts as 0)
    bp = np.where(x == 0, np.uint32(0), b)[pos]
    want[pos] = np.searchsorted(thr, bp, side="right")
    # X (1 +- 2^-40) lies strictly between X's f32 neighbours, so only a
    # threshold and the f32 just below it can be undecided: those exactly
    cand = np.concatenate([thr, thr - 1])
    und_bits = np.array([c for c in cand if not is_decided(f32_bits_to_fraction(int(c)), toon)], dtype=np.uint32)
    undecided[pos] = np.isin(bp, und_bits)
    for i in np.flatnonzero(neg):
        X = Fr(float(x[i]))
        want[i] = exact_byte(X, toon)
        undecided[i] = not is_decided(X, toon)
    return want, undecided


def neighbours(bits, ulps):
    """The f32 bit patterns within `ulps` of each of `bits` (positive values)."""
    d = np.arange(-ulps, ulps + 1, dtype=np.int64)
    v = (np.asarray(bits, dtype=np.int64)[:, None] + d[None, :]).ravel()
    return v[(v >= 0) & (v <= 0x7F7FFFFF)].astype(np.uint32)


EDGES = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1e-3, -1.0, 1.0, np.nextafter(np.float32(1), np.float32(0)),
                  np.nextafter(np.float32(1), np.float32(2)), 2.0, 1e30], dtype=np.float32)


def boundary_inputs(toon):
    """The +-64-ulp neighbourhood of every byte threshold, the +-4-ulp
    neighbourhood of the knee, and the finite edge values."""
    knee = int(_bits(np.array([0.0031308], dtype=np.float32))[0])
    b = np.concatenate([neighbours(thresholds(toon), 64), neighbours([knee], 4)])
    return np.concatenate([b.view(np.float32), EDGES])


def random_inputs(n, seed=2025):
    """n random f32 bit patterns in [0, 4]."""
    rng = np.random.default_rng(seed)
    four = int(_bits(np.array([4.0], dtype=np.float32))[0])
    return rng.integers(0, four + 1, n, dtype=np.uint32).view(np.float32)


def f64_formula(x, toon):
    """The formula as the oracle and the kernel evaluate it, in numpy f64."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        if toon:
            m = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14)
            x = np.where(m < 0.0, 0.0, np.where(m > 1.0, 1.0, m))
        sv = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(np.maximum(x, 0.0), 1.0 / 2.4) - 0.055)
        v = sv * 255.0
        fl = np.floor(np.abs(v))
        q = np.copysign(fl + ((np.abs(v) - fl) >= 0.5), v)  # round half away from zero
        return np.clip(q, 0.0, 255.0).astype(np.int64)
