// rt_primary.h -- the basic tier's primary-ray candidates: a conservative test
// of "can any camera ray of this pixel hit this sphere", and the shape of the
// per-launch table the test fills.
//
// Host and device: the table kernel (rt_kernel_common.hip rt_primary_kernel)
// and the path kernel's basic tier (rt_kernel_path.hip) use it, and the CPU
// property test (tests/test_primary_beam_cpu.py, tests/cpp/primary_beam_prop.cpp)
// holds the verdict against brute force.
//
// Camera::get_ray (camera.rs:247-273) makes, for pixel (px, py), the rays
//   o = center + a disk_u + b disk_v,  a^2 + b^2 <= 1   (o = center without defocus)
//   p = pixel00 + (px + ox) du + (py + oy) dv,  ox, oy in [-0.5, 0.5]
//   x(t) = o + t (p - o) = (1 - t) o + t p
// Against the central ray x0(t) = (1 - t) center + t p0 (p0 the footprint's
// centre) a point of any of them lies within
//   |x(t) - x0(t)| <= |1 - t| Rl + t Rp      (t >= 0)
// with Rl >= |a disk_u + b disk_v| (sqrt(|disk_u|^2 + |disk_v|^2): no
// orthogonality assumed) and Rp >= |ox du + oy dv| (hx |du| + hy |dv|).  So a
// ray of the set comes within rho of a sphere's centre c only if, for some
// t >= 0,  |center - c + t (p0 - center)| <= rho + |1 - t| Rl + t Rp:  two
// quadratics in t, one on [0, 1] and one on [1, inf), each decided from its
// end points and its vertex.
//
// What makes the verdict safe for the f64 Sphere::hit (sphere.rs:77-108) as
// the kernel runs it, the way sphere_box_f (rt_slab.h) pads its box:
//  - rho = r + the test's own slop at a grazing ray: a root it accepts lies
//    within r + 16 u M^2 / r of the centre (u = 2^-53, M = 2 |c - o| + r), and
//    at least 2^-16 r is added; the accepted root is >= t_min > 0, so the
//    point at it is a witness with t >= 0;
//  - the camera's own roundings (the origin, the target, cos^2 + sin^2 and
//    (s + xi) / sqrt_spp a hair past their ranges) by Rl and Rp widened by
//    2^-30 relative and rho by 2^-40 of the sum of the magnitudes that make
//    the ray;
//  - this file's roundings by deciding "cannot hit" only where a quadratic is
//    above 2^-40 of the sum of its terms' magnitudes (they err by a few 2^-53
//    of it), and by saying "may hit" where a vertex is ill-conditioned;
//  - every comparison is written so that a NaN gives "may hit"; r = 0 and a
//    pad that is not finite give "may hit".
// A loose bound only costs exact tests; a wrong "cannot hit" changes the image.
#pragma once
#include <cmath>
#include <cstdint>

#include "rt_slab.h"

namespace rtk {

// ------------------------------------------------------------------ the table
// CAP 16-bit sphere indices per pixel of the launch's rows (launch pixel =
// shard row * W + px), ascending, the unused slots PRIMARY_NONE; a pixel with
// more than CAP candidates holds PRIMARY_WALK in slot 0 and its primary rays
// walk the tree.  Eight slots are one 16-byte load.  (C2 at 1920x1080: the
// histogram is profiles/r18/primary_table_hist_c2.json.)
#ifndef RT_PRIMARY_CAP
#define RT_PRIMARY_CAP 8
#endif
constexpr uint32_t PRIMARY_CAP = RT_PRIMARY_CAP;
static_assert(PRIMARY_CAP == 8, "the path kernel reads a pixel's slots as one uint4");
constexpr uint32_t PRIMARY_NONE = 0xfffeu, PRIMARY_WALK = 0xffffu;
// sphere indices are 15 bits in the basic tier (rt_stack.h bword), below both marks
constexpr uint32_t PRIMARY_MAX_SPHERES = 32768u;
// the table kernel works on tiles of launch pixels: a tile's spheres first,
// then each pixel's among them
constexpr uint32_t PRIMARY_TILE = 16u;

RT_HD uint64_t primary_table_slots(uint32_t W, uint32_t rows) { return (uint64_t)W * rows * PRIMARY_CAP; }
RT_HD uint64_t primary_table_bytes(uint32_t W, uint32_t rows) { return primary_table_slots(W, rows) * sizeof(uint16_t); }
// the image row of a shard's row, and back (py must be a row of the shard)
RT_HD uint32_t primary_image_row(uint32_t prow, uint32_t row_offset, uint32_t row_stride) {
    return row_offset + prow * row_stride;
}
RT_HD uint32_t primary_shard_row(uint32_t py, uint32_t row_offset, uint32_t row_stride) {
    return (py - row_offset) / row_stride;
}
// first slot of image pixel (px, py) in the shard's table
RT_HD uint64_t primary_table_index(uint32_t W, uint32_t px, uint32_t py, uint32_t row_offset, uint32_t row_stride) {
    return ((uint64_t)primary_shard_row(py, row_offset, row_stride) * W + px) * PRIMARY_CAP;
}
RT_HD uint32_t primary_tiles(uint32_t n) { return (n + PRIMARY_TILE - 1u) / PRIMARY_TILE; }

// ------------------------------------------------------------------ the beam
// the Frame's camera fields
struct BeamCam {
    double center[3], disk_u[3], disk_v[3], pixel00[3], du[3], dv[3];
    uint32_t defocus;
};

// the rays of a footprint: targets pixel00 + (fx + x) du + (fy + y) dv with
// |x| <= hx, |y| <= hy (a pixel: its centre and 0.5, 0.5)
struct Beam {
    double o[3], D[3];  // the central ray: center, p0 - center
    double DD;          // |D|^2
    double Rl, Rp;      // the lens' and the footprint's radius, widened
    double pad;         // the camera's roundings, added to a sphere's radius
};

RT_HD double beam_len(const double v[3]) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
RT_HD double beam_abs1(const double v[3]) { return std::fabs(v[0]) + std::fabs(v[1]) + std::fabs(v[2]); }

RT_HD Beam make_beam(const BeamCam& C, double fx, double fy, double hx, double hy) {
    constexpr double WIDE = 1.0 + 0x1p-30;
    Beam B;
    for (int k = 0; k < 3; ++k) {
        B.o[k] = C.center[k];
        B.D[k] = ((C.pixel00[k] + fx * C.du[k]) + fy * C.dv[k]) - C.center[k];
    }
    B.DD = B.D[0] * B.D[0] + B.D[1] * B.D[1] + B.D[2] * B.D[2];
    const double lu = beam_len(C.disk_u), lv = beam_len(C.disk_v);
    B.Rl = C.defocus ? std::sqrt(lu * lu + lv * lv) * WIDE : 0.0;
    B.Rp = (hx * beam_len(C.du) + hy * beam_len(C.dv)) * WIDE;
    B.pad = 0x1p-40 * (beam_abs1(C.center) + beam_abs1(C.pixel00) + (std::fabs(fx) + hx + 1.0) * beam_abs1(C.du) +
                       (std::fabs(fy) + hy + 1.0) * beam_abs1(C.dv) + beam_abs1(C.disk_u) + beam_abs1(C.disk_v));
    return B;
}

// May some t of [t0, t1] (open: of [t0, inf)) have |E + t D| <= al + be t?
// (al + be t >= 0 on the interval.)  EE, ED, DD: the dot products.
RT_HD bool beam_piece(double EE, double ED, double DD, double al, double be, double t0, double t1, bool open) {
    constexpr double K = 0x1p-40, KA = 0x1p-10;
    const double A = DD - be * be, Bh = ED - al * be, Cc = EE - al * al;
    const double mA = DD + be * be, mB = std::fabs(ED) + std::fabs(al * be), mC = EE + al * al;
    // f(t) = A t^2 + 2 Bh t + Cc certainly above zero
    auto clear = [&](double t) {
        const double f = (A * t + 2.0 * Bh) * t + Cc;
        const double m = (mA * t + 2.0 * mB) * t + mC;
        return f > K * m;
    };
    if (!clear(t0)) return true;
    if (!open && !clear(t1)) return true;
    // concave or linear: the least value is at an end -- the far end of the
    // open piece is below zero (or as good as)
    if (!(A > 0.0)) return open;
    if (!(A > KA * mA)) return true;  // the vertex is ill-conditioned
    const double tv = -Bh / A;
    if (tv > t0 && (open || tv < t1)) return !clear(tv);
    return false;
}

// false: no ray of the beam has a root of the f64 Sphere::hit on sphere
// s = {cx, cy, cz, r} in [t_min, inf), t_min > 0.  true: it may have one.
RT_HD bool beam_may_hit(const Beam& B, const double s[4]) {
    const double r = std::fabs(s[3]);
    if (!(r > 0.0)) return true;  // r = 0 (and NaN)
    const double E[3] = {B.o[0] - s[0], B.o[1] - s[1], B.o[2] - s[2]};
    const double EE = E[0] * E[0] + E[1] * E[1] + E[2] * E[2];
    const double ED = E[0] * B.D[0] + E[1] * B.D[1] + E[2] * B.D[2];
    const double M = 2.0 * (std::sqrt(EE) + B.Rl) + r;
    double slop = r * 0x1p-16;
    const double far = 0x1p-49 * M * M / r;  // 16 u M^2 / r
    if (!(far <= slop)) slop = far;          // (the larger; a NaN is taken and caught below)
    const double rho = r + slop + B.pad;
    if (!(rho < __builtin_huge_val())) return true;
    // t in [0, 1]: rho + (1 - t) Rl + t Rp;  t >= 1: rho + (t - 1) Rl + t Rp
    if (beam_piece(EE, ED, B.DD, rho + B.Rl, B.Rp - B.Rl, 0.0, 1.0, false)) return true;
    return beam_piece(EE, ED, B.DD, rho - B.Rl, B.Rl + B.Rp, 1.0, 0.0, true);
}

}  // namespace rtk
