// rt_slab.h -- the conservative f32 box test every kernel tier walks with.
//
// Host and device: the kernels' walk (rt_walk.h, rt_walk4.h) runs it, and the
// CPU property test (tests/test_slab_cpu.py, tests/cpp/slab_prop.cpp) checks
// it against the slab test of aabb.rs:62-78 evaluated in extended precision.
// The basic tier walks with the sign-ordered form of the same test (RaySF,
// slab_sorted_f at the end of this file; tests/test_slab_sorted_cpu.py).
//
// aabb.rs:62-78: per axis t0 = (lo - o) / d, t1 = (hi - o) / d, the interval
// [min, max] of the two intersected with the ray's [t_min, t_max]; a hit when
// the result is not empty (inclusive).  Here in f32, made conservative --
// whenever the exact test on the exact box admits part of [t_min, c], this one
// does too:
//  - boxes are stored rounded outward (rth flatten / bvh4_convert);
//  - the origin's f32 rounding (and the rounding of o * idf) is absorbed by
//    widening the slab by pad = 2^-22 |o| per axis in space (RayF::nlo/nhi);
//  - the fma and 1/d roundings (relative, < 3u) by widening the t-interval
//    by 2^-22 |t| (REL);
//  - 1/d is clamped to |.| <= 2^60 so a zero direction component gives huge
//    finite t (the reference's +-inf) instead of inf - inf = NaN.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

namespace rtk {

#ifndef RT_SLAB_FOLD
#define RT_SLAB_FOLD 1
#endif
// 1/d of the f32 ray: 2 = the hardware reciprocal (below; C2 -1.3 % kernel
// time against 1, C4 +-0, A/B at 128 spp, RMSE 0), 1 = the correctly rounded
// f32 quotient of d rounded to f32, 0 = the f64 quotient rounded once
#ifndef RT_RCP_F32
#define RT_RCP_F32 2
#endif

// RT_RCP_F32 == 2: 1/x as the hardware reciprocal (v_rcp_f32, within 1 ulp
// of 1/x: the correctly rounded quotient or its neighbour) instead of the
// ~10-instruction IEEE division.  Host builds (the CPU property tests) cannot
// run v_rcp_f32, so they take the correctly rounded quotient moved one ulp in
// the direction RT_RCP_EMU (+1 up, -1 down, 0 none): the tests run both, which
// covers whatever the hardware returns -- tests/test_walk_filters_gpu.py holds
// the device to that over the whole normal range (measured: worst 0.88 ulp).
// (Results below 2^-126 flush to zero on the device: |d| >= 2^126 does not
// occur for a ray direction.  A subnormal x gives +-inf there as on the host,
// which make_rayf clamps like the reciprocal of zero.)
#ifndef RT_RCP_EMU
#define RT_RCP_EMU 0
#endif
RT_HD float rcp_f32(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    const float q = 1.0f / x;
    return RT_RCP_EMU > 0 ? std::nextafter(q, __builtin_huge_valf())
                          : RT_RCP_EMU < 0 ? std::nextafter(q, -__builtin_huge_valf()) : q;
#endif
}

// The f32 square root of the sphere filter's per-ray data (make_sphf, with
// RT_RCP_F32 == 2): the hardware's on the device (v_sqrt_f32: the correctly
// rounded root or a neighbour over the normal range, measured worst 0.92 ulp,
// tests/test_walk_filters_gpu.py; a subnormal argument gives 0, |d| < 2^-63),
// the correctly rounded one on the host.  The result goes out by reference:
// a returned float carries clang's `noundef` onto the inlined call, which
// changes the basic tier's code (a freeze dropped) for no measured gain.
RT_HD void sqrt_f32(float x, float& r) {
#if defined(__HIP_DEVICE_COMPILE__)
    r = __builtin_amdgcn_sqrtf(x);
#else
    r = std::sqrt(x);
#endif
}

#if RT_SLAB_FOLD
// The t-interval widening folded into the ray: the plane distances of the
// near planes (lo when 1/d > 0) are scaled by 1 - 2^-21, those of the far
// planes by 1 + 2^-21, so the box's entry is moved earlier and its exit later
// by that relative amount whenever they are positive -- the only case where
// they decide a hit (a negative entry is clamped to t_min, a negative exit
// misses either way).  The scalings' own roundings are covered by the doubled
// widths: pad = 2^-21 |o| in space, 2^-21 relative in t.
struct RayF {
    float idl[3], idh[3];  // 1/d scaled for the lo and hi planes
    float nlo[3];          // -(o + pad) * idl  (lo planes moved outward)
    float nhi[3];          // -(o - pad) * idh  (hi planes moved outward)
};

RT_HD RayF make_rayf(const double o[3], const double d[3]) {
    RayF R;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#if RT_RCP_F32 == 2
        // d rounded to f32, then the hardware reciprocal: < 2.01u relative,
        // common to both plane distances of the axis (a relative error of t,
        // inside the 2^-21 widening with the other roundings; the CPU test
        // holds it there with the quotient moved an ulp either way)
        float f = rcp_f32((float)d[k]);
#elif RT_RCP_F32
        // d rounded to f32, then the correctly rounded f32 quotient: < 1.01u
        // relative (the f64 quotient rounded once: 0.5u).  The error is
        // common to both plane distances of the axis, a relative error of t,
        // inside the 2^-21 widening with the other roundings.
        float f = 1.0f / (float)d[k];
#else
        float f = (float)(1.0 / d[k]);
#endif
        if (!(fabsf(f) <= 1.152921504606847e18f)) f = copysignf(1.152921504606847e18f, f);
        const float of = (float)o[k];
        const float pad = fabsf(of) * 4.76837158203125e-07f + 1e-30f;  // 2^-21 |o|
        constexpr float SHRINK = 1.0f - 4.76837158203125e-07f, GROW = 1.0f + 4.76837158203125e-07f;
        const float sl = f > 0.0f ? SHRINK : GROW, sh = f > 0.0f ? GROW : SHRINK;
        R.idl[k] = f * sl;
        R.idh[k] = f * sh;
        R.nlo[k] = -((of + pad) * f) * sl;
        R.nhi[k] = -((of - pad) * f) * sh;
    }
    return R;
}
#else
struct RayF {
    float idf[3];  // 1/d
    float nlo[3];  // -(o + pad) * idf  (lo planes moved outward)
    float nhi[3];  // -(o - pad) * idf  (hi planes moved outward)
};

RT_HD RayF make_rayf(const double o[3], const double d[3]) {
    RayF R;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double id = 1.0 / d[k];
        float f = (float)id;
        if (!(fabsf(f) <= 1.152921504606847e18f)) f = copysignf(1.152921504606847e18f, (float)id);
        const float of = (float)o[k];
        const float pad = fabsf(of) * 2.384185791015625e-07f + 1e-30f;
        R.idf[k] = f;
        R.nlo[k] = -((of + pad) * f);
        R.nhi[k] = -((of - pad) * f);
    }
    return R;
}
#endif

// f32 not above x (round to nearest, then one ulp down when that rounded up)
RT_HD float f32_down(double x) {
    float f = (float)x;
    if ((double)f > x) {
        union {
            float f;
            uint32_t u;
        } b{f};
        b.u = (f > 0.0f) ? b.u - 1u : (f == 0.0f ? 0x80000001u : b.u + 1u);
        f = b.f;
    }
    return f;
}

// Closest-hit state of one traversal: t and its f32 upper bound.
struct Closest {
    double c;
    float c_f;
    // c_f = (float)t plus at least one ulp: an upper bound of t in two
    // instructions (|f| * 2^-23 >= 1 ulp of f, and (float)t is within half an
    // ulp), where the exact round-up takes a compare-and-step sequence.
    RT_HD void set(double t) {
        c = t;
        const float f = (float)t;
        c_f = fmaf(fabsf(f), 1.1920928955078125e-07f, f);
    }
    // a hit t <= c that never loosens c_f (basic tier's sphere rounds)
    RT_HD void lower(double t) {
        c = t;
        const float f = (float)t;
        c_f = fminf(c_f, fmaf(fabsf(f), 1.1920928955078125e-07f, f));
    }
};

// The f32 box of a basic-tier sphere child {cx, cy, cz, r} (rth::bvh4_convert):
// the walk slab-tests it and runs the exact f64 Sphere::hit (sphere.rs:77-108)
// only on a hit, so the box must hold every point that test can return -- and
// the f64 test has a slop of its own.  With u = 2^-53 and M = 2 |c - o| + r its
// discriminant is off by less than 32 u |d|^2 M^2, so a root it accepts lies
// within r + 16 u M^2 / r of the centre: outside the sphere by a hair when
// the ray grazes it.  Where the graze is at a pole, on a face of the exact box,
// and the f32 roundings happen to leave no slack (c +- r exact in f32, the
// origin's coordinate zero), a ray in that face's plane would be culled and
// the image change.  So the radius is widened before rounding outward, by the
// larger of
//   2^-16 r: the slop for every origin within 4.6e4 radii of the centre
//     (2^-16 >= 16 u (M / r)^2 for M / r <= 2^16.5), which is every sphere of
//     an ordinary world and costs no measurable false positives, and
//   16 u (2 reach + r)^2 / r: the slop for every origin within reach of the
//     centre.  The flatten passes the diagonal of the world's bounding box, so
//     this holds for every scattered ray, whose origin lies on a surface of
//     the world; it is the larger term only for a sphere more than 2.3e4 times
//     smaller than the world.
// A sphere so small that the pad would exceed reach (r = 0 included) gets
// c -+ (r + reach), which holds the whole world: a ray from inside it always
// hits.  What is left to the caller is the camera: a primary ray's origin
// outside the world's box is covered only within max(reach, 4.6e4 r) of the
// centre.  tests/test_sphere_box_cpu.py holds the property.
RT_HD void sphere_box_f(const double s[4], double reach, float lo[3], float hi[3]) {
    const double r = s[3], M = 2.0 * reach + r;
    double pad = r * 0x1p-16;
    const double far = 0x1p-49 * M * M / r;  // 16 u M^2 / r
    if (far > pad) pad = far;
    if (!(pad <= reach)) pad = reach;  // (also r = 0: far is inf or NaN)
    if (!(pad >= r * 0x1p-16)) pad = r * 0x1p-16;  // (reach < 2^-16 r: a one-sphere world)
    const double m = r + pad;
    for (int k = 0; k < 3; ++k) {
        lo[k] = f32_down(s[k] - m);
        hi[k] = -f32_down(-(s[k] + m));
    }
}

// Entry distance (clamped to t_min) and hit of box [lo, hi] for t in [tmin_f, c_f].
RT_HD bool slab_f(const float* lo, const float* hi, const RayF& R, float tmin_f, float c_f, float& entry) {
#if RT_SLAB_FOLD
    const float tlx = fmaf(lo[0], R.idl[0], R.nlo[0]), thx = fmaf(hi[0], R.idh[0], R.nhi[0]);
    const float tly = fmaf(lo[1], R.idl[1], R.nlo[1]), thy = fmaf(hi[1], R.idh[1], R.nhi[1]);
    const float tlz = fmaf(lo[2], R.idl[2], R.nlo[2]), thz = fmaf(hi[2], R.idh[2], R.nhi[2]);
    entry = fmaxf(fmaxf(fmaxf(fminf(tlx, thx), fminf(tly, thy)), fminf(tlz, thz)), tmin_f);
    return entry <= fminf(fminf(fminf(fmaxf(tlx, thx), fmaxf(tly, thy)), fmaxf(tlz, thz)), c_f);
#else
    const float tlx = fmaf(lo[0], R.idf[0], R.nlo[0]), thx = fmaf(hi[0], R.idf[0], R.nhi[0]);
    const float tly = fmaf(lo[1], R.idf[1], R.nlo[1]), thy = fmaf(hi[1], R.idf[1], R.nhi[1]);
    const float tlz = fmaf(lo[2], R.idf[2], R.nlo[2]), thz = fmaf(hi[2], R.idf[2], R.nhi[2]);
    const float nr = fmaxf(fmaxf(fminf(tlx, thx), fminf(tly, thy)), fminf(tlz, thz));
    const float fr = fminf(fminf(fmaxf(tlx, thx), fmaxf(tly, thy)), fmaxf(tlz, thz));
    constexpr float REL = 2.384185791015625e-07f;  // 2^-22
    entry = fmaxf(fmaf(-fabsf(nr), REL, nr), tmin_f);
    return entry <= fminf(fmaf(fabsf(fr), REL, fr), c_f);
#endif
}

#if RT_SLAB_FOLD
// The same test with the min / max pairing of an axis' two plane distances
// done once per ray (the basic tier's visit4_rows): make_rayf already scales
// the lo planes as the near ones where 1/d > 0 and the hi planes otherwise, so
// the ray knows which plane of an axis it meets first.  RaySF holds the
// coefficient pairs in that order and the caller hands the box's planes over
// in it: near[k] = pos[k] ? lo[k] : hi[k], far[k] the other.  The six plane
// distances are the very values slab_f computes.  Where an axis has near <=
// far -- always, when the box is not wholly behind the origin on that axis --
// slab_f's min / max return them as they stand and both tests give the same
// entry and verdict.  Where rounding leaves near > far (both negative: the
// slab lies behind the origin, and the two scalings move the planes apart the
// other way), slab_f has exit <= max(near, far) < 0 < t_min <= entry and this
// one entry >= near > far >= exit: both miss.  tests/test_slab_sorted_cpu.py
// holds the agreement, bit for bit.
struct RaySF {
    float idn[3], nn[3];  // the near planes' coefficient pair (RayF's idl, nlo where pos)
    float idf[3], nf[3];  // the far planes'
    bool pos[3];          // 1/d > 0: the lo plane is the near one
};

// make_rayf's clamped 1/d of one axis, the same expression
RT_HD float rayf_inv(double dk) {
#if RT_RCP_F32 == 2
    float f = rcp_f32((float)dk);
#elif RT_RCP_F32
    float f = 1.0f / (float)dk;
#else
    float f = (float)(1.0 / dk);
#endif
    if (!(fabsf(f) <= 1.152921504606847e18f)) f = copysignf(1.152921504606847e18f, f);
    return f;
}

// make_rayf(o, d) with each axis' two pairs in the ray's order, by make_rayf's
// own predicate f > 0: {idn, nn} = pos ? {idl, nlo} : {idh, nhi}, {idf, nf}
// the other pair, bit for bit (tests/cpp/slab_sorted_prop.cpp compares them).
// Written out, not selected from a RayF: the near plane's scale is 1 - 2^-21
// and the far plane's 1 + 2^-21 whatever the sign, and only the pad changes
// sides -- one select an axis where picking from make_rayf's result takes
// four on top of make_rayf's two (which the compiler does not fold).
RT_HD RaySF make_raysf(const double o[3], const double d[3]) {
    RaySF Q;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = rayf_inv(d[k]);
        const bool p = f > 0.0f;
        const float of = (float)o[k];
        const float pad = fabsf(of) * 4.76837158203125e-07f + 1e-30f;  // 2^-21 |o|
        const float pn = p ? pad : -pad;  // the lo plane moves down, the hi plane up
        constexpr float SHRINK = 1.0f - 4.76837158203125e-07f, GROW = 1.0f + 4.76837158203125e-07f;
        Q.pos[k] = p;
        Q.idn[k] = f * SHRINK;
        Q.idf[k] = f * GROW;
        Q.nn[k] = -((of + pn) * f) * SHRINK;
        Q.nf[k] = -((of - pn) * f) * GROW;
    }
    return Q;
}

RT_HD bool slab_sorted_f(const float* near, const float* far, const RaySF& Q, float tmin_f, float c_f, float& entry) {
    const float tnx = fmaf(near[0], Q.idn[0], Q.nn[0]), tfx = fmaf(far[0], Q.idf[0], Q.nf[0]);
    const float tny = fmaf(near[1], Q.idn[1], Q.nn[1]), tfy = fmaf(far[1], Q.idf[1], Q.nf[1]);
    const float tnz = fmaf(near[2], Q.idn[2], Q.nn[2]), tfz = fmaf(far[2], Q.idf[2], Q.nf[2]);
    entry = fmaxf(fmaxf(fmaxf(tnx, tny), tnz), tmin_f);
    return entry <= fminf(fminf(fminf(tfx, tfy), tfz), c_f);
}
#endif

}  // namespace rtk
