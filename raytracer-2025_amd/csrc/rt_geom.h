// rt_geom.h -- the ray, the exact f64 geometry tests, Transform's maps and
// what a walk records of its closest hit.
#pragma once
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_slab.h"

namespace rtk {

struct Ray {
    D3 o, d;
    double time;
};

// ------------------------------------------------------------------ geometry tests
__device__ __forceinline__ RayF make_rayf(const Ray& r) {
    const double o[3] = {r.o.x, r.o.y, r.o.z}, d[3] = {r.d.x, r.d.y, r.d.z};
    return make_rayf(o, d);
}

// sphere.rs:77-96 -- t of the accepted root, or false
__device__ __forceinline__ bool sphere_t(D3 c, double radius, const Ray& r, double a, double tmin, double tmax,
                                         double& t) {
    const D3 oc = c - r.o;
    const double h = dot(r.d, oc);
    const double cc = len2(oc) - radius * radius;
    const double disc = h * h - a * cc;
    if (disc < 0.0) return false;
    const double sq = k_sqrt(disc);
    double root = (h - sq) / a;
    if (!(root >= tmin && root <= tmax)) {
        root = (h + sq) / a;
        if (!(root >= tmin && root <= tmax)) return false;
    }
    t = root;
    return true;
}

// num / a for a ray's a = |d|^2 with the correctly rounded inva = 1/a computed
// once per ray: q = num*inva is within 1 ulp, the FMA residual is exact, and
// the corrected quotient is the correctly rounded num / a (Markstein) -- the
// value sphere.rs:88-92's division gives, for 3 instructions instead of 10.
__device__ __forceinline__ double div_a(double num, double a, double inva) {
    const double q = num * inva;
    const double r = fma(-q, a, num);
    return fma(r, inva, q);
}
__device__ __forceinline__ bool sphere_t_inv(D3 c, double radius, const Ray& r, double a, double inva, double tmin,
                                             double tmax, double& t) {
    const D3 oc = c - r.o;
    const double h = dot(r.d, oc);
    const double cc = len2(oc) - radius * radius;
    const double disc = h * h - a * cc;
    if (disc < 0.0) return false;
    const double sq = k_sqrt(disc);
    double root = div_a(h - sq, a, inva);
    if (!(root >= tmin && root <= tmax)) {
        root = div_a(h + sq, a, inva);
        if (!(root >= tmin && root <= tmax)) return false;
    }
    t = root;
    return true;
}

// quad.rs:71-102 / triangle.rs:69-98 on the record's values: unit normal n,
// parm_d D, anchor Q, edges u / v, w = n / |n|^2
__device__ __forceinline__ bool planar_t_v(const D3 n, const double D, const D3 Q, const D3 u, const D3 v, const D3 w,
                                           bool tri, const Ray& r, double tmin, double tmax, double& t) {
    const double denom = dot(n, r.d);
    if (fabs(denom) < 1e-8) return false;
    const double num = D - dot(n, r.o);
    const double tt = num / denom;
    if (!(tt >= tmin && tt <= tmax)) return false;
    const D3 hv = (r.o + tt * r.d) - Q;
    const double alpha = dot(w, cross(hv, v));
    const double beta = dot(w, cross(u, hv));
    if (!(alpha >= 0.0 && alpha <= 1.0 && beta >= 0.0 && beta <= 1.0)) return false;
    if (tri) {
        const double ab = alpha + beta;
        if (!(ab >= 0.0 && ab <= 1.0)) return false;
    }
    t = tt;
    return true;
}
// quad.rs:71-102 / triangle.rs:69-98
__device__ __forceinline__ bool planar_t(const DPlanar& P, bool tri, const Ray& r, double tmin, double tmax,
                                         double& t) {
    return planar_t_v(d3(P.f[0], P.f[1], P.f[2]), P.f[3], d3(P.f[4], P.f[5], P.f[6]), d3(P.f[7], P.f[8], P.f[9]),
                      d3(P.f[10], P.f[11], P.f[12]), d3(P.f[13], P.f[14], P.f[15]), tri, r, tmin, tmax, t);
}

// Quaternion::rotate_vector (quaternion.rs:72-82): (q * (0, v)) * conj(q)
// with Mul (quaternion.rs:94-103) term by term in the reference's order; the
// products with qv.w = 0 are exact zeros, so a + 0*b is a and those terms
// are left out without changing a bit.
__device__ __forceinline__ D3 quat_rotate(double w, double x, double y, double z, D3 v) {
    const double pw = ((-(x * v.x)) - y * v.y) - z * v.z;
    const double px = (w * v.x + y * v.z) - z * v.y;
    const double py = (w * v.y - x * v.z) + z * v.x;
    const double pz = (w * v.z + x * v.y) - y * v.x;
    const double cx = -x, cy = -y, cz = -z;  // conjugate
    return d3(((pw * cx + px * w) + py * cz) - pz * cy, ((pw * cy - px * cz) + py * w) + pz * cx,
              ((pw * cz + px * cy) - py * cx) + pz * w);
}
// Transform::detransform (shapes.rs:80-84): conj(q).rotate_vector(v - offset) / scale
// 1: a Transform whose scale is exactly (1, 1, 1) (the reference's `None`,
// every Transform of C3 and C5) skips the three f64 divisions: x / 1.0 is x,
// bit for bit, NaN, infinities and signed zeros included
__device__ __forceinline__ D3 xf_in(const DXform& X, D3 v) {
    const D3 p = quat_rotate(X.q[0], -X.q[1], -X.q[2], -X.q[3], v - d3(X.off[0], X.off[1], X.off[2]));
    if (X.flags & XF_UNIT_SCALE) return p;
    return p / d3(X.scale[0], X.scale[1], X.scale[2]);
}
// Transform::transform (shapes.rs:74-78): q.rotate_vector(v * scale) + offset
__device__ __forceinline__ D3 xf_out(const DXform& X, D3 v) {
    return quat_rotate(X.q[0], X.q[1], X.q[2], X.q[3], v * d3(X.scale[0], X.scale[1], X.scale[2])) +
           d3(X.off[0], X.off[1], X.off[2]);
}
// shapes.rs:93-99 local ray
__device__ __forceinline__ Ray xf_ray(const DXform& X, const Ray& r) {
    const D3 lo = xf_in(X, r.o);
    const D3 lt = xf_in(X, r.o + 1.0 * r.d);
    return Ray{lo, lt - lo, r.time};
}

// The Transforms entered on the way to a hit, innermost last.  Two named
// fields, not an array: a dynamically indexed private array is placed in
// scratch memory by the compiler.
struct XfIds {
    uint32_t a = 0, b = 0;
    __device__ __forceinline__ uint32_t get(uint32_t k) const { return k == 0 ? a : b; }
    __device__ __forceinline__ void set(uint32_t k, uint32_t v) {
        if (k == 0)
            a = v;
        else
            b = v;
    }
};

struct HitInfo {
    double t;
    uint32_t ref;
    uint32_t nxf;
    XfIds xf;
};

}  // namespace rtk
