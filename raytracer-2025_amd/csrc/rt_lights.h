// rt_lights.h -- pdf_value and random of the lights (HittablePDF).
#pragma once
#include "rt_builds.h"
#include "rt_geom.h"
#include "rt_kernel.h"
#include "rt_math.h"

namespace rtk {

// ------------------------------------------------------------------ lights (pdf.rs:66-88)
__device__ double light_pdf_one(const SceneView& S, uint32_t ref, D3 o, D3 d) {
    const uint32_t kind = ref_kind(ref), idx = ref_idx(S, ref);
    const Ray r{o, d, 0.0};
    double t;
    if (kind == K_QUAD || kind == K_TRI) {  // quad.rs:108-120
        const DPlanar& P = S.planars[idx];
        if (!planar_t(P, kind == K_TRI, r, 1e-8, __builtin_huge_val(), t)) return 0.0;
        const D3 n = d3(P.f[0], P.f[1], P.f[2]);
        const D3 rn = dot(d, n) < 0.0 ? n : -n;
        const double distance_squared = t * t * len2(d);
        const double cosine = fabs(dot(d, rn) / len(d));
        return distance_squared / (cosine * S.planar_area[idx]);
    }
    if (kind == K_SPHERE) {  // sphere.rs:114-132
        const double4 s = S.spheres[idx];
        if (!sphere_t(d3(s.x, s.y, s.z), s.w, r, len2(d), 1e-8, __builtin_huge_val(), t)) return 0.0;
        const double dist_squared = len2(d3(s.x, s.y, s.z) - o);
        const double ctm = k_sqrt(1.0 - s.w * s.w / dist_squared);
        if (isnan(ctm)) return 1.0 / (4.0 * PI);
        return 1.0 / (2.0 * PI * (1.0 - ctm));
    }
    return 0.0;
}
__device__ double light_pdf(const SceneView& S, D3 o, D3 d) {
    const uint32_t root = S.lights_root;
    if (ref_kind(root) != K_LIST) return light_pdf_one(S, root, o, d);
    double sum = 0.0;  // hits.rs:52-67
    uint32_t n = 0;
    for (uint32_t i = ref_idx(S, root); S.list_children[i] != REF_NONE; ++i, ++n) sum += light_pdf_one(S, S.list_children[i], o, d);
    return sum / (double)n;
}
__device__ __forceinline__ D3 onb_world(D3 n, D3 v, bool& ok) {  // onb.rs:8-21, 34-38
    const D3 a = fabs(n.x) > 0.9 ? d3(0.0, 1.0, 0.0) : d3(1.0, 0.0, 0.0);
    const D3 u = unit(cross(n, a), ok);
    const D3 w = cross(u, n);
    return v.x * u + v.y * n + v.z * w;
}
// Quad / Triangle / Sphere::random (quad.rs:122-125, triangle.rs:117-128, sphere.rs:134-144)
__device__ __forceinline__ D3 light_random_one(const SceneView& S, uint32_t ref, D3 o, Rng& rng, uint32_t& ovf,
                                               bool& ok) {
    const uint32_t kind = ref_kind(ref), idx = ref_idx(S, ref);
    if (kind == K_QUAD || kind == K_TRI) {  // quad.rs:122-125, triangle.rs:117-128
        const DPlanar& P = S.planars[idx];
        double a = rng.next(ovf);
        double b = rng.next(ovf);
        if (kind == K_TRI && a + b > 1.0) {
            const double na = 1.0 - b, nb = 1.0 - a;
            a = na;
            b = nb;
        }
        const D3 p = d3(P.f[4], P.f[5], P.f[6]) + (a * d3(P.f[7], P.f[8], P.f[9])) + (b * d3(P.f[10], P.f[11], P.f[12]));
        return unit(p - o, ok);
    }
    // sphere.rs:134-144
    const double4 s = S.spheres[idx];
    const D3 direction = d3(s.x, s.y, s.z) - o;
    const double distance_squared = len2(direction);
    bool ok1, ok2;
    const D3 nd = unit(direction, ok1);
    const double r1 = rng.next(ovf), r2 = rng.next(ovf);
    const double y = 1.0 + r2 * (k_sqrt(1.0 - s.w * s.w / distance_squared) - 1.0);
    double sphi, cphi;
    k_sincos_2pi(r1, &sphi, &cphi);  // phi = 2.0 * PI * r1
    const double x = cphi * k_sqrt(1.0 - y * y), z = sphi * k_sqrt(1.0 - y * y);
    const D3 wv = onb_world(nd, d3(x, y, z), ok2);
    bool ok3;
    const D3 res = unit(wv, ok3);
    ok = ok1 && ok2 && ok3;
    return res;
}
__device__ D3 light_random(const SceneView& S, D3 o, Rng& rng, uint32_t& ovf, bool& ok) {
    uint32_t ref = S.lights_root;
    if (ref_kind(ref) == K_LIST) {  // hits.rs:69-75 choose
        uint32_t n = 0;
        for (uint32_t i = ref_idx(S, ref); S.list_children[i] != REF_NONE; ++i) ++n;
        uint32_t k = (uint32_t)(rng.next(ovf) * (double)n);
        if (k >= n) k = n - 1;
        ref = S.list_children[ref_index(ref) + k];
    }
    return light_random_one(S, ref, o, rng, ovf, ok);
}

// ---- general lights (tier FULL_GL): any tree of Hittables lists and
// Transforms over spheres (static or moving: pdf_value / random use the
// center at time 0, sphere.rs:114-144), quads and triangles.
// Hittables::pdf_value averages its children's values in order
// (hits.rs:52-67); Hittables::random draws one child (hits.rs:69-75);
// Transform maps the origin and direction into its frame and the sampled
// point back out (shapes.rs:117-132).  The tree is walked by compile-time
// recursion over its depth (the flattener rejects deeper trees), as a
// reference call chain would.
constexpr int RT_LIGHT_DEPTH = 4;  // list / Transform levels of a lights tree (rt_scene.cpp light_tree_ok)

__device__ double light_pdf_leaf(const SceneView& S, uint32_t ref, D3 o, D3 d) {
    if (ref_kind(ref) != K_MSPHERE) return light_pdf_one(S, ref, o, d);
    const double4 s = S.msph_center[ref_idx(S, ref)];  // Ray::new: time 0 (ray.rs:11-17) -> center.at(0)
    const Ray r{o, d, 0.0};
    double t;
    if (!sphere_t(d3(s.x, s.y, s.z), s.w, r, len2(d), 1e-8, __builtin_huge_val(), t)) return 0.0;
    const double dist_squared = len2(d3(s.x, s.y, s.z) - o);
    const double ctm = k_sqrt(1.0 - s.w * s.w / dist_squared);
    if (isnan(ctm)) return 1.0 / (4.0 * PI);
    return 1.0 / (2.0 * PI * (1.0 - ctm));
}

template <int D>
__device__ double light_pdf_tree(const SceneView& S, uint32_t ref, D3 o, D3 d, bool& panic) {
    const uint32_t kind = ref_kind(ref), idx = ref_idx(S, ref);
    if constexpr (D > 0) {
        if (kind == K_LIST) {  // hits.rs:52-67
            double sum = 0.0;
            uint32_t n = 0;
            for (uint32_t i = idx; S.list_children[i] != REF_NONE; ++i, ++n)
                sum += light_pdf_tree<D - 1>(S, S.list_children[i], o, d, panic);
            const double ret = sum / (double)n;
            if (isnan(ret)) panic = true;  // "The sum of pdf is NaN!"
            return ret;
        }
        if (kind == K_XFORM) {  // shapes.rs:117-123
            const DXform& X = S.xforms[idx];
            const D3 lo = xf_in(X, o);
            const D3 lt = xf_in(X, o + d);
            return light_pdf_tree<D - 1>(S, X.child, lo, lt - lo, panic);
        }
    }
    return light_pdf_leaf(S, ref, o, d);
}

template <int D>
__device__ D3 light_random_tree(const SceneView& S, uint32_t ref, D3 o, Rng& rng, uint32_t& ovf, bool& ok) {
    const uint32_t kind = ref_kind(ref), idx = ref_idx(S, ref);
    if constexpr (D > 0) {
        if (kind == K_LIST) {  // hits.rs:69-75 choose
            uint32_t n = 0;
            for (uint32_t i = idx; S.list_children[i] != REF_NONE; ++i) ++n;
            uint32_t k = (uint32_t)(rng.next(ovf) * (double)n);
            if (k >= n) k = n - 1;
            return light_random_tree<D - 1>(S, S.list_children[idx + k], o, rng, ovf, ok);
        }
        if (kind == K_XFORM) {  // shapes.rs:125-132
            const DXform& X = S.xforms[idx];
            const D3 lo = xf_in(X, o);
            const D3 ld = light_random_tree<D - 1>(S, X.child, lo, rng, ovf, ok);
            const D3 world_to = xf_out(X, lo + ld);
            bool ok2;
            const D3 res = unit(world_to - o, ok2);  // "Random direction can't be normalized!"
            ok = ok && ok2;
            return res;
        }
    }
    if (kind == K_MSPHERE) {  // sphere.rs:134-144 with center.at(0)
        const double4 s = S.msph_center[idx];
        const D3 direction = d3(s.x, s.y, s.z) - o;
        const double distance_squared = len2(direction);
        bool ok1, ok2, ok3;
        const D3 nd = unit(direction, ok1);
        const double r1 = rng.next(ovf), r2 = rng.next(ovf);
        const double y = 1.0 + r2 * (k_sqrt(1.0 - s.w * s.w / distance_squared) - 1.0);
        double sphi, cphi;
        k_sincos_2pi(r1, &sphi, &cphi);  // phi = 2.0 * PI * r1
        const double x = cphi * k_sqrt(1.0 - y * y), z = sphi * k_sqrt(1.0 - y * y);
        const D3 res = unit(onb_world(nd, d3(x, y, z), ok2), ok3);
        ok = ok1 && ok2 && ok3;
        return res;
    }
    return light_random_one(S, ref, o, rng, ovf, ok);
}

}  // namespace rtk
