// rt_record.h -- the HitRecord of a walk's closest hit.
#pragma once
#include "rt_builds.h"
#include "rt_geom.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_texture.h"

namespace rtk {

// ------------------------------------------------------------------ hit record
struct Rec {
    D3 p, n;
    double u, v;
    int mat;
    bool front;
};

// HitRecord::new (hit.rs:24-43) of the recorded closest hit, in the frame of
// its innermost Transform, then carried out through the chain (shapes.rs:104-108).
// QUERY (rt_hit_kernel): the record as Hittable::hit returns it -- the
// primitive's own (u, v) always, whether or not a texture reads them, and an
// OBJ triangle's record before RemappedMaterial::remap_record, which is the
// material's work (obj.rs:32-62), not hit's.
template <int TIER, bool QUERY = false>
__device__ Rec make_record(const SceneView& S, const Ray& wr, const HitInfo& h, bool& panic) {
    constexpr bool FULL = tier_full(TIER), PLANAR = TIER >= TIER_MESH;
    Ray r = wr;
    if constexpr (FULL)
        for (uint32_t k = 0; k < h.nxf; ++k) r = xf_ray(S.xforms[h.xf.get(k)], r);
    const uint32_t kind = ref_kind(h.ref), idx = ref_idx(S, h.ref);
    Rec rec;
    rec.u = 0.0;
    rec.v = 0.0;
    const D3 p = r.o + h.t * r.d;
    D3 outward;
    if (!PLANAR || kind == K_SPHERE || kind == K_MSPHERE) {
        D3 c;
        double rinv;  // sphere.rs:99: (p - c) / radius = (1.0 / radius) * (p - c) (vec3.rs:225-227)
        if (!FULL || kind == K_SPHERE) {
            const double4 s = S.spheres[idx];
            c = d3(s.x, s.y, s.z);
            // basic / mesh tiers: the host's 1.0 / r, the same double (C2 -0.5 %);
            // the full tiers divide (C5 +1.0 % with the load: A/B, RMSE 0)
            rinv = !FULL ? S.sphere_rinv[idx] : 1.0 / s.w;
            rec.mat = S.sphere_mat[idx];
        } else {
            const double4 s = S.msph_center[idx], m = S.msph_dir[idx];
            c = d3(s.x, s.y, s.z) + r.time * d3(m.x, m.y, m.z);
            rinv = 1.0 / s.w;
            rec.mat = S.msph_mat[idx];
        }
        outward = rinv * (p - c);
        if (QUERY || (S.materials[rec.mat].flags & MF_NEEDS_UV)) {
            // sphere.rs:53-61
            const double theta = k_acos(-outward.y);
            const double phi = k_atan2(-outward.z, outward.x) + PI;
            rec.u = phi / (2.0 * PI);
            rec.v = theta / PI;
        }
    } else if (kind == K_QUAD || kind == K_TRI) {
        const DPlanar& P = S.planars[idx];
        outward = d3(P.f[0], P.f[1], P.f[2]);
        rec.mat = S.planar_mat[idx];
        // (u, v) = (alpha, beta) of quad.rs:93-99, for a texture that reads
        // them or an OBJ triangle's RemappedMaterial (obj.rs:32-62); nothing
        // else looks at them (full tiers: C3 -1.3 %, C5 -2 %; the mesh tier's
        // OBJ triangles always need them)
        if (QUERY || !FULL || (S.materials[rec.mat].flags & MF_NEEDS_UV) ||
            (PLANAR && kind == K_TRI && S.planar_remap[idx] >= 0)) {
            const D3 hv = p - d3(P.f[4], P.f[5], P.f[6]);
            const D3 u = d3(P.f[7], P.f[8], P.f[9]), v = d3(P.f[10], P.f[11], P.f[12]), w = d3(P.f[13], P.f[14], P.f[15]);
            rec.u = dot(w, cross(hv, v));
            rec.v = dot(w, cross(u, hv));
        }
    } else {  // K_MEDIUM (volume.rs:67-72)
        outward = d3(1.0, 0.0, 0.0);
        rec.mat = S.media[idx].phase_mat;
    }
    rec.front = dot(r.d, outward) < 0.0;
    rec.n = rec.front ? outward : -outward;
    rec.p = p;
    if constexpr (FULL) {
        for (int k = (int)h.nxf - 1; k >= 0; --k) {
            const DXform& X = S.xforms[h.xf.get(k)];
            rec.p = xf_out(X, rec.p);
            bool ok;
            rec.n = unit(quat_rotate(X.q[0], X.q[1], X.q[2], X.q[3], rec.n / d3(X.scale[0], X.scale[1], X.scale[2])), ok);
        }
    }
    if constexpr (PLANAR && !QUERY) {
        // RemappedMaterial::remap_record (obj.rs:32-62), no normal map: applied to
        // the record every material of an OBJ triangle sees (scatter and emitted)
        if (kind == K_TRI) {
            const int32_t ri = S.planar_remap[idx];
            if (ri >= 0) {
                const DRemap& R = S.remaps[ri];
                const double u = rec.u, v = rec.v;
                const double tu = (R.tex_ori[0] + u * R.tex_u[0]) + v * R.tex_v[0];
                const double tv = (R.tex_ori[1] + u * R.tex_u[1]) + v * R.tex_v[1];
                const double w0 = (1.0 - u) - v;
                const D3 nm = ((w0 * d3(R.n[0], R.n[1], R.n[2])) + (u * d3(R.n[3], R.n[4], R.n[5]))) +
                              (v * d3(R.n[6], R.n[7], R.n[8]));
                bool ok;
                rec.n = unit(nm, ok);
                if (!ok) panic = true;  // .unwrap() (obj.rs:40)
                if constexpr (FULL) {
                    if (R.normal_tex >= 0) {  // obj.rs:42-51
                        if (!R.uv_ok) panic = true;  // u_vec.unwrap()
                        const DRemapNM& F = S.remap_nm[ri];
                        const D3 c = tex_value<FULL>(S, R.normal_tex, tu, tv, rec.p);
                        const D3 nc = 2.0 * c - d3(1.0, 1.0, 1.0);
                        const D3 raw = ((nc.x * d3(F.u_vec[0], F.u_vec[1], F.u_vec[2])) +
                                        (nc.y * d3(F.v_vec[0], F.v_vec[1], F.v_vec[2]))) + (nc.z * rec.n);
                        bool ok2;
                        rec.n = unit(raw, ok2);
                        if (!ok2) panic = true;  // "The mapped normal can't normalized!"
                    }
                }
                rec.u = tu;
                rec.v = tv;
            }
        }
    }
    return rec;
}

}  // namespace rtk
