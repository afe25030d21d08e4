// rt_shade.h -- one level of ray_color: the miss, the materials' emitted and
// scatter, the PDF mix (shade), and the basic tier's merged form of a hit
// (shade_hit_basic).
#pragma once
#include "rt_disney.h"
#include "rt_geom.h"
#include "rt_kernel.h"
#include "rt_lights.h"
#include "rt_math.h"
#include "rt_record.h"
#include "rt_texture.h"

namespace rtk {

// A material's texture value; a SolidColor's colour comes with the material
// record (MF_SOLID, set by the flatten), one dependent load fewer.
template <bool FULL, bool PL = false>
__device__ __forceinline__ D3 mat_tex(const SceneView& S, const DMaterial& M, double u, double v, D3 p) {
    if (M.flags & MF_SOLID) return d3(M.albedo[0], M.albedo[1], M.albedo[2]);
    return tex_value<FULL, PL>(S, M.tex, u, v, p);
}

// vec3.rs:313-322
__device__ __forceinline__ D3 random_unit_vector(Rng& rng, uint32_t& ovf) {
    const double r1 = rng.next(ovf), r2 = rng.next(ovf);
    double sn, cs;
    k_sincos_2pi(r1, &sn, &cs);
    const double s = k_sqrt(r2 * (1.0 - r2));
    return d3(cs * 2.0 * s, sn * 2.0 * s, 1.0 - 2.0 * r2);
}

// Basic / mesh tiers: the draws of one path vertex that every scattering
// material there takes -- slots 0 and 1 of the vertex (one Philox block) and
// cos / sin(2 pi xi0) (Lambertian's cosine direction and Metal's
// random_unit_vector, vec3.rs:313-343; Dielectric's Schlick draw is xi0) --
// made once per wave iteration by the main loop, shared with the camera rays
// of the lanes that start a sample there (random_in_unit_disk's theta is
// 2 pi xi too, vec3.rs:63-69): one Philox block and one sincos per lane and
// iteration instead of a shading set and a camera set.
struct Draws {
    double xi0, xi1, sn, cs;
};
// The basic tier's main loop shares the draws.  A/B (RMSE 0): C2 -1.3 % (64
// spp) / -1.8 % (128 spp) kernel time; the mesh tier +3.3 % on C4 (64 spp,
// round 4: the loop's extra live state spills 44 B/lane) and +1.0 % in round
// 5 (28 B/lane), so it keeps the loop of the full tiers.

// ---- general materials (tier FULL_GL): DiffuseLight / Mix wrappers nested
// up to RT_MAT_DEPTH levels (rt_scene.cpp checks), Mix::from_image ratios.
constexpr int RT_MAT_DEPTH = 4;
// Mix::get_ratio (material.rs:249-251): the constant, or the image's alpha
__device__ __forceinline__ double mix_ratio(const SceneView& S, const DMaterial& M, double u, double v) {
    return M.tex >= 0 ? tex_alpha(S, M.tex, u, v) : M.fuzz;
}
// Material::emitted of a wrapper tree: DiffuseLight = its texture + the
// wrapped material's emission (material.rs:171-178), Mix = mat1 * (1 - r) +
// mat2 * r (material.rs:262-266), anything else BLACK
template <int D>
__device__ D3 emitted_tree(const SceneView& S, int mid, double u, double v, D3 p) {
    const DMaterial& M = S.materials[mid];
    if (M.type == M_DIFFUSE_LIGHT) {
        const D3 self = mat_tex<true, true>(S, M, u, v, p);
        D3 inner = d3(0.0, 0.0, 0.0);
        if constexpr (D > 0)
            if (M.inner >= 0) inner = emitted_tree<D - 1>(S, M.inner, u, v, p);
        return self + inner;
    }
    if constexpr (D > 0) {
        if (M.type == M_MIX) {
            const double r = mix_ratio(S, M, u, v);
            return ((1.0 - r) * emitted_tree<D - 1>(S, M.inner, u, v, p)) + (r * emitted_tree<D - 1>(S, M.inner2, u, v, p));
        }
    }
    return d3(0.0, 0.0, 0.0);
}

// ------------------------------------------------------------------ one ray_color level
// camera.rs:275-325 at path vertex `vertex`; updates (ray, beta, L).  Returns
// true when the path ends here (miss, no scatter, panic).
template <int TIER>
__device__ __forceinline__ bool shade(const SceneView& S, Ray& ray, D3& beta, D3& L, Rng& rng, bool hit_any,
                                      const HitInfo& h, bool& panic, const Draws& Dr = Draws{}) {
    constexpr bool FULL = tier_full(TIER);
    constexpr bool PL = tier_full_bvh(TIER);  // the block holds the LDS copy of the first Perlin table (the flat tier's LDS is full)
    uint32_t ovf = 0;
    if (!hit_any) {
        // miss: Environment::value (environment.rs:14-24)
        if constexpr (TIER == TIER_BASIC) {
            // (C2 -1.4 %, profiles/r05/ab_sky_y_c2_128spp.json; the mesh tier
            // measured +0.4 % on C4 with it and keeps unit())
            // Basic tier under a sky gradient (the world's background
            // is wave-uniform: a scalar branch): the gradient reads the unit
            // direction's y only, so only that component is made, as unit()
            // makes it: (1 / l) * d.y (vec3.rs:225-232, rt_math.h divs).
            // `ok` is the same as unit()'s finite3 of the three products:
            // with l = |d| not NaN and not 0 and every component finite,
            // 1 / l is finite (a nonzero l is >= sqrt(5e-324) ~ 2e-162) and
            // each (1 / l) * d_i is finite (|d_i| <= l, or l = inf over
            // finite components: 0); l = 0 or NaN, or an infinite component
            // (0 * inf), gives a NaN (tests/test_miss_unit_cpu.py)
            // The gradient's colours come with the launch parameters
            // (SceneView::bg_c0 / bg_c1), not from the texture table.
            if (S.bg_kind == BG_SKY) {
                const double l = len(ray.d);
                if (isnan(l) || l == 0.0 || !finite3(ray.d)) panic = true;
                L = L + beta * sky_value(S.bg_c0, S.bg_c1, (1.0 / l) * ray.d.y);
                return true;
            }
        }
        if (!FULL && S.bg_kind == BG_SKY) {  // the mesh tier: unit(), the gradient from the launch parameters
            bool ok;
            const D3 p = unit(ray.d, ok);
            if (!ok) panic = true;
            L = L + beta * sky_value(S.bg_c0, S.bg_c1, p.y);
            return true;
        }
        if (S.background_tex >= 0) {
            bool ok;
            const D3 p = unit(ray.d, ok);
            if (!ok) panic = true;
            double u = 0.0, v = 0.0;
            if (FULL && S.textures[S.background_tex].needs_uv) {
                const double theta = k_acos(-p.y);
                const double phi = PI - k_atan2(-p.z, p.x);
                u = phi / (2.0 * PI);
                v = theta / PI;
            }
            L = L + beta * tex_value<FULL, PL>(S, S.background_tex, u, v, p);
        }
        return true;
    }
    const Rec rec = make_record<TIER>(S, ray, h, panic);
    if (panic) return true;
    DMaterial M = S.materials[rec.mat];
    // Basic / mesh tiers: every scattering material draws slot 0 (and 1) of
    // this vertex first, and Lambertian and Metal both turn the first draw
    // into cos/sin(2 pi r1) (vec3.rs:313-322, 333-343): the main loop's Draws.
    constexpr bool HOIST = !FULL;
    const double xi0 = Dr.xi0, xi1 = Dr.xi1, sn0 = Dr.sn, cs0 = Dr.cs;
    if constexpr (tier_general(TIER)) {
        if (M.flags & MF_EMISSIVE) L = L + beta * emitted_tree<RT_MAT_DEPTH>(S, rec.mat, rec.u, rec.v, rec.p);
        // the wrappers' scatter: DiffuseLight -> its material or None, Mix -> one draw (material.rs:180-185, 254-260)
        for (int k = 0; k < RT_MAT_DEPTH && (M.type == M_DIFFUSE_LIGHT || M.type == M_MIX); ++k) {
            if (M.type == M_DIFFUSE_LIGHT) {
                if (M.inner < 0) return true;
                M = S.materials[M.inner];
            } else {
                M = S.materials[rng.next(ovf) > mix_ratio(S, M, rec.u, rec.v) ? M.inner : M.inner2];
            }
        }
        if (M.type == M_DIFFUSE_LIGHT) return true;  // a plain light at the last level
    } else if constexpr (FULL) {
        // emitted (material.rs:30-33, 171-178, 262-266)
        if (M.flags & MF_EMISSIVE) {
            D3 em;
            if (M.type == M_DIFFUSE_LIGHT) {
                em = mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
            } else {  // Mix of non-wrapping materials (flatten checks)
                const DMaterial& A = S.materials[M.inner];
                const DMaterial& B = S.materials[M.inner2];
                const D3 ea = A.type == M_DIFFUSE_LIGHT ? mat_tex<FULL, PL>(S, A, rec.u, rec.v, rec.p) : d3(0, 0, 0);
                const D3 eb = B.type == M_DIFFUSE_LIGHT ? mat_tex<FULL, PL>(S, B, rec.u, rec.v, rec.p) : d3(0, 0, 0);
                em = ((1.0 - M.fuzz) * ea) + (M.fuzz * eb);
            }
            L = L + beta * em;
        }
        // wrappers: DiffuseLight(inner) scatters as inner (material.rs:180-185); Mix draws (254-260)
        if (M.type == M_DIFFUSE_LIGHT) {
            if (M.inner < 0) return true;
            M = S.materials[M.inner];
        }
        if (M.type == M_MIX) {
            M = S.materials[rng.next(ovf) > M.fuzz ? M.inner : M.inner2];
            if (M.type == M_DIFFUSE_LIGHT) return true;
        }
    }
    const D3 n = rec.n;
    int pdf_kind = -1;  // 0 cosine, 1 sphere, 2 Disney (TIER_FULL_DS)
    D3 albedo = d3(0, 0, 0);
    disney::Params dsp{};  // (TIER_FULL_DS only: unused, so absent, elsewhere)
    disney::Pdf dsq{};
    switch (M.type) {
        case M_LAMBERTIAN:  // material.rs:60-65
            albedo = mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
            pdf_kind = 0;
            break;
        case M_EMPTY:  // material.rs:41-46
            albedo = d3(0.75, 0.75, 0.75);
            pdf_kind = 0;
            break;
        case M_METAL: {  // material.rs:82-95
            bool ok1, ok2;
            const D3 ud = unit(ray.d, ok1);
            if (!ok1) return true;
            const D3 rr = unit(reflect(ud, n), ok2);
            if (!ok2) return true;
            D3 ruv;
            if constexpr (!HOIST) {
                ruv = random_unit_vector(rng, ovf);
            } else {
                const double s = k_sqrt(xi1 * (1.0 - xi1));
                ruv = d3(cs0 * 2.0 * s, sn0 * 2.0 * s, 1.0 - 2.0 * xi1);
            }
            beta = beta * d3(M.albedo[0], M.albedo[1], M.albedo[2]);
            ray = Ray{rec.p, rr + (M.fuzz * ruv), ray.time};
            break;
        }
        case M_DIELECTRIC: {  // material.rs:117-143
            const double ri = rec.front ? 1.0 / M.fuzz : M.fuzz;
            bool ok;
            const D3 ud = unit(ray.d, ok);
            if (!ok) panic = true;
            const double cos_theta = fmin(dot(-ud, n), 1.0);
            const double sin_theta = k_sqrt(1.0 - cos_theta * cos_theta);
            bool do_reflect = ri * sin_theta > 1.0;
            if (!do_reflect) {  // Schlick (material.rs:110-114); the draw only when refraction is possible
                const double r0 = (1.0 - ri) / (1.0 + ri);
                const double r0sq = r0 * r0;
                const double x = 1.0 - cos_theta;
                const double x2 = x * x;
                do_reflect = r0sq + (1.0 - r0sq) * (x * (x2 * x2)) > (HOIST ? xi0 : rng.next(ovf));
            }
            D3 dir;
            if (do_reflect) {
                dir = reflect(ud, n);
            } else {  // vec3.rs:345-354
                const D3 perp = ri * (ud + cos_theta * n);
                const double pl = k_sqrt(1.0 - len2(perp));
                if (isnan(pl)) panic = true;
                dir = perp + (-pl * n);
            }
            beta = beta * mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
            ray = Ray{rec.p, dir, ray.time};
            break;
        }
        default:
            if constexpr (TIER == TIER_FULL_DS) {
                if (M.type == M_DISNEY) {  // Disney::scatter (disney.rs:71-89): param_fn at the hit, DisneyPDF::new
                    dsp = disney::make_params(S.disney[M.inner], mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p));
                    dsq = disney::pdf_new(n, -ray.d, rec.front, panic);
                    if (panic) return true;
                    pdf_kind = 2;
                    break;
                }
            }
            if constexpr (FULL) {
                if (M.type == M_ISOTROPIC) {  // material.rs:199-206
                    albedo = mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
                    pdf_kind = 1;
                    break;
                }
                if (M.type == M_TRANSPARENT) {  // material.rs:211-217
                    ray = Ray{rec.p, ray.d, ray.time};
                    break;
                }
            }
            if constexpr (tier_general(TIER)) {
                // Portal::scatter (portal.rs:15-30): ScatterRecord::Ray, so no draw and no
                // PDF (camera.rs:317-319); the quaternion and the rotated direction are
                // used as they come.  The record is read here only
                if (M.type == M_PORTAL) {
                    const DPortal P = S.portals[M.inner];
                    beta = beta * d3(P.attenuation[0], P.attenuation[1], P.attenuation[2]);
                    ray = Ray{rec.p + d3(P.offset[0], P.offset[1], P.offset[2]),
                              quat_rotate(P.q[0], P.q[1], P.q[2], P.q[3], ray.d), ray.time};
                    break;
                }
            }
            return true;
    }
    if (pdf_kind >= 0) {
        // PDF branch (camera.rs:297-316)
        const bool use_lights = FULL && S.lights_root != REF_NONE;
        bool from_material = true;
        if (use_lights) from_material = rng.next(ovf) < 0.5;  // MixturePDF::generate (pdf.rs:113-119)
        D3 dir;
        bool ok = true;
        if (from_material) {
            if (TIER == TIER_FULL_DS && pdf_kind == 2) {
                // DisneyPDF::generate; None ends the path with the emission only (camera.rs:313-315)
                if constexpr (TIER == TIER_FULL_DS) {
                    if (!disney::generate(dsp, dsq, rng, ovf, dir, panic)) {
                        if (ovf) panic = true;
                        return true;
                    }
                }
            } else if (!FULL || pdf_kind == 0) {  // CosinePDF::generate (pdf.rs:59-63), vec3.rs:333-343
                double r2 = xi1, sn = sn0, cs = cs0;
                if constexpr (!HOIST) {
                    const double r1 = rng.next(ovf);
                    r2 = rng.next(ovf);
                    k_sincos_2pi(r1, &sn, &cs);
                }
                const double sr2 = k_sqrt(r2);
                dir = onb_world(n, d3(sn * sr2, k_sqrt(1.0 - r2), cs * sr2), ok);
            } else {
                dir = random_unit_vector(rng, ovf);
            }
        } else {
            if constexpr (tier_general(TIER))
                dir = light_random_tree<RT_LIGHT_DEPTH>(S, S.lights_root, rec.p, rng, ovf, ok);
            else
                dir = light_random(S, rec.p, rng, ovf, ok);
        }
        if (!ok) panic = true;
        // value (pdf.rs:22-28, 50-57, 101-111)
        D3 f;
        double pdf;
        if (TIER == TIER_FULL_DS && pdf_kind == 2) {  // DisneyPDF::value (disney.rs:662-670)
            if constexpr (TIER == TIER_FULL_DS) disney::pdf_value(dsp, dsq, dir, f, pdf, panic);
        } else if (!FULL || pdf_kind == 0) {
            bool okd;
            const D3 ud = unit(dir, okd);
            if (!okd) panic = true;
            const double ct = dot(ud, n);
            pdf = fmax(0.0, ct / PI);
            const double cp = fmax(ct, 0.0);
            f = divs(albedo * d3(cp, cp, cp), PI);
        } else {
            pdf = 1.0 / (4.0 * PI);
            f = divs(albedo, 4.0 * PI);
        }
        if (use_lights) {
            double pdf1;
            if constexpr (tier_general(TIER))
                pdf1 = light_pdf_tree<RT_LIGHT_DEPTH>(S, S.lights_root, rec.p, dir, panic);
            else
                pdf1 = light_pdf(S, rec.p, dir);
            if (isnan(pdf1)) panic = true;
            if (pdf == 0.0 && pdf1 == 0.0) panic = true;
            pdf = pdf * 0.5 + pdf1 * 0.5;
        }
        if (pdf == 0.0) panic = true;  // camera.rs:309
        beta = beta * divs(f, pdf);
        ray = Ray{rec.p, dir, ray.time};
    }
    if (ovf) panic = true;
    return panic;
}

// ------------------------------------------------------------------ basic tier: one hit, merged
// shade() for a hit in the basic tier (camera.rs:286-316; Lambertian /
// EmptyMaterial, Metal, Dielectric: material.rs:41-143, onb.rs:8-38,
// pdf.rs:50-63), with the three scatter codes' square roots and divisions
// merged.  As one switch, a wave whose shading batch holds all three
// classes ran every class's unit vectors, square roots and divisions one
// after the other (10 square roots and 9 divisions); here each stage is one
// square root or division that every lane runs on its own class's operand:
//   A  unit(cross(n, a)) (Lambertian's ONB)  |  unit(r_in.direction) (Metal, Dielectric)
//   B1 sqrt(r2)  |  sqrt(r2 (1 - r2)) (random_unit_vector)  |  sin_theta
//   B2 sqrt(1 - r2) (Lambertian)
//   C  unit(direction) (Lambertian)  |  unit(reflect) (Metal);  1 / ior (Dielectric, front face)
//   D1 cos_theta / PI (Lambertian pdf)  |  r0 = (1 - ri) / (1 + ri) (Dielectric, Schlick)
//   D2 1 / pdf (Lambertian);  E  the refracted ray's sqrt (Dielectric)
// Every lane computes exactly the operations of its class, in the
// reference's order (the same doubles as shade()); only the instructions
// are shared.  Returns true when the path ends (panic: a reference panic
// condition).
__device__ __forceinline__ bool shade_hit_basic(const SceneView& S, Ray& ray, D3& beta, const HitInfo& h, bool& panic,
                                                const Draws& Dr) {
    const Rec rec = make_record<TIER_BASIC>(S, ray, h, panic);
    if (panic) return true;
    const DMaterial M = S.materials[rec.mat];
    constexpr int LAMB = 0, METAL = 1, DIEL = 2;
    const int cls = (M.type == M_LAMBERTIAN || M.type == M_EMPTY) ? LAMB
                  : M.type == M_METAL ? METAL : M.type == M_DIELECTRIC ? DIEL : 3;
    if (cls == 3) return true;  // (no other material reaches the basic tier)
    const D3 n = rec.n;
    const double xi0 = Dr.xi0, xi1 = Dr.xi1, sn0 = Dr.sn, cs0 = Dr.cs;
    // the albedo (Lambertian, material.rs:60-65) or attenuation (Dielectric, :141)
    D3 tex = d3(0.75, 0.75, 0.75);  // EmptyMaterial (material.rs:41-46)
    if (M.type == M_LAMBERTIAN || cls == DIEL) tex = mat_tex<false, false>(S, M, rec.u, rec.v, rec.p);
    // ---- A
    D3 vA = ray.d;
    if (cls == LAMB) {  // onb.rs:8-21
        const D3 a = fabs(n.x) > 0.9 ? d3(0.0, 1.0, 0.0) : d3(1.0, 0.0, 0.0);
        vA = cross(n, a);
    }
    bool okA;
    const D3 uA = unit(vA, okA);
    if (!okA) {
        if (cls == METAL) return true;  // material.rs:83: r_in.direction not normalizable -> None
        panic = true;                   // onb.rs / material.rs:120: .expect
    }
    // ---- B1, B2
    double cosd = 0.0, xB1 = xi1;  // Lambertian: r2 (vec3.rs:333-343)
    if (cls == METAL) xB1 = xi1 * (1.0 - xi1);  // vec3.rs:313-322
    if (cls == DIEL) {                          // material.rs:121-122
        cosd = fmin(dot(-uA, n), 1.0);
        xB1 = 1.0 - cosd * cosd;
    }
    const double sB1 = k_sqrt(xB1);
    double sB2 = 0.0;
    if (cls == LAMB) sB2 = k_sqrt(1.0 - xi1);
    // ---- C
    D3 vC = ray.d;
    if (cls == LAMB) {  // onb_world: v.x u + v.y n + v.z w (onb.rs:34-38)
        const D3 w = cross(uA, n);
        const D3 v = d3(sn0 * sB1, sB2, cs0 * sB1);
        vC = v.x * uA + v.y * n + v.z * w;
    } else if (cls == METAL) {
        vC = reflect(uA, n);
    }
    const double lC = len(vC);
    const double qC = 1.0 / (cls == DIEL ? M.fuzz : lC);  // unit(): (1 / |v|) v; Dielectric: 1 / ior
    const D3 uC = qC * vC;
    const bool okC = finite3(uC);
    if (cls == METAL) {  // material.rs:82-95
        if (!okC) return true;
        const double s = sB1;
        const D3 ruv = d3(cs0 * 2.0 * s, sn0 * 2.0 * s, 1.0 - 2.0 * xi1);
        beta = beta * d3(M.albedo[0], M.albedo[1], M.albedo[2]);
        ray = Ray{rec.p, uC + (M.fuzz * ruv), ray.time};
        return panic;
    }
    // ---- D1
    double ct = 0.0, ri = 0.0;
    bool refl = false;
    if (cls == LAMB) {
        if (!okC) panic = true;  // pdf.rs:22-28 (the direction's unit)
        ct = dot(uC, n);
    } else {  // Dielectric: ri (material.rs:118), total internal reflection (:123)
        ri = rec.front ? qC : M.fuzz;
        refl = ri * sB1 > 1.0;
    }
    const double qD1 = (cls == LAMB ? ct : 1.0 - ri) / (cls == LAMB ? PI : 1.0 + ri);
    if (cls == LAMB) {  // pdf.rs:50-57, camera.rs:305-316
        const double pdf = fmax(0.0, qD1);
        const double cp = fmax(ct, 0.0);
        const D3 f = divs(tex * d3(cp, cp, cp), PI);
        if (pdf == 0.0) panic = true;  // camera.rs:309
        beta = beta * divs(f, pdf);
        ray = Ray{rec.p, vC, ray.time};
        return panic;
    }
    // Dielectric: Schlick (material.rs:110-114), the draw only when refraction is possible
    if (!refl) {
        const double r0 = qD1;
        const double r0sq = r0 * r0;
        const double x = 1.0 - cosd;
        const double x2 = x * x;
        refl = r0sq + (1.0 - r0sq) * (x * (x2 * x2)) > xi0;
    }
    D3 dir;
    if (refl) {
        dir = reflect(uA, n);
    } else {  // vec3.rs:345-354
        const D3 perp = ri * (uA + cosd * n);
        const double pl = k_sqrt(1.0 - len2(perp));
        if (isnan(pl)) panic = true;
        dir = perp + (-pl * n);
    }
    beta = beta * tex;
    ray = Ray{rec.p, dir, ray.time};
    return panic;
}

}  // namespace rtk
