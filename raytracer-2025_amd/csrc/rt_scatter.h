// rt_scatter.h -- one ray_color level opened up for rt_world_scatter: the miss,
// Material::emitted, Material::scatter and the PDF's generate / value, each
// handed back instead of folded into (beta, L).
//
// The material code is shade()'s (rt_shade.h), built from the same leaf device
// functions in the same order, with three differences: the draws are made
// where the reference makes them (rng.next per draw, no Draws hoist: the same
// doubles, and rng.slot is then the count of slots the level consumed); there
// is no lights mix (no MixturePDF, no mixture draw); and a zero pdf is
// returned, not a panic (camera.rs:309 is the caller's assert).  shade() and
// shade_hit_basic() stay as they are: the switch is duplicated here so that no
// path-kernel object changes.
#pragma once
#include "rt_disney.h"
#include "rt_geom.h"
#include "rt_kernel.h"
#include "rt_lights.h"
#include "rt_math.h"
#include "rt_record.h"
#include "rt_shade.h"
#include "rt_texture.h"

namespace rtk {

// What a level returns beside the hit record; `flags` are rt_scatter's
// (RT_SCATTER_*), spelled out here so that the header needs no C ABI.
struct ScatterOut {
    D3 emitted, f, origin, dir, eval_f;
    double pdf, eval_pdf;
    uint32_t flags;
};
constexpr uint32_t SC_RAY = 1u, SC_PDF = 2u, SC_NO_SAMPLE = 4u, SC_EVAL = 8u, SC_PANIC = 16u;

// The PDF object a material's scatter returned: CosinePDF, SpherePDF or DisneyPDF
struct ScatterPdf {
    int kind;  // 0 cosine, 1 sphere, 2 Disney (TIER_FULL_DS)
    D3 albedo, n;
    disney::Params dsp;
    disney::Pdf dsq;
};

// PDF::value(direction) (pdf.rs:22-28, 50-57; disney.rs:662-670), as shade() evaluates it
template <int TIER>
__device__ __forceinline__ void scatter_pdf_value(const ScatterPdf& q, D3 dir, D3& f, double& pdf, bool& panic) {
    constexpr bool FULL = tier_full(TIER);
    if (TIER == TIER_FULL_DS && q.kind == 2) {
        if constexpr (TIER == TIER_FULL_DS) disney::pdf_value(q.dsp, q.dsq, dir, f, pdf, panic);
    } else if (!FULL || q.kind == 0) {
        bool okd;
        const D3 ud = unit(dir, okd);
        if (!okd) panic = true;
        const double ct = dot(ud, q.n);
        pdf = fmax(0.0, ct / PI);
        const double cp = fmax(ct, 0.0);
        f = divs(q.albedo * d3(cp, cp, cp), PI);
    } else {
        pdf = 1.0 / (4.0 * PI);
        f = divs(q.albedo, 4.0 * PI);
    }
}

// camera.rs:286-316 for one ray without the recursion: fills `o` (zeroed by the
// caller).  A reference panic of the level leaves o.flags == SC_PANIC; the
// caller then writes zeros for every other field.
template <int TIER>
__device__ __forceinline__ void scatter_level(const SceneView& S, const Ray& ray, bool hit_any, const HitInfo& h, Rng& rng,
                                              bool has_eval, D3 eval_dir, ScatterOut& o) {
    constexpr bool FULL = tier_full(TIER);
    constexpr bool PL = tier_full_bvh(TIER);  // the block holds the LDS copy of the first Perlin table
    uint32_t ovf = 0;
    bool panic = false;
    if (!hit_any) {
        // miss: Environment::value (environment.rs:14-24), as shade() has it
        // (the basic tier takes the mesh tier's form: unit() gives the same y)
        if (!FULL && S.bg_kind == BG_SKY) {
            bool ok;
            const D3 p = unit(ray.d, ok);
            if (!ok) panic = true;
            o.emitted = sky_value(S.bg_c0, S.bg_c1, p.y);
        } else if (S.background_tex >= 0) {
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
            o.emitted = tex_value<FULL, PL>(S, S.background_tex, u, v, p);
        }
        if (panic) o.flags = SC_PANIC;
        return;
    }
    const Rec rec = make_record<TIER>(S, ray, h, panic);
    if (panic) {
        o.flags = SC_PANIC;
        return;
    }
    DMaterial M = S.materials[rec.mat];
    bool none = false;  // scatter returned None
    if constexpr (tier_general(TIER)) {
        if (M.flags & MF_EMISSIVE) o.emitted = emitted_tree<RT_MAT_DEPTH>(S, rec.mat, rec.u, rec.v, rec.p);
        // the wrappers' scatter: DiffuseLight -> its material or None, Mix -> one draw (material.rs:180-185, 254-260)
        for (int k = 0; k < RT_MAT_DEPTH && !none && (M.type == M_DIFFUSE_LIGHT || M.type == M_MIX); ++k) {
            if (M.type == M_DIFFUSE_LIGHT) {
                if (M.inner < 0)
                    none = true;
                else
                    M = S.materials[M.inner];
            } else {
                M = S.materials[rng.next(ovf) > mix_ratio(S, M, rec.u, rec.v) ? M.inner : M.inner2];
            }
        }
        if (M.type == M_DIFFUSE_LIGHT) none = true;  // a plain light at the last level
    } else if constexpr (FULL) {
        // emitted (material.rs:30-33, 171-178, 262-266)
        if (M.flags & MF_EMISSIVE) {
            if (M.type == M_DIFFUSE_LIGHT) {
                o.emitted = mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
            } else {  // Mix of non-wrapping materials (flatten checks)
                const DMaterial& A = S.materials[M.inner];
                const DMaterial& B = S.materials[M.inner2];
                const D3 ea = A.type == M_DIFFUSE_LIGHT ? mat_tex<FULL, PL>(S, A, rec.u, rec.v, rec.p) : d3(0, 0, 0);
                const D3 eb = B.type == M_DIFFUSE_LIGHT ? mat_tex<FULL, PL>(S, B, rec.u, rec.v, rec.p) : d3(0, 0, 0);
                o.emitted = ((1.0 - M.fuzz) * ea) + (M.fuzz * eb);
            }
        }
        // wrappers: DiffuseLight(inner) scatters as inner (material.rs:180-185); Mix draws (254-260)
        if (M.type == M_DIFFUSE_LIGHT) {
            if (M.inner < 0)
                none = true;
            else
                M = S.materials[M.inner];
        }
        if (!none && M.type == M_MIX) {
            M = S.materials[rng.next(ovf) > M.fuzz ? M.inner : M.inner2];
            if (M.type == M_DIFFUSE_LIGHT) none = true;
        }
    }
    const D3 n = rec.n;
    ScatterPdf q{};
    q.kind = -1;
    q.n = n;
    bool is_ray = false;
    if (!none) {
        switch (M.type) {
            case M_LAMBERTIAN:  // material.rs:60-65
                q.albedo = mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
                q.kind = 0;
                break;
            case M_EMPTY:  // material.rs:41-46
                q.albedo = d3(0.75, 0.75, 0.75);
                q.kind = 0;
                break;
            case M_METAL: {  // material.rs:82-95
                bool ok1, ok2;
                const D3 ud = unit(ray.d, ok1);
                if (!ok1) break;  // `?`: None
                const D3 rr = unit(reflect(ud, n), ok2);
                if (!ok2) break;
                const D3 ruv = random_unit_vector(rng, ovf);
                o.f = d3(M.albedo[0], M.albedo[1], M.albedo[2]);
                o.origin = rec.p;
                o.dir = rr + (M.fuzz * ruv);
                is_ray = true;
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
                    do_reflect = r0sq + (1.0 - r0sq) * (x * (x2 * x2)) > rng.next(ovf);
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
                o.f = mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
                o.origin = rec.p;
                o.dir = dir;
                is_ray = true;
                break;
            }
            default:
                if constexpr (TIER == TIER_FULL_DS) {
                    if (M.type == M_DISNEY) {  // Disney::scatter (disney.rs:71-89): param_fn at the hit, DisneyPDF::new
                        q.dsp = disney::make_params(S.disney[M.inner], mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p));
                        q.dsq = disney::pdf_new(n, -ray.d, rec.front, panic);
                        q.kind = 2;
                        break;
                    }
                }
                if constexpr (FULL) {
                    if (M.type == M_ISOTROPIC) {  // material.rs:199-206
                        q.albedo = mat_tex<FULL, PL>(S, M, rec.u, rec.v, rec.p);
                        q.kind = 1;
                        break;
                    }
                    if (M.type == M_TRANSPARENT) {  // material.rs:211-217
                        o.f = d3(1.0, 1.0, 1.0);
                        o.origin = rec.p;
                        o.dir = ray.d;
                        is_ray = true;
                        break;
                    }
                }
                if constexpr (tier_general(TIER)) {
                    if (M.type == M_PORTAL) {  // Portal::scatter (portal.rs:15-30)
                        const DPortal P = S.portals[M.inner];
                        o.f = d3(P.attenuation[0], P.attenuation[1], P.attenuation[2]);
                        o.origin = rec.p + d3(P.offset[0], P.offset[1], P.offset[2]);
                        o.dir = quat_rotate(P.q[0], P.q[1], P.q[2], P.q[3], ray.d);
                        is_ray = true;
                        break;
                    }
                }
                break;  // None
        }
    }
    if (is_ray) o.flags = SC_RAY;
    if (q.kind >= 0 && !panic) {
        // ScatterRecord::PDF: generate (camera.rs:306, no MixturePDF), then value of the direction made
        o.flags = SC_PDF;
        D3 dir = d3(0, 0, 0);
        bool ok = true, made = true;
        if (TIER == TIER_FULL_DS && q.kind == 2) {
            // DisneyPDF::generate; None leaves the emission only (camera.rs:313-315)
            if constexpr (TIER == TIER_FULL_DS) made = disney::generate(q.dsp, q.dsq, rng, ovf, dir, panic);
        } else if (!FULL || q.kind == 0) {  // CosinePDF::generate (pdf.rs:59-63), vec3.rs:333-343
            const double r1 = rng.next(ovf);
            const double r2 = rng.next(ovf);
            double sn, cs;
            k_sincos_2pi(r1, &sn, &cs);
            const double sr2 = k_sqrt(r2);
            dir = onb_world(n, d3(sn * sr2, k_sqrt(1.0 - r2), cs * sr2), ok);
        } else {
            dir = random_unit_vector(rng, ovf);
        }
        if (!ok) panic = true;
        if (made && !panic) {
            o.origin = rec.p;
            o.dir = dir;
            scatter_pdf_value<TIER>(q, dir, o.f, o.pdf, panic);
        } else {
            o.flags |= SC_NO_SAMPLE;
        }
        if (has_eval) {
            o.flags |= SC_EVAL;
            scatter_pdf_value<TIER>(q, eval_dir, o.eval_f, o.eval_pdf, panic);
        }
    }
    if (ovf) panic = true;
    if (panic) o.flags = SC_PANIC;
}

}  // namespace rtk
