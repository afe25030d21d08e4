// rt_disney.h -- the Disney BSDF (material/disney.rs) as device functions:
// Disney::evaluate_disney and its lobes (disney.rs:102-423), the helpers
// (425-514), DisneyPDF's four lobe samplers and the VNDF sampler (516-716),
// utils/fresnel.rs, and the UnitVec3 / OrthonormalBasis helpers they use
// (vec3.rs:76-78, 357-426, onb.rs:39-45).  Only the full tier with the Disney
// case (TIER_FULL_DS) and the Disney self-test kernel include it.
//
// The reference is restated as it computes, quirks included:
//  - UnitVec3::cos_theta2 returns y, not y^2 (vec3.rs:380-382): sin_theta2 =
//    clamp(1 - y, 0, 1) and tan_theta = sqrt(that) / y;
//  - cos_phi / sin_phi are 1.0 whenever |sin_theta| < 1e8 (vec3.rs:400-416):
//    the Smith G1's a = sqrt(ax^2 + ay^2);
//  - a zero forward pdf becomes +inf (disney.rs:395-398): the sample then
//    contributes 0, with no panic;
//  - powi multiplies as compiler-rt's __powidf2: x^2 = x x, x^5 = x (x^2)^2;
//  - f64::signum of +-0 is +-1; f64::clamp and Vec3 / f64 (1.0 / s * v) as
//    the reference writes them.
// Every unwrap / expect / assert! of those lines sets `panic`: the path ends
// and is counted (rt_stats.panics).  f64, -ffp-contract=off like the rest of
// the path.
#pragma once
#include "rt_kernel.h"
#include "rt_math.h"

// The evaluator and the generator are inlined into shade(), each at its one
// call site: as calls their Params / Pdf arguments travel through scratch and
// the tier's scratch grows (736 against 608 B/lane in the resource report;
// DESIGN.md "Tier 5").  RT_DISNEY_INLINE=0 compiles them as calls (A/B only).
#ifndef RT_DISNEY_INLINE
#define RT_DISNEY_INLINE 1
#endif
#if RT_DISNEY_INLINE
#define RT_DISNEY_FN __device__ __forceinline__
#else
#define RT_DISNEY_FN __device__ inline __attribute__((noinline))
#endif

namespace rtk {
namespace disney {

// DisneyParameters (disney.rs:17-34) at one hit: param_fn's result
struct Params {
    D3 base_color;
    double roughness, anisotropic, sheen, sheen_tint, clearcoat, clearcoat_gloss, specular_tint, metallic, ior, flatness,
        spec_trans, diff_trans;
    bool thin;
};
__device__ __forceinline__ Params make_params(const RT_GLOBAL DDisney& R, D3 base_color) {
    Params p;
    p.base_color = base_color;
    p.roughness = R.roughness, p.anisotropic = R.anisotropic, p.sheen = R.sheen, p.sheen_tint = R.sheen_tint;
    p.clearcoat = R.clearcoat, p.clearcoat_gloss = R.clearcoat_gloss, p.specular_tint = R.specular_tint;
    p.metallic = R.metallic, p.ior = R.ior, p.flatness = R.flatness, p.spec_trans = R.spec_trans;
    p.diff_trans = R.diff_trans;
    p.thin = R.thin != 0;
    return p;
}

// ---------------------------------------------------------------- scalar helpers
__device__ __forceinline__ double pow2(double x) { return x * x; }  // powi(2)
__device__ __forceinline__ double pow5(double x) {                  // powi(5)
    const double x2 = x * x;
    return x * (x2 * x2);
}
// f64::clamp: NaN passes through
__device__ __forceinline__ double clampd(double x, double lo, double hi) {
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return x;
}
// utils.rs:14-19
__device__ __forceinline__ double lerp(double a, double b, double t) { return a * (1.0 - t) + b * t; }
__device__ __forceinline__ D3 mulr(D3 v, double s) { return d3(v.x * s, v.y * s, v.z * s); }  // Vec3 * f64
__device__ __forceinline__ D3 lerp(D3 a, D3 b, double t) { return mulr(a, 1.0 - t) + mulr(b, t); }
// f64::signum
__device__ __forceinline__ double signum(double x) { return isnan(x) ? x : __builtin_copysign(1.0, x); }

// ---------------------------------------------------------------- UnitVec3 (vec3.rs:357-426)
__device__ __forceinline__ double sin_theta2(D3 w) { return clampd(1.0 - w.y, 0.0, 1.0); }  // cos_theta2() is y
__device__ __forceinline__ double sin_theta(D3 w) { return k_sqrt(sin_theta2(w)); }
__device__ __forceinline__ double tan_theta(D3 w) { return sin_theta(w) / w.y; }
__device__ __forceinline__ double cos_phi2(D3 w) {
    const double st = sin_theta(w);
    const double c = fabs(st) < 1e8 ? 1.0 : w.x / st;
    return c * c;
}
__device__ __forceinline__ double sin_phi2(D3 w) {
    const double st = sin_theta(w);
    const double s = fabs(st) < 1e8 ? 1.0 : w.z / st;
    return s * s;
}
// vec3.rs:76-78: the incoming direction already flipped
__device__ __forceinline__ D3 reflect2(D3 v, D3 n) { return (-v) + (2.0 * dot(v, n)) * n; }
// vec3.rs:357-366
__device__ __forceinline__ bool refract2(D3 v, D3 n, double eta, D3& out) {
    const double cos_theta = fmin(dot(v, n), 1.0);
    const D3 perp = eta * ((-v) + cos_theta * n);
    const double pl = k_sqrt(1.0 - len2(perp));
    if (isnan(pl)) return false;
    out = perp + (-pl) * n;
    return true;
}

// onb.rs:8-45
struct Onb {
    D3 u, v, w;
};
__device__ __forceinline__ Onb onb_new(D3 n, bool& ok) {
    const D3 a = fabs(n.x) > 0.9 ? d3(0.0, 1.0, 0.0) : d3(1.0, 0.0, 0.0);
    Onb b;
    b.u = unit(cross(n, a), ok);
    b.v = n;
    b.w = cross(b.u, n);
    return b;
}
__device__ __forceinline__ D3 onb_to_world(const Onb& b, D3 v) { return (v.x * b.u + v.y * b.v) + v.z * b.w; }
__device__ __forceinline__ D3 world_to_onb(const Onb& b, D3 v) { return d3(dot(v, b.u), dot(v, b.v), dot(v, b.w)); }

// ---------------------------------------------------------------- fresnel.rs
__device__ __forceinline__ double schlick_weight(double u) { return pow5(clampd(1.0 - u, 0.0, 1.0)); }  // :12-15
__device__ __forceinline__ D3 schlick(D3 r0, double radians) {                                           // :3-6
    const double e = pow5(1.0 - radians);
    return r0 + mulr(d3(1.0, 1.0, 1.0) - r0, e);
}
__device__ __forceinline__ double schlick_f64(double r0, double radians) {  // :8-10
    return lerp(1.0, schlick_weight(radians), r0);
}
__device__ __forceinline__ double schlick_r0_from_relative_ior(double eta) {  // :17-19
    return pow2(eta - 1.0) / pow2(eta + 1.0);
}
__device__ __forceinline__ double dielectric(double cos_theta_in, double n_in, double n_out) {  // :21-46
    cos_theta_in = clampd(cos_theta_in, -1.0, 1.0);
    if (cos_theta_in < 0.0) {
        const double t = n_in;
        n_in = n_out;
        n_out = t;
        cos_theta_in = -cos_theta_in;
    }
    const double sin_theta_in = k_sqrt(fmax(1.0 - cos_theta_in * cos_theta_in, 0.0));
    const double sin_theta_out = n_in / n_out * sin_theta_in;
    if (sin_theta_out >= 1.0) return 1.0;
    const double cos_theta_out = k_sqrt(fmax(1.0 - sin_theta_out * sin_theta_out, 0.0));
    const double r_parallel = (n_out * cos_theta_in - n_in * cos_theta_out) / (n_out * cos_theta_in + n_in * cos_theta_out);
    const double r_perp = (n_in * cos_theta_in - n_out * cos_theta_out) / (n_in * cos_theta_in + n_out * cos_theta_out);
    return (r_parallel * r_parallel + r_perp * r_perp) / 2.0;
}

// ---------------------------------------------------------------- helpers (disney.rs:425-514)
__device__ __forceinline__ D3 calculate_tint(D3 base_color) {  // :425-433
    const double luminance = 0.3 * base_color.x + 0.6 * base_color.y + 1.0 * base_color.z;
    if (luminance > 0.0) return mulr(base_color, 1.0 / luminance);
    return d3(1.0, 1.0, 1.0);
}
__device__ __forceinline__ double gtr1(double dot_hl, double a) {  // :435-443
    if (a >= 1.0) return 1.0 / PI;
    const double a2 = a * a;
    return (a2 - 1.0) / (PI * k_log(a2) * (1.0 + (a2 - 1.0) * dot_hl * dot_hl));
}
__device__ __forceinline__ double separable_smith_ggxg1(D3 w, double a) {  // :445-450
    const double a2 = a * a;
    const double dot_nv = w.y;
    return 2.0 / (1.0 + k_sqrt(a2 + (1.0 - a2) * dot_nv * dot_nv));
}
__device__ __forceinline__ double ggx_anisotropic_d(D3 h, double ax, double ay) {  // :452-460
    const double dot_hx2 = pow2(h.x), dot_hy2 = pow2(h.z), cos_theta2 = pow2(h.y);
    const double ax2 = ax * ax, ay2 = ay * ay;
    return 1.0 / (PI * ax * ay * pow2(dot_hx2 / ax2 + dot_hy2 / ay2 + cos_theta2));
}
__device__ __forceinline__ double anisotropic_separable_smith_ggxg1(D3 w, D3 h, double ax, double ay, bool& panic) {  // :462-480
    const double dot_hw = dot(w, h);
    if (dot_hw <= 0.0) return 0.0;
    const double abs_tan_theta = fabs(tan_theta(w));
    if (isnan(abs_tan_theta)) panic = true;  // :469
    if (isinf(abs_tan_theta)) return 0.0;
    const double a = k_sqrt(cos_phi2(w) * ax * ax + sin_phi2(w) * ay * ay);
    const double a2_tan_theta2 = pow2(a * abs_tan_theta);
    const double lambda = 0.5 * (-1.0 + k_sqrt(1.0 + a2_tan_theta2));
    return 1.0 / (1.0 + lambda);
}
__device__ __forceinline__ void calculate_anisotropic_params(double roughness, double anisotropic, double& ax, double& ay) {  // :482-488
    const double aspect = k_sqrt(1.0 - 0.9 * anisotropic);
    const double roughness2 = roughness * roughness;
    ax = fmax(0.001, roughness2 / aspect);
    ay = fmax(0.001, roughness2 * aspect);
}
__device__ __forceinline__ void ggx_vndf_anisotropic_pdf(D3 v_in, D3 h, D3 v_out, double ax, double ay, double& fwd,
                                                         double& rev, bool& panic) {  // :490-510
    const double d = ggx_anisotropic_d(h, ax, ay);
    const double abs_dot_nv = fabs(v_out.y);
    const double abs_dot_hv = fabs(dot(h, v_out));
    const double g1v = anisotropic_separable_smith_ggxg1(v_out, h, ax, ay, panic);
    fwd = g1v * abs_dot_hv * d / abs_dot_nv;
    const double abs_dot_nl = fabs(v_in.y);
    const double abs_dot_hl = fabs(dot(h, v_in));
    const double g1l = anisotropic_separable_smith_ggxg1(v_in, h, ax, ay, panic);
    rev = g1l * abs_dot_hl * d / abs_dot_nl;
}
__device__ __forceinline__ double thin_transmission_roughness(double ior, double roughness) {  // :512-514
    return clampd((0.65 * ior - 0.35) * roughness, 0.0, 1.0);
}

// ---------------------------------------------------------------- the lobes (disney.rs:102-287)
__device__ __forceinline__ D3 disney_fresnel(const Params& P, D3 v_out, D3 h, D3 v_in, double relative_ior) {  // :175-198
    const double dot_hv = dot(h, v_out);
    const D3 tint = calculate_tint(P.base_color);
    D3 r0 = schlick_r0_from_relative_ior(relative_ior) * lerp(d3(1.0, 1.0, 1.0), tint, P.specular_tint);
    r0 = lerp(r0, P.base_color, P.metallic);
    const double dielectric_fresnel = dielectric(dot_hv, 1.0, P.ior);
    const D3 metallic_fresnel = schlick(r0, dot(v_in, h));
    return lerp(d3(dielectric_fresnel, dielectric_fresnel, dielectric_fresnel), metallic_fresnel, P.metallic);
}
__device__ __forceinline__ void evaluate_brdf(const Params& P, D3 v_out, D3 h, D3 v_in, double relative_ior, D3& value,
                                              double& fwd, double& rev, bool& panic) {  // :102-130
    const double dot_nl = v_in.y, dot_nv = v_out.y;
    if (dot_nl <= 0.0 || dot_nv <= 0.0) {
        value = d3(0.0, 0.0, 0.0);
        fwd = rev = 0.0;
        return;
    }
    double ax, ay;
    calculate_anisotropic_params(P.roughness, P.anisotropic, ax, ay);
    const double d = ggx_anisotropic_d(h, ax, ay);
    const double gl = anisotropic_separable_smith_ggxg1(v_in, h, ax, ay, panic);
    const double gv = anisotropic_separable_smith_ggxg1(v_out, h, ax, ay, panic);
    const D3 f = disney_fresnel(P, v_out, h, v_in, relative_ior);
    ggx_vndf_anisotropic_pdf(v_in, h, v_out, ax, ay, fwd, rev, panic);
    fwd = fwd / (4.0 * fabs(dot(v_in, h)));
    rev = rev / (4.0 * fabs(dot(v_out, h)));
    value = divs((d * gl * gv) * f, 4.0 * dot_nl * dot_nv);
}
__device__ __forceinline__ D3 evaluate_sheen(const Params& P, D3 h, D3 v_in) {  // :132-147
    if (P.sheen <= 0.0) return d3(0.0, 0.0, 0.0);
    const double dot_hl = dot(h, v_in);
    const D3 tint = calculate_tint(P.base_color);
    return mulr(P.sheen * lerp(d3(1.0, 1.0, 1.0), tint, P.sheen_tint), schlick_weight(dot_hl));
}
__device__ __forceinline__ void evaluate_clearcoat(const Params& P, D3 v_out, D3 h, D3 v_in, double& value, double& fwd,
                                                   double& rev) {  // :149-173
    if (P.clearcoat <= 0.0) {
        value = fwd = rev = 0.0;
        return;
    }
    const double dot_nh = h.y;
    const double dot_hl = dot(h, v_in);
    const double d = gtr1(dot_nh, lerp(0.1, 0.001, P.clearcoat_gloss));
    const double f = schlick_f64(0.04, dot_hl);
    const double gl = separable_smith_ggxg1(v_in, 0.25);
    const double gv = separable_smith_ggxg1(v_out, 0.25);
    value = 0.25 * P.clearcoat * d * f * gl * gv;
    fwd = d / (4.0 * fabs(dot(v_in, h)));
    rev = d / (4.0 * fabs(dot(v_out, h)));
}
__device__ __forceinline__ D3 evaluate_disney_spec_transmission(const Params& P, D3 v_out, D3 h, D3 v_in, double ax,
                                                                double ay, double relative_ior, bool& panic) {  // :200-233
    const double n2 = relative_ior * relative_ior;
    const double abs_dot_nl = fabs(v_in.y), abs_dot_nv = fabs(v_out.y);
    const double dot_hl = dot(h, v_in), dot_hv = dot(h, v_out);
    const double abs_dot_hl = fabs(dot_hl), abs_dot_hv = fabs(dot_hv);
    const double d = ggx_anisotropic_d(h, ax, ay);
    const double gl = anisotropic_separable_smith_ggxg1(v_in, h, ax, ay, panic);
    const double gv = anisotropic_separable_smith_ggxg1(v_out, h, ax, ay, panic);
    const double f = dielectric(dot_hv, 1.0, 1.0 / relative_ior);
    D3 color = P.base_color;
    if (P.thin) {  // Vec3::sqrt (vec3.rs:127-133): panics on a NaN
        color = d3(k_sqrt(color.x), k_sqrt(color.y), k_sqrt(color.z));
        if (isnan(color.x) || isnan(color.y) || isnan(color.z)) panic = true;
    }
    const double c = (abs_dot_hl * abs_dot_hv) / (abs_dot_nl * abs_dot_nv);
    const double t = n2 / pow2(dot_hl + relative_ior * dot_hv);
    return (c * t * (1.0 - f) * gl * gv * d) * color;
}
__device__ __forceinline__ double evaluate_disney_retro_diffuse(const Params& P, D3 v_out, D3 v_in) {  // :271-287
    const double abs_dot_nl = fabs(v_in.y), abs_dot_nv = fabs(v_out.y);
    const double roughness = P.roughness * P.roughness;
    const double rr = 0.5 + 2.0 * abs_dot_nl * abs_dot_nl * roughness;
    const double fl = schlick_weight(abs_dot_nl), fv = schlick_weight(abs_dot_nv);
    return rr * (fl + fv + fl * fv * (rr - 1.0));
}
__device__ __forceinline__ double evaluate_disney_diffuse(const Params& P, D3 v_out, D3 h, D3 v_in, bool thin) {  // :235-269
    const double abs_dot_nl = fabs(v_in.y), abs_dot_nv = fabs(v_out.y);
    const double fl = schlick_weight(abs_dot_nl), fv = schlick_weight(abs_dot_nv);
    double hanrahan_krueger = 0.0;
    if (thin && P.flatness > 0.0) {
        const double roughness = P.roughness * P.roughness;
        const double dot_hl = dot(h, v_in);
        const double fss90 = dot_hl * dot_hl * roughness;
        const double fss = lerp(1.0, fss90, fl) * lerp(1.0, fss90, fv);
        hanrahan_krueger = 1.25 * (fss * (1.0 / (abs_dot_nl + abs_dot_nv) - 0.5) + 0.5);
    }
    const double lambert = 1.0;
    const double retro = evaluate_disney_retro_diffuse(P, v_out, v_in);
    const double subsurface_approx = lerp(lambert, hanrahan_krueger, thin ? P.flatness : 0.0);
    return 1.0 / PI * (retro + subsurface_approx * (1.0 - 0.5 * fl) * (1.0 - 0.5 * fv));
}
// :403-422 -> (p_specular, p_diffuse, p_clearcoat, p_spec_trans)
__device__ __forceinline__ void calculate_lobe_pdfs(const Params& P, double& p_specular, double& p_diffuse,
                                                    double& p_clearcoat, double& p_spec_trans) {
    const double metallic_brdf = P.metallic;
    const double specular_bsdf = (1.0 - P.metallic) * P.spec_trans;
    const double dielectric_brdf = (1.0 - P.spec_trans) * (1.0 - P.metallic);
    const double specular_weight = metallic_brdf + dielectric_brdf;
    const double transmission_weight = specular_bsdf;
    const double diffuse_weight = dielectric_brdf;
    const double clearcoat_weight = 1.0 * clampd(P.clearcoat, 0.0, 1.0);
    const double norm = 1.0 / (specular_weight + transmission_weight + diffuse_weight + clearcoat_weight);
    p_specular = specular_weight * norm;
    p_spec_trans = transmission_weight * norm;
    p_diffuse = diffuse_weight * norm;
    p_clearcoat = clearcoat_weight * norm;
}

// ---------------------------------------------------------------- Disney::evaluate_disney (disney.rs:289-401)
// v_out, v_in in the shading frame (y = the normal)
RT_DISNEY_FN void evaluate_disney(const Params& P, D3 v_out, D3 v_in, bool front_face, D3& reflectance_out,
                                  double& forward_pdf_out, double& reverse_pdf_out, bool& panic) {
    const double relative_ior = front_face ? P.ior : 1.0 / P.ior;
    const double dot_nv = v_out.y, dot_nl = v_in.y;
    const bool is_transmission = dot_nv * dot_nl < 0.0;
    bool ok;
    const D3 h = unit(is_transmission ? v_in - v_out : v_in + v_out, ok);
    if (!ok) panic = true;  // "The half veator can't be normalized!"
    D3 reflectance = d3(0.0, 0.0, 0.0);
    double forward_pdf = 0.0, reverse_pdf = 0.0;
    double p_brdf, p_diffuse, p_clearcoat, p_spec_trans;
    calculate_lobe_pdfs(P, p_brdf, p_diffuse, p_clearcoat, p_spec_trans);
    const double metallic = P.metallic, spec_trans = P.spec_trans;
    const double diffuse_weight = (1.0 - metallic) * (1.0 - spec_trans);
    const double trans_weight = (1.0 - metallic) * spec_trans;
    const bool upper_hemisphere = dot_nl > 0.0 && dot_nv > 0.0;
    if (upper_hemisphere && P.clearcoat > 0.0) {
        double clearcoat, fw, rv;
        evaluate_clearcoat(P, v_out, h, v_in, clearcoat, fw, rv);
        reflectance = reflectance + d3(clearcoat, clearcoat, clearcoat);
        forward_pdf += p_clearcoat * fw;
        reverse_pdf += p_clearcoat * rv;
    }
    if (diffuse_weight > 0.0) {
        const double fw = fabs(v_in.y), rv = fabs(v_out.y);
        const double diffuse = evaluate_disney_diffuse(P, v_out, h, v_in, P.thin);
        const D3 sheen = evaluate_sheen(P, h, v_in);
        reflectance = reflectance + diffuse_weight * (diffuse * P.base_color + sheen);
        forward_pdf += p_diffuse * fw;
        reverse_pdf += p_diffuse * rv;
    }
    if (trans_weight > 0.0) {
        const double rscaled = P.thin ? thin_transmission_roughness(P.ior, P.roughness) : P.roughness;
        double tax, tay;
        calculate_anisotropic_params(rscaled, P.anisotropic, tax, tay);
        const D3 t_v_out = is_transmission ? -v_out : v_out;
        const D3 transmission = evaluate_disney_spec_transmission(P, t_v_out, h, v_in, tax, tay, relative_ior, panic);
        reflectance = reflectance + trans_weight * transmission;
        double fw, rv;
        ggx_vndf_anisotropic_pdf(v_in, h, t_v_out, tax, tay, fw, rv, panic);
        const double dot_lh = dot(h, v_in), dot_vh = dot(h, t_v_out);
        const double jacobian = (relative_ior * relative_ior * dot_lh) / pow2(dot_lh + relative_ior * dot_vh);
        forward_pdf += p_spec_trans * fw * fabs(jacobian);
        reverse_pdf += p_spec_trans * rv * fabs(jacobian);
    }
    if (upper_hemisphere) {
        D3 specular;
        double fw, rv;
        evaluate_brdf(P, v_out, h, v_in, relative_ior, specular, fw, rv, panic);
        reflectance = reflectance + specular;
        forward_pdf += p_brdf * fw;
        reverse_pdf += p_brdf * rv;
    }
    reflectance = mulr(reflectance, fabs(dot_nl));
    if (forward_pdf == 0.0) forward_pdf = __builtin_huge_val();  // :395-398
    reflectance_out = reflectance;
    forward_pdf_out = forward_pdf;
    reverse_pdf_out = reverse_pdf;
}

// ---------------------------------------------------------------- DisneyPDF (disney.rs:516-716)
// :692-716
__device__ __forceinline__ D3 sample_ggx_vndf_anisotropic(D3 v_out, double ax, double ay, double u1, double u2, bool& panic) {
    bool ok;
    const D3 v = unit(d3(v_out.x * ax, v_out.y, v_out.z * ay), ok);
    if (!ok) panic = true;
    const D3 t1 = v.y < 0.9999999 ? cross(v, d3(0.0, 1.0, 0.0)) : d3(1.0, 0.0, 0.0);
    const D3 t2 = cross(t1, v);
    const double a = 1.0 / (1.0 + v.y);
    const double r = k_sqrt(u1);
    const double phi = u2 < a ? (u2 / a) * PI : PI + (u2 - a) / (1.0 - a) * PI;
    double sn, cs;
    k_sincos(phi, &sn, &cs);
    const double p1 = r * cs;
    const double p2 = r * sn * (u2 < a ? 1.0 : v.y);
    const D3 n = (p1 * t1 + p2 * t2) + k_sqrt(fmax(1.0 - p1 * p1 - p2 * p2, 0.0)) * v;
    const D3 res = unit(d3(ax * n.x, n.y, ay * n.z), ok);
    if (!ok) panic = true;
    return res;
}

// The PDF's state: DisneyPDF::new (:524-540) with Disney::scatter's v_out (:77)
struct Pdf {
    Onb uvw;
    D3 v_out;  // in the shading frame
    bool front_face;
};
// wo = -r_in.direction (world), not normalised
__device__ __forceinline__ Pdf pdf_new(D3 normal, D3 wo, bool front_face, bool& panic) {
    bool ok1, ok2;
    const D3 v_out = unit(wo, ok1);  // :77
    Pdf q;
    q.uvw = onb_new(normal, ok2);
    if (!ok1 || !ok2) panic = true;
    q.v_out = world_to_onb(q.uvw, v_out);
    q.front_face = front_face;
    return q;
}
__device__ __forceinline__ bool to_world(const Pdf& q, D3 v_in, D3& out, bool& panic) {
    bool ok;
    out = unit(onb_to_world(q.uvw, v_in), ok);
    if (!ok) panic = true;
    return true;
}

// DisneyPDF::generate (:672-690) with the four lobe samplers (:542-658);
// `draw()` is Random::f64.  False: None.
template <class DrawFn>
__device__ __forceinline__ bool generate_impl(const Params& P, const Pdf& q, DrawFn& draw, D3& out, bool& panic) {
    double p_specular, p_diffuse, p_clearcoat, p_transmission;
    calculate_lobe_pdfs(P, p_specular, p_diffuse, p_clearcoat, p_transmission);
    const double p = draw();
    const D3 v_out = q.v_out;
    bool ok;
    if (p <= p_specular) {  // sample_disney_brdf (:542-558)
        double ax, ay;
        calculate_anisotropic_params(P.roughness, P.anisotropic, ax, ay);
        const double r0 = draw(), r1 = draw();
        const D3 h = sample_ggx_vndf_anisotropic(v_out, ax, ay, r0, r1, panic);
        const D3 v_in = unit(reflect2(v_out, h), ok);
        if (!ok) panic = true;
        if (v_in.y <= 0.0) return false;
        return to_world(q, v_in, out, panic);
    }
    if (p <= p_specular + p_clearcoat) {  // sample_disney_clearcoat (:560-587)
        const double a = 0.25;
        const double a2 = a * a;
        const double r0 = draw(), r1 = draw();
        const double cos_theta = k_sqrt(fmax((1.0 - rtcr::pow_2m4(1.0 - r0)) / (1.0 - a2), 0.0));
        const double sin_theta = k_sqrt(fmax(1.0 - cos_theta * cos_theta, 0.0));
        double sn, cs;
        k_sincos_2pi(r1, &sn, &cs);  // phi = 2.0 * PI * r1
        D3 h = d3(sin_theta * cs, cos_theta, sin_theta * sn);
        if (dot(h, v_out) < 0.0) h = -h;
        const D3 v_in = reflect2(v_out, h);  // not normalised
        if (dot(v_in, v_out) < 0.0) return false;
        return to_world(q, v_in, out, panic);
    }
    if (p <= p_specular + p_diffuse + p_clearcoat) {  // sample_disney_diffuse (:589-605)
        const double sign = signum(v_out.y);
        const double r1 = draw(), r2 = draw();  // random_cosine_direction (vec3.rs:333-343)
        double sn, cs;
        k_sincos_2pi(r1, &sn, &cs);
        const double sr2 = k_sqrt(r2);
        D3 v_in = sign * d3(sn * sr2, k_sqrt(1.0 - r2), cs * sr2);
        if (draw() <= P.diff_trans) v_in = -v_in;
        if (v_in.y == 0.0) return false;
        return to_world(q, v_in, out, panic);
    }
    if (p_transmission >= 0.0) {  // disney_spec_transmission (:607-658)
        const double ior = q.front_face ? P.ior : 1.0 / P.ior;
        if (v_out.y == 0.0) return false;
        const double rscaled = P.thin ? thin_transmission_roughness(ior, P.roughness) : P.roughness;
        double tax, tay;
        calculate_anisotropic_params(rscaled, P.anisotropic, tax, tay);
        const double r0 = draw(), r1 = draw();
        const D3 h = sample_ggx_vndf_anisotropic(v_out, tax, tay, r0, r1, panic);
        double dot_vh = dot(v_out, h);
        if (h.y < 0.0) dot_vh = -dot_vh;
        const double ni = v_out.y > 0.0 ? 1.0 : ior;
        const double nt = v_out.y > 0.0 ? ior : 1.0;
        const double relative_ior = ni / nt;
        const double f = dielectric(dot_vh, 1.0, P.ior);
        D3 v_in;
        if (draw() <= f) {
            v_in = unit(reflect2(v_out, h), ok);
            if (!ok) panic = true;
        } else if (P.thin) {
            const D3 wi = reflect2(v_out, h);
            v_in = unit(d3(wi.x, -wi.y, wi.z), ok);
            if (!ok) panic = true;
        } else if (!refract2(v_out, h, relative_ior, v_in)) {
            v_in = unit(reflect2(v_out, h), ok);
            if (!ok) panic = true;
        }
        if (v_in.y == 0.0) return false;
        return to_world(q, v_in, out, panic);
    }
    panic = true;  // "The conditions should be exhausted!"
    return false;
}

// DisneyPDF::value (:662-670): direction in world space
__device__ __forceinline__ void pdf_value(const Params& P, const Pdf& q, D3 direction, D3& f, double& pdf, bool& panic) {
    bool ok;
    const D3 v_in = world_to_onb(q.uvw, unit(direction, ok));
    if (!ok) panic = true;
    double rev;
    evaluate_disney(P, q.v_out, v_in, q.front_face, f, pdf, rev, panic);
}

// the path's generate: the draws from the vertex's stream
struct RngDraw {
    Rng& rng;
    uint32_t& ovf;
    __device__ __forceinline__ double operator()() { return rng.next(ovf); }
};
RT_DISNEY_FN bool generate(const Params& P, const Pdf& q, Rng& rng, uint32_t& ovf, D3& out, bool& panic) {
    RngDraw d{rng, ovf};
    return generate_impl(P, q, d, out, panic);
}
// the self-test's: the draws given
struct ArrayDraw {
    const double* u;
    int n;
    __device__ __forceinline__ double operator()() { return u[n++]; }
};

}  // namespace disney
}  // namespace rtk
