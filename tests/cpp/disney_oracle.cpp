// tests/cpp/disney_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The oracle's side of the Disney BSDF: the oracle's C ABI
// (oracle/rt_oracle_capi.cpp, included here to reach its rt_scene) plus
//   orc::Disney : orc::Material and orc::DisneyPDF : orc::PDF -- an f64 C++
//     restatement of material/disney.rs, utils/fresnel.rs and the UnitVec3 /
//     OrthonormalBasis helpers they call, on the oracle's Vec3 / ONB / Random,
//     written from the reference's lines (cited), not from rt_disney.h;
//   orc_disney_params_default / orc_mat_disney -- the constructor under the
//     oracle's prefix, so that one rt.Scene script drives product and oracle
//     (capi.Api(lib, "orc_", ...));
//   orcx_disney_selftest -- rt_disney_selftest's in / out layout on the host.
// Built at test time by tests/disney_query.py (g++ -ffp-contract=off
// -DORC_CRMATH, with oracle/rt_oracle.cpp and oracle/rt_oracle_obj.cpp); the
// transcendentals go through orc::m (rt_crmath.h), 0.0625^y through
// rtcr::pow_2m4.
#include "../../oracle/rt_oracle_capi.cpp"

#include <tuple>

#ifndef ORC_CRMATH
#include "../../raytracer-2025_amd/csrc/rt_crmath.h"
#endif

namespace orc {

// DisneyParameters (disney.rs:17-34)
struct DisneyParameters {
    Color base_color = Color(0.8, 0.8, 0.8);
    double roughness = 0.5, anisotropic = 0.0, sheen = 0.0, sheen_tint = 0.0, clearcoat = 0.0, clearcoat_gloss = 0.0,
           specular_tint = 0.0, metallic = 0.0, ior = 1.45, flatness = 0.0, spec_trans = 0.0, diff_trans = 0.0;
    bool thin = false;
};

namespace dz {
// ---- f64 methods as Rust defines them
inline double powi(double x, int n) {  // compiler-rt __powidf2 (n >= 0 here)
    double r = 1.0;
    for (;;) {
        if (n & 1) r *= x;
        n /= 2;
        if (n == 0) break;
        x *= x;
    }
    return r;
}
inline double clamp(double x, double lo, double hi) {  // f64::clamp: NaN stays NaN
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return x;
}
inline double signum(double x) { return std::isnan(x) ? x : std::copysign(1.0, x); }
// utils.rs:14-19 lerp: a * (1.0 - t) + b * t
inline double lerp(double a, double b, double t) { return a * (1.0 - t) + b * t; }
inline Vec3 lerp(const Vec3& a, const Vec3& b, double t) { return a * (1.0 - t) + b * t; }

// ---- UnitVec3 (vec3.rs:291-431): a Vec3 assumed unit, with the accessors the BSDF calls
struct U3 {
    Vec3 v;
    U3() = default;
    explicit U3(const Vec3& raw) : v(raw) {}  // from_vec3_raw
    static U3 make(const Vec3& x, const char* what) { return U3(expect_unit(x, what)); }  // from_vec3(..).unwrap()
    double x() const { return v.x(); }
    double y() const { return v.y(); }
    double z() const { return v.z(); }
    double dot(const U3& o) const { return v.dot(o.v); }
    U3 operator-() const { return U3(-v); }
    double cos_theta() const { return y(); }                                   // :376-378
    double cos_theta2() const { return y(); }                                  // :380-382 (y, not y^2)
    double sin_theta2() const { return clamp(1.0 - cos_theta2(), 0.0, 1.0); }  // :388-390
    double sin_theta() const { return std::sqrt(sin_theta2()); }               // :384-386
    double tan_theta() const { return sin_theta() / cos_theta(); }             // :392-394
    double cos_phi() const {                                                   // :400-407
        double st = sin_theta();
        return std::fabs(st) < 1e8 ? 1.0 : x() / st;
    }
    double sin_phi() const {  // :409-416
        double st = sin_theta();
        return std::fabs(st) < 1e8 ? 1.0 : z() / st;
    }
    double cos_phi2() const { return cos_phi() * cos_phi(); }
    double sin_phi2() const { return sin_phi() * sin_phi(); }
    // vec3.rs:76-78 (Vec3::reflect2 through Deref)
    Vec3 reflect2(const U3& n) const { return -v + 2.0 * v.dot(n.v) * n.v; }
    // vec3.rs:357-366
    std::optional<U3> refract2(const U3& n, double relative_eta) const {
        double cos_theta = std::fmin(dot(n), 1.0);
        Vec3 out_perp = relative_eta * (-v + cos_theta * n.v);
        double out_parallel_length = std::sqrt(1.0 - out_perp.length_squared());
        if (std::isnan(out_parallel_length)) return std::nullopt;
        Vec3 out_parallel = -out_parallel_length * n.v;
        return U3(out_perp + out_parallel);
    }
};
// onb.rs:39-45
inline Vec3 world_to_onb(const ONB& b, const Vec3& v) { return Vec3(v.dot(b.axis[0]), v.dot(b.axis[1]), v.dot(b.axis[2])); }

// ---- fresnel.rs
inline double schlick_weight(double u) { return powi(clamp(1.0 - u, 0.0, 1.0), 5); }
inline Vec3 schlick(const Vec3& r0, double radians) {
    double e = powi(1.0 - radians, 5);
    return r0 + (Vec3(1.0, 1.0, 1.0) - r0) * e;
}
inline double schlick_f64(double r0, double radians) { return lerp(1.0, schlick_weight(radians), r0); }
inline double schlick_r0_from_relative_ior(double eta) { return powi(eta - 1.0, 2) / powi(eta + 1.0, 2); }
inline double dielectric(double cos_theta_in, double n_in, double n_out) {
    cos_theta_in = clamp(cos_theta_in, -1.0, 1.0);
    if (cos_theta_in < 0.0) {
        std::swap(n_in, n_out);
        cos_theta_in = -cos_theta_in;
    }
    double sin_theta_in = std::sqrt(std::fmax(1.0 - cos_theta_in * cos_theta_in, 0.0));
    double sin_theta_out = n_in / n_out * sin_theta_in;
    if (sin_theta_out >= 1.0) return 1.0;
    double cos_theta_out = std::sqrt(std::fmax(1.0 - sin_theta_out * sin_theta_out, 0.0));
    double r_parallel = (n_out * cos_theta_in - n_in * cos_theta_out) / (n_out * cos_theta_in + n_in * cos_theta_out);
    double r_perp = (n_in * cos_theta_in - n_out * cos_theta_out) / (n_in * cos_theta_in + n_out * cos_theta_out);
    return (r_parallel * r_parallel + r_perp * r_perp) / 2.0;
}

// ---- disney.rs:425-514
inline Color calculate_tint(const Color& base_color) {
    double luminance = Color(0.3, 0.6, 1.0).dot(base_color);
    return luminance > 0.0 ? base_color * (1.0 / luminance) : Color(1.0, 1.0, 1.0);
}
inline double gtr1(double dot_hl, double a) {
    if (a >= 1.0) return 1.0 / PI;
    double a2 = a * a;
    return (a2 - 1.0) / (PI * m::log(a2) * (1.0 + (a2 - 1.0) * dot_hl * dot_hl));
}
inline double separable_smith_ggxg1(const U3& w, double a) {
    double a2 = a * a;
    double dot_nv = w.y();
    return 2.0 / (1.0 + std::sqrt(a2 + (1.0 - a2) * dot_nv * dot_nv));
}
inline double ggx_anisotropic_d(const U3& v_half, double ax, double ay) {
    double dot_hx2 = powi(v_half.x(), 2);
    double dot_hy2 = powi(v_half.z(), 2);
    double cos_theta2 = powi(v_half.y(), 2);
    double ax2 = ax * ax;
    double ay2 = ay * ay;
    return 1.0 / (PI * ax * ay * powi(dot_hx2 / ax2 + dot_hy2 / ay2 + cos_theta2, 2));
}
inline double anisotropic_separable_smith_ggxg1(const U3& w, const U3& v_half, double ax, double ay) {
    double dot_hw = w.dot(v_half);
    if (dot_hw <= 0.0) return 0.0;
    double abs_tan_theta = std::fabs(w.tan_theta());
    if (std::isnan(abs_tan_theta)) throw Panic("assert!(!abs_tan_theta.is_nan())");  // :469
    if (std::isinf(abs_tan_theta)) return 0.0;
    double a = std::sqrt(w.cos_phi2() * ax * ax + w.sin_phi2() * ay * ay);
    double a2_tan_theta2 = powi(a * abs_tan_theta, 2);
    double lambda = 0.5 * (-1.0 + std::sqrt(1.0 + a2_tan_theta2));
    return 1.0 / (1.0 + lambda);
}
inline std::pair<double, double> calculate_anisotropic_params(double roughness, double anisotropic) {
    double aspect = std::sqrt(1.0 - 0.9 * anisotropic);
    double roughness2 = roughness * roughness;
    return {std::fmax(0.001, roughness2 / aspect), std::fmax(0.001, roughness2 * aspect)};
}
inline std::pair<double, double> ggx_vndf_anisotropic_pdf(const U3& v_in, const U3& v_half, const U3& v_out, double ax,
                                                          double ay) {
    double d = ggx_anisotropic_d(v_half, ax, ay);
    double abs_dot_nv = std::fabs(v_out.cos_theta());
    double abs_dot_hv = std::fabs(v_half.dot(v_out));
    double g1v = anisotropic_separable_smith_ggxg1(v_out, v_half, ax, ay);
    double forward_pdf_weight = g1v * abs_dot_hv * d / abs_dot_nv;
    double abs_dot_nl = std::fabs(v_in.cos_theta());
    double abs_dot_hl = std::fabs(v_half.dot(v_in));
    double g1l = anisotropic_separable_smith_ggxg1(v_in, v_half, ax, ay);
    double reverse_pdf_weight = g1l * abs_dot_hl * d / abs_dot_nl;
    return {forward_pdf_weight, reverse_pdf_weight};
}
inline double thin_transmission_roughness(double ior, double roughness) {
    return clamp((0.65 * ior - 0.35) * roughness, 0.0, 1.0);
}
// vec3.rs:127-133
inline Vec3 vec_sqrt(const Vec3& c) {
    Vec3 r(std::sqrt(c.x()), std::sqrt(c.y()), std::sqrt(c.z()));
    if (r.any_nan()) throw Panic("The answer of sqrt is NaN!");
    return r;
}

// disney.rs:692-716
inline U3 sample_ggx_vndf_anisotropic(const U3& v_out, double ax, double ay, double u1, double u2) {
    U3 v = U3::make(Vec3(v_out.x() * ax, v_out.y(), v_out.z() * ay), "UnitVec3::new (vndf v)");
    U3 t1 = v.y() < 0.9999999 ? U3(v.v.cross(Vec3(0.0, 1.0, 0.0))) : U3(Vec3(1.0, 0.0, 0.0));
    Vec3 t2 = t1.v.cross(v.v);
    double a = 1.0 / (1.0 + v.y());
    double r = std::sqrt(u1);
    double phi = u2 < a ? (u2 / a) * PI : PI + (u2 - a) / (1.0 - a) * PI;
    double p1 = r * m::cos(phi);
    double p2 = r * m::sin(phi) * (u2 < a ? 1.0 : v.y());
    Vec3 n = p1 * t1.v + p2 * t2 + std::sqrt(std::fmax(1.0 - p1 * p1 - p2 * p2, 0.0)) * v.v;
    return U3::make(Vec3(ax * n.x(), n.y(), ay * n.z()), "UnitVec3::from_vec3 (vndf)");
}
}  // namespace dz

// disney.rs:59-423
struct Disney : Material {
    std::shared_ptr<Texture> base_color;  // param_fn: base_color = tex.value(u, v, p), ..params
    DisneyParameters params;
    Disney(std::shared_ptr<Texture> t, const DisneyParameters& p) : base_color(std::move(t)), params(p) {}
    std::optional<ScatterRecord> scatter(const Ray& r_in, const HitRecord& rec) const override;

    using U3 = dz::U3;
    // -> (p_specular, p_diffuse, p_clearcoat, p_spec_trans), :403-422
    static std::tuple<double, double, double, double> calculate_lobe_pdfs(const DisneyParameters& param) {
        double metallic_brdf = param.metallic;
        double specular_bsdf = (1.0 - param.metallic) * param.spec_trans;
        double dielectric_brdf = (1.0 - param.spec_trans) * (1.0 - param.metallic);
        double specular_weight = metallic_brdf + dielectric_brdf;
        double transmission_weight = specular_bsdf;
        double diffuse_weight = dielectric_brdf;
        double clearcoat_weight = 1.0 * dz::clamp(param.clearcoat, 0.0, 1.0);
        double norm = 1.0 / (specular_weight + transmission_weight + diffuse_weight + clearcoat_weight);
        return {specular_weight * norm, diffuse_weight * norm, clearcoat_weight * norm, transmission_weight * norm};
    }
    static Color disney_fresnel(const DisneyParameters& param, const U3& v_out, const U3& v_half, const U3& v_in,
                                double relative_ior) {  // :175-198
        double dot_hv = v_half.dot(v_out);
        Color tint = dz::calculate_tint(param.base_color);
        Color r0 = dz::schlick_r0_from_relative_ior(relative_ior) * dz::lerp(Vec3(1.0, 1.0, 1.0), tint, param.specular_tint);
        r0 = dz::lerp(r0, param.base_color, param.metallic);
        double dielectric_fresnel = dz::dielectric(dot_hv, 1.0, param.ior);
        Color metallic_fresnel = dz::schlick(r0, v_in.dot(v_half));
        return dz::lerp(Vec3(dielectric_fresnel, dielectric_fresnel, dielectric_fresnel), metallic_fresnel, param.metallic);
    }
    static std::tuple<Color, double, double> evaluate_brdf(const DisneyParameters& param, const U3& v_out, const U3& v_half,
                                                           const U3& v_in, double relative_ior) {  // :102-130
        double dot_nl = v_in.cos_theta();
        double dot_nv = v_out.cos_theta();
        if (dot_nl <= 0.0 || dot_nv <= 0.0) return {Color(), 0.0, 0.0};
        auto [ax, ay] = dz::calculate_anisotropic_params(param.roughness, param.anisotropic);
        double d = dz::ggx_anisotropic_d(v_half, ax, ay);
        double gl = dz::anisotropic_separable_smith_ggxg1(v_in, v_half, ax, ay);
        double gv = dz::anisotropic_separable_smith_ggxg1(v_out, v_half, ax, ay);
        Color f = disney_fresnel(param, v_out, v_half, v_in, relative_ior);
        auto [fw, rv] = dz::ggx_vndf_anisotropic_pdf(v_in, v_half, v_out, ax, ay);
        double forward_pdf = fw / (4.0 * std::fabs(v_in.dot(v_half)));
        double reverse_pdf = rv / (4.0 * std::fabs(v_out.dot(v_half)));
        Color value = d * gl * gv * f / (4.0 * dot_nl * dot_nv);
        return {value, forward_pdf, reverse_pdf};
    }
    static Color evaluate_sheen(const DisneyParameters& param, const U3& v_half, const U3& v_in) {  // :132-147
        if (param.sheen <= 0.0) return Color();
        double dot_hl = v_half.dot(v_in);
        Color tint = dz::calculate_tint(param.base_color);
        return param.sheen * dz::lerp(Vec3(1.0, 1.0, 1.0), tint, param.sheen_tint) * dz::schlick_weight(dot_hl);
    }
    static std::tuple<double, double, double> evaluate_clearcoat(const DisneyParameters& param, const U3& v_out,
                                                                 const U3& v_half, const U3& v_in) {  // :149-173
        if (param.clearcoat <= 0.0) return {0.0, 0.0, 0.0};
        double dot_nh = v_half.y();
        double dot_hl = v_half.dot(v_in);
        double d = dz::gtr1(dot_nh, dz::lerp(0.1, 0.001, param.clearcoat_gloss));
        double f = dz::schlick_f64(0.04, dot_hl);
        double gl = dz::separable_smith_ggxg1(v_in, 0.25);
        double gv = dz::separable_smith_ggxg1(v_out, 0.25);
        double value = 0.25 * param.clearcoat * d * f * gl * gv;
        double forward_pdf = d / (4.0 * std::fabs(v_in.dot(v_half)));
        double reverse_pdf = d / (4.0 * std::fabs(v_out.dot(v_half)));
        return {value, forward_pdf, reverse_pdf};
    }
    static Color evaluate_disney_spec_transmission(const DisneyParameters& param, const U3& v_out, const U3& v_half,
                                                   const U3& v_in, double ax, double ay, double relative_ior) {  // :200-233
        double n2 = relative_ior * relative_ior;
        double abs_dot_nl = std::fabs(v_in.cos_theta());
        double abs_dot_nv = std::fabs(v_out.cos_theta());
        double dot_hl = v_half.dot(v_in);
        double dot_hv = v_half.dot(v_out);
        double abs_dot_hl = std::fabs(dot_hl);
        double abs_dot_hv = std::fabs(dot_hv);
        double d = dz::ggx_anisotropic_d(v_half, ax, ay);
        double gl = dz::anisotropic_separable_smith_ggxg1(v_in, v_half, ax, ay);
        double gv = dz::anisotropic_separable_smith_ggxg1(v_out, v_half, ax, ay);
        double f = dz::dielectric(dot_hv, 1.0, 1.0 / relative_ior);
        Color color = param.thin ? dz::vec_sqrt(param.base_color) : param.base_color;
        double c = (abs_dot_hl * abs_dot_hv) / (abs_dot_nl * abs_dot_nv);
        double t = n2 / dz::powi(dot_hl + relative_ior * dot_hv, 2);
        return c * t * (1.0 - f) * gl * gv * d * color;
    }
    static double evaluate_disney_retro_diffuse(const DisneyParameters& param, const U3& v_out, const U3& v_in) {  // :271-287
        double abs_dot_nl = std::fabs(v_in.cos_theta());
        double abs_dot_nv = std::fabs(v_out.cos_theta());
        double roughness = param.roughness * param.roughness;
        double rr = 0.5 + 2.0 * abs_dot_nl * abs_dot_nl * roughness;
        double fl = dz::schlick_weight(abs_dot_nl);
        double fv = dz::schlick_weight(abs_dot_nv);
        return rr * (fl + fv + fl * fv * (rr - 1.0));
    }
    static double evaluate_disney_diffuse(const DisneyParameters& param, const U3& v_out, const U3& v_half, const U3& v_in,
                                          bool thin) {  // :235-269
        double abs_dot_nl = std::fabs(v_in.cos_theta());
        double abs_dot_nv = std::fabs(v_out.cos_theta());
        double fl = dz::schlick_weight(abs_dot_nl);
        double fv = dz::schlick_weight(abs_dot_nv);
        double hanrahan_krueger = 0.0;
        if (thin && param.flatness > 0.0) {
            double roughness = param.roughness * param.roughness;
            double dot_hl = v_half.dot(v_in);
            double fss90 = dot_hl * dot_hl * roughness;
            double fss = dz::lerp(1.0, fss90, fl) * dz::lerp(1.0, fss90, fv);
            hanrahan_krueger = 1.25 * (fss * (1.0 / (abs_dot_nl + abs_dot_nv) - 0.5) + 0.5);
        }
        double lambert = 1.0;
        double retro = evaluate_disney_retro_diffuse(param, v_out, v_in);
        double subsurface_approx = dz::lerp(lambert, hanrahan_krueger, thin ? param.flatness : 0.0);
        return 1.0 / PI * (retro + subsurface_approx * (1.0 - 0.5 * fl) * (1.0 - 0.5 * fv));
    }
    // :289-401 -> (reflectance, forward_pdf, reverse_pdf)
    static std::tuple<Color, double, double> evaluate_disney(const DisneyParameters& param, const U3& v_out, const U3& v_in,
                                                             bool front_face) {
        double relative_ior = front_face ? param.ior : 1.0 / param.ior;
        double dot_nv = v_out.cos_theta();
        double dot_nl = v_in.cos_theta();
        bool is_transmission = dot_nv * dot_nl < 0.0;
        U3 v_half = is_transmission ? U3::make(v_in.v - v_out.v, "The half veator can't be normalized!")
                                    : U3::make(v_in.v + v_out.v, "The half veator can't be normalized!");
        Color reflectance;
        double forward_pdf = 0.0, reverse_pdf = 0.0;
        auto [p_brdf, p_diffuse, p_clearcoat, p_spec_trans] = calculate_lobe_pdfs(param);
        double metallic = param.metallic;
        double spec_trans = param.spec_trans;
        double diffuse_weight = (1.0 - metallic) * (1.0 - spec_trans);
        double trans_weight = (1.0 - metallic) * spec_trans;
        bool upper_hemisphere = dot_nl > 0.0 && dot_nv > 0.0;
        if (upper_hemisphere && param.clearcoat > 0.0) {
            auto [clearcoat, fw, rv] = evaluate_clearcoat(param, v_out, v_half, v_in);
            reflectance += Vec3(clearcoat, clearcoat, clearcoat);
            forward_pdf += p_clearcoat * fw;
            reverse_pdf += p_clearcoat * rv;
        }
        if (diffuse_weight > 0.0) {
            double fw = std::fabs(v_in.cos_theta());
            double rv = std::fabs(v_out.cos_theta());
            double diffuse = evaluate_disney_diffuse(param, v_out, v_half, v_in, param.thin);
            Color sheen = evaluate_sheen(param, v_half, v_in);
            reflectance += diffuse_weight * (diffuse * param.base_color + sheen);
            forward_pdf += p_diffuse * fw;
            reverse_pdf += p_diffuse * rv;
        }
        if (trans_weight > 0.0) {
            double rscaled = param.thin ? dz::thin_transmission_roughness(param.ior, param.roughness) : param.roughness;
            auto [tax, tay] = dz::calculate_anisotropic_params(rscaled, param.anisotropic);
            U3 t_v_out = is_transmission ? -v_out : v_out;
            Color transmission = evaluate_disney_spec_transmission(param, t_v_out, v_half, v_in, tax, tay, relative_ior);
            reflectance += trans_weight * transmission;
            auto [fw, rv] = dz::ggx_vndf_anisotropic_pdf(v_in, v_half, t_v_out, tax, tay);
            double dot_lh = v_half.dot(v_in);
            double dot_vh = v_half.dot(t_v_out);
            double jacobian = (relative_ior * relative_ior * dot_lh) / dz::powi(dot_lh + relative_ior * dot_vh, 2);
            forward_pdf += p_spec_trans * fw * std::fabs(jacobian);
            reverse_pdf += p_spec_trans * rv * std::fabs(jacobian);
        }
        if (upper_hemisphere) {
            auto [specular, fw, rv] = evaluate_brdf(param, v_out, v_half, v_in, relative_ior);
            reflectance += specular;
            forward_pdf += p_brdf * fw;
            reverse_pdf += p_brdf * rv;
        }
        reflectance = reflectance * std::fabs(dot_nl);
        if (forward_pdf == 0.0) forward_pdf = INF;  // :395-398
        return {reflectance, forward_pdf, reverse_pdf};
    }
};

// disney.rs:516-690.  `draw` is Random::f64 (the self-test hands its own)
struct DisneyPDF : PDF {
    using U3 = dz::U3;
    ONB uvw;
    U3 v_out;
    bool front_face;
    DisneyParameters params;
    std::function<double()> draw;
    mutable int draws = 0;
    DisneyPDF(const Vec3& normal, const U3& v_out_world, bool ff, const DisneyParameters& p,
              std::function<double()> d = [] { return Random::f64(); })
        : uvw(normal), v_out(dz::world_to_onb(uvw, v_out_world.v)), front_face(ff), params(p), draw(std::move(d)) {}
    double next() const {
        ++draws;
        return draw();
    }
    std::optional<Vec3> to_world(const Vec3& v_in) const {
        return expect_unit(uvw.onb_to_world(v_in), "DisneyPDF: onb_to_world unwrap");
    }
    std::optional<Vec3> sample_disney_brdf() const {  // :542-558
        auto [ax, ay] = dz::calculate_anisotropic_params(params.roughness, params.anisotropic);
        double r0 = next();
        double r1 = next();
        U3 v_half = dz::sample_ggx_vndf_anisotropic(v_out, ax, ay, r0, r1);
        U3 v_in = U3::make(v_out.reflect2(v_half), "sample_disney_brdf unwrap");
        if (v_in.cos_theta() <= 0.0) return std::nullopt;
        return to_world(v_in.v);
    }
    std::optional<Vec3> sample_disney_clearcoat() const {  // :560-587
        double a = 0.25;
        double a2 = a * a;
        double r0 = next();
        double r1 = next();
        double cos_theta = std::sqrt(std::fmax((1.0 - rtcr::pow_2m4(1.0 - r0)) / (1.0 - a2), 0.0));
        double sin_theta = std::sqrt(std::fmax(1.0 - cos_theta * cos_theta, 0.0));
        double phi = 2.0 * PI * r1;
        U3 v_half(Vec3(sin_theta * m::cos(phi), cos_theta, sin_theta * m::sin(phi)));
        if (v_half.dot(v_out) < 0.0) v_half = -v_half;
        Vec3 v_in = v_out.reflect2(v_half);
        if (v_in.dot(v_out.v) < 0.0) return std::nullopt;
        return to_world(v_in);
    }
    std::optional<Vec3> sample_disney_diffuse() const {  // :589-605
        double sign = dz::signum(v_out.cos_theta());
        // random_cosine_direction (vec3.rs:333-343) on this PDF's draws
        double r1 = next();
        double r2 = next();
        double phi = 2.0 * PI * r1;
        Vec3 rcd(m::sin(phi) * std::sqrt(r2), std::sqrt(1.0 - r2), m::cos(phi) * std::sqrt(r2));
        U3 v_in(sign * rcd);
        if (next() <= params.diff_trans) v_in = -v_in;
        if (v_in.cos_theta() == 0.0) return std::nullopt;
        return to_world(v_in.v);
    }
    std::optional<Vec3> disney_spec_transmission() const {  // :607-658
        double ior = front_face ? params.ior : 1.0 / params.ior;
        if (v_out.cos_theta() == 0.0) return std::nullopt;
        double rscaled = params.thin ? dz::thin_transmission_roughness(ior, params.roughness) : params.roughness;
        auto [tax, tay] = dz::calculate_anisotropic_params(rscaled, params.anisotropic);
        double r0 = next();
        double r1 = next();
        U3 v_half = dz::sample_ggx_vndf_anisotropic(v_out, tax, tay, r0, r1);
        double dot_vh = v_out.dot(v_half);
        if (v_half.y() < 0.0) dot_vh = -dot_vh;
        double ni = v_out.y() > 0.0 ? 1.0 : ior;
        double nt = v_out.y() > 0.0 ? ior : 1.0;
        double relative_ior = ni / nt;
        double f = dz::dielectric(dot_vh, 1.0, params.ior);
        U3 v_in;
        if (next() <= f) {
            v_in = U3::make(v_out.reflect2(v_half), "spec_transmission reflect unwrap");
        } else if (params.thin) {
            Vec3 wi = v_out.reflect2(v_half);
            v_in = U3::make(Vec3(wi.x(), -wi.y(), wi.z()), "spec_transmission thin unwrap");
        } else if (auto wi = v_out.refract2(v_half, relative_ior)) {
            v_in = *wi;
        } else {
            v_in = U3::make(v_out.reflect2(v_half), "spec_transmission reflect unwrap");
        }
        if (v_in.cos_theta() == 0.0) return std::nullopt;
        return to_world(v_in.v);
    }
    std::pair<Color, double> value(const Vec3& direction) const override {  // :662-670
        U3 v_in(dz::world_to_onb(uvw, expect_unit(direction, "DisneyPDF::value unwrap")));
        auto [attenuation, f_pdf, r_pdf] = Disney::evaluate_disney(params, v_out, v_in, front_face);
        (void)r_pdf;
        return {attenuation, f_pdf};
    }
    std::optional<Vec3> generate() const override {  // :672-690
        auto [p_specular, p_diffuse, p_clearcoat, p_transmission] = Disney::calculate_lobe_pdfs(params);
        double p = next();
        if (p <= p_specular) return sample_disney_brdf();
        if (p <= p_specular + p_clearcoat) return sample_disney_clearcoat();
        if (p <= p_specular + p_diffuse + p_clearcoat) return sample_disney_diffuse();
        if (p_transmission >= 0.0) return disney_spec_transmission();
        throw Panic("The conditions should be exhausted!");
    }
};

// disney.rs:71-89
std::optional<ScatterRecord> Disney::scatter(const Ray& r_in, const HitRecord& rec) const {
    dz::U3 v_out = dz::U3::make(-r_in.dir, "Disney::scatter v_out unwrap");
    DisneyParameters p = params;
    p.base_color = base_color->value(rec.u, rec.v, rec.p);
    return pdf_record(std::make_unique<DisneyPDF>(rec.normal, v_out, rec.front_face, p));
}

}  // namespace orc

static orc::DisneyParameters disney_from_abi(const rt_disney_params* p) {
    orc::DisneyParameters d;
    d.roughness = p->roughness, d.anisotropic = p->anisotropic, d.sheen = p->sheen, d.sheen_tint = p->sheen_tint;
    d.clearcoat = p->clearcoat, d.clearcoat_gloss = p->clearcoat_gloss, d.specular_tint = p->specular_tint;
    d.metallic = p->metallic, d.ior = p->ior, d.flatness = p->flatness, d.spec_trans = p->spec_trans;
    d.diff_trans = p->diff_trans;
    d.thin = p->thin != 0;
    return d;
}

extern "C" void orc_disney_params_default(rt_disney_params* p) {  // disney.rs:36-55
    if (!p) return;
    const orc::DisneyParameters d;
    p->struct_size = (uint32_t)sizeof(rt_disney_params);
    p->thin = d.thin ? 1 : 0;
    p->roughness = d.roughness, p->anisotropic = d.anisotropic, p->sheen = d.sheen, p->sheen_tint = d.sheen_tint;
    p->clearcoat = d.clearcoat, p->clearcoat_gloss = d.clearcoat_gloss, p->specular_tint = d.specular_tint;
    p->metallic = d.metallic, p->ior = d.ior, p->flatness = d.flatness, p->spec_trans = d.spec_trans;
    p->diff_trans = d.diff_trans;
}

extern "C" int32_t orc_mat_disney(rt_scene* s, int32_t tex, const rt_disney_params* p) {
    if (!s || !p) return fail(RT_EINVAL, "null");
    if (p->struct_size < sizeof(rt_disney_params)) return fail(RT_EINVAL, "rt_disney_params.struct_size too small");
    const double* f = &p->roughness;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(f[k])) return fail(RT_EINVAL, "non-finite Disney parameter");
    if (!s->tex_ok(tex)) return fail(RT_EHANDLE, "unknown texture");
    return push_mat(s, std::make_shared<orc::Disney>(s->tex[tex], disney_from_abi(p)));
}

// rt_disney_selftest's layout (include/rt_mi355x.h): fn 0 evaluate_disney, 7
// doubles in, 6 out; fn 1 scatter's v_out + DisneyPDF::new + generate with the
// four draws given, 11 in, 6 out.  A case that panics is zeros and the flag.
extern "C" int32_t orcx_disney_selftest(int32_t fn, const rt_disney_params* params, const double base_color[3],
                                        const double* in, double* out, uint64_t n) {
    if (fn < 0 || fn > 1) return fail(RT_EINVAL, "unknown function");
    if (!params || !base_color || (n && (!in || !out))) return fail(RT_EINVAL, "null");
    orc::DisneyParameters P = disney_from_abi(params);
    P.base_color = v3(base_color);
    const int in_w = fn == 0 ? 7 : 11;
    for (uint64_t i = 0; i < n; ++i) {
        const double* p = in + i * in_w;
        double* q = out + i * 6;
        for (int k = 0; k < 6; ++k) q[k] = 0.0;
        try {
            if (fn == 0) {
                auto [refl, fwd, rev] = orc::Disney::evaluate_disney(P, orc::dz::U3(v3(p)), orc::dz::U3(v3(p + 3)), p[6] != 0.0);
                q[0] = refl.x(), q[1] = refl.y(), q[2] = refl.z(), q[3] = fwd, q[4] = rev;
            } else {
                const orc::dz::U3 v_out = orc::dz::U3::make(v3(p + 3), "Disney::scatter v_out unwrap");
                int k = 0;
                const double* u = p + 7;
                orc::DisneyPDF pdf(v3(p), v_out, p[6] != 0.0, P, [&k, u] { return u[k++]; });
                auto dir = pdf.generate();
                q[0] = dir ? 1.0 : 0.0;
                if (dir) q[1] = dir->x(), q[2] = dir->y(), q[3] = dir->z();
                q[4] = (double)pdf.draws;
            }
        } catch (const orc::Panic&) {
            for (int k = 0; k < 5; ++k) q[k] = 0.0;
            q[5] = 1.0;
        }
    }
    return RT_OK;
}
