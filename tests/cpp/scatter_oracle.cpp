// tests/cpp/scatter_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The oracle's side of rt_world_scatter: tests/cpp/radiance_oracle.cpp (the
// oracle's C ABI with the Disney and Portal materials and the radiance driver)
// plus
//   orcx_world_scatter -- one ray_color level (camera.rs:286-316) for a batch
//     of caller-given rays, without the recursion and without the lights mix:
//     begin_vertex(vertex), world.hit, rec.mat->emitted, rec.mat->scatter, then
//     the PDF's generate() and value(), and value(eval_dir), in that order.
// Built at test time by tests/scatter_query.py (g++ -ffp-contract=off, with
// -DORC_CRMATH and without) and loaded through capi.Api(..., "orc_").
//
// rays8: n x {origin[3], dir[3], time, t_max}; eval_dirs3: n x 3 or NULL;
// indices: n or NULL.  out: n rt_scatter, the product's layout.  Ray i runs
// under PathRng{seed, pixel = indices ? indices[i] : first_index + i, sample};
// `draws` is rng.slot after the level.  hit.mat is the index of rec.mat in the
// scene's material table by pointer, -1 when it is not there (the tests do not
// compare it); RT_HIT_MEDIUM as tests/cpp/hit_query_oracle.cpp tells it.  A
// Panic thrown anywhere after the hit leaves `hit`, flags = RT_SCATTER_PANIC
// and zeros.
#include <cstring>

#include "radiance_oracle.cpp"

namespace {
void put3(double* o, const Vec3& v) { o[0] = v[0], o[1] = v[1], o[2] = v[2]; }
}  // namespace

extern "C" int32_t orcx_world_scatter(rt_scene* s, int32_t world, int32_t bg_tex, uint64_t seed, uint32_t sample,
                                      uint32_t vertex, uint32_t first_index, const double* rays8,
                                      const double* eval_dirs3, const uint32_t* indices, uint64_t n, rt_scatter* out) {
    if (!s || (n && (!rays8 || !out))) return fail(RT_EINVAL, "null");
    if (vertex < 1 || vertex >= (1u << 28)) return fail(RT_EINVAL, "vertex must be in [1, 2^28)");
    if (n >= (1ull << 32) || (!indices && n > (1ull << 32) - first_index)) return fail(RT_EINVAL, "n");
    int32_t rc;
    if ((rc = s->check_obj(world)) != RT_OK) return rc;
    if (bg_tex != -1 && !s->tex_ok(bg_tex)) return fail(RT_EHANDLE, "unknown background");
    GUARD_BEGIN
    Camera cam;
    cam.background = bg_tex == -1 ? nullptr : s->tex[bg_tex];
    const Hittable& w = *s->obj[world];
    PathRng rng;
    rng.seed = seed;
    rng.sample = sample;
    RngScope scope(&rng);
    for (uint64_t i = 0; i < n; ++i) {
        const double* q = rays8 + 8 * i;
        rt_scatter o;
        std::memset(&o, 0, sizeof o);
        o.hit.mat = -1;
        const Ray r(Point3(q[0], q[1], q[2]), Vec3(q[3], q[4], q[5]), q[6]);
        rng.pixel = indices ? indices[i] : first_index + (uint32_t)i;
        try {
            rng.begin_vertex(vertex);
            const std::optional<HitRecord> rec = w.hit(r, Interval::range(1e-8, q[7]));
            if (!rec) {
                put3(o.emitted, cam.background_value(r));
            } else {
                o.hit.t = rec->t;
                put3(o.hit.p, rec->p);
                put3(o.hit.normal, rec->normal);
                o.hit.u = rec->u;
                o.hit.v = rec->v;
                for (size_t k = 0; k < s->mat.size(); ++k)
                    if (s->mat[k].get() == rec->mat) {
                        o.hit.mat = (int32_t)k;
                        break;
                    }
                const bool medium = o.hit.mat < 0 && dynamic_cast<const Isotropic*>(rec->mat) != nullptr;
                o.hit.flags = RT_HIT_FOUND | (rec->front_face ? RT_HIT_FRONT_FACE : 0u) | (medium ? RT_HIT_MEDIUM : 0u);
                put3(o.emitted, rec->mat->emitted(r, *rec));
                const std::optional<ScatterRecord> sr = rec->mat->scatter(r, *rec);
                if (sr && sr->is_pdf()) {
                    o.flags = RT_SCATTER_PDF;
                    const std::optional<Vec3> gen = sr->pdf->generate();
                    if (gen) {
                        const auto [f, pdf] = sr->pdf->value(*gen);
                        put3(o.origin, rec->p);
                        put3(o.dir, *gen);
                        put3(o.f, f);
                        o.pdf = pdf;
                    } else {
                        o.flags |= RT_SCATTER_NO_SAMPLE;
                    }
                    if (eval_dirs3) {
                        const double* e = eval_dirs3 + 3 * i;
                        const auto [f, pdf] = sr->pdf->value(Vec3(e[0], e[1], e[2]));
                        put3(o.eval_f, f);
                        o.eval_pdf = pdf;
                        o.flags |= RT_SCATTER_EVAL;
                    }
                } else if (sr) {
                    o.flags = RT_SCATTER_RAY;
                    put3(o.f, sr->attenuation);
                    put3(o.origin, sr->ray.orig);
                    put3(o.dir, sr->ray.dir);
                }
            }
            o.draws = rng.slot;
        } catch (const Panic&) {
            const rt_hit_record hit = o.hit;
            std::memset(&o, 0, sizeof o);
            o.hit = hit;
            o.flags = RT_SCATTER_PANIC;
        }
        out[i] = o;
    }
    return RT_OK;
    GUARD_END
}
