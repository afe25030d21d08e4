// tests/cpp/edge_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// tests/cpp/obj_disney_oracle.cpp (the oracle's C ABI with the loader, the
// Disney and Portal materials and the radiance and scatter drivers) plus
//   orcx_render_partials_loop -- orc_render_partials' (pixel, s_i) sums with
//     Camera::ray_color (camera.rs:275-325) unrolled into the loop the path
//     kernel runs (csrc/rt_shade.h): the same hits, emissions, PDF draws and
//     values in the same order and under the same RNG keys, but the radiance
//     gathered front to back,
//         L += beta * emitted;  beta *= (1 / pdf) * f   (or *= attenuation),
//     instead of back to front, emitted + (f * deeper) / pdf.  The two
//     orders round differently in the last bits of a multi-bounce path, so
//     the kernel's f64 sums can equal the recursion's only to ~1e-15
//     relative; against this loop they must be equal bit for bit.
// For worlds without `lights` (the PDF is the material's own).  A panic of a
// sample (an unwrap, pdf == 0, a NaN radiance) is RT_EPANIC, as in
// orc_render: the frames compared hold none.
// Built at test time by tests/edge_query.py.
#include "obj_disney_oracle.cpp"

namespace {
Color ray_color_loop(const Camera& cam, const Ray& r0, const Hittable& world) {
    Color L, beta(1.0, 1.0, 1.0);
    Ray ray = r0;
    PathRng* rng = current_rng();
    for (uint32_t vertex = 1; vertex <= cam.max_depth; ++vertex) {
        rng->begin_vertex(vertex);
        const std::optional<HitRecord> rec = world.hit(ray, Interval::range(1e-8, INF));
        if (!rec) {
            L = L + beta * cam.background_value(ray);
            break;
        }
        const Color e = rec->mat->emitted(ray, *rec);
        if (e[0] != 0.0 || e[1] != 0.0 || e[2] != 0.0) L = L + beta * e;
        const std::optional<ScatterRecord> sr = rec->mat->scatter(ray, *rec);
        if (!sr) break;
        if (sr->is_pdf()) {
            const std::optional<Vec3> gen = sr->pdf->generate();
            if (!gen) break;
            const auto [f, pdf] = sr->pdf->value(*gen);
            if (pdf == 0.0) throw Panic("assert_ne!(pdf_value, 0.0)");
            beta = beta * ((1.0 / pdf) * f);
            ray = Ray(rec->p, *gen, ray.time);
        } else {
            beta = beta * sr->attenuation;
            ray = sr->ray;
        }
    }
    if (L.any_nan()) throw Panic("ray_color returned NaN");
    return L;
}
}  // namespace

// partials: H x W x sqrt_spp x 3 doubles, orc_render_partials' layout (row_offset 0, row_stride 1).
extern "C" int32_t orcx_render_partials_loop(rt_scene* s, int32_t world, const rt_camera* c, uint64_t seed,
                                             double* partials, uint64_t n_doubles) {
    if (!s || !c || !partials) return fail(RT_EINVAL, "null");
    int32_t rc;
    if ((rc = s->check_obj(world)) != RT_OK) return rc;
    if (c->background_tex != -1 && !s->tex_ok(c->background_tex)) return fail(RT_EHANDLE, "unknown background");
    GUARD_BEGIN
    Camera cam = camera_from_abi(s, c);
    cam.initialize();
    const uint32_t W = cam.image_width, H = cam.image_height;
    if (n_doubles != (uint64_t)W * H * cam.sqrt_spp * 3) return fail(RT_EINVAL, "n_doubles must be W * H * sqrt_spp * 3");
    const Hittable& w = *s->obj[world];
    PathRng rng;
    rng.seed = seed;
    RngScope scope(&rng);
    for (uint64_t k = 0; k < (uint64_t)W * H; ++k) {
        const uint32_t i = (uint32_t)(k % W), j = (uint32_t)(k / W);
        for (uint32_t s_i = 0; s_i < cam.sqrt_spp; ++s_i) {
            Color row_sum;
            for (uint32_t s_j = 0; s_j < cam.sqrt_spp; ++s_j) {
                rng.pixel = (uint32_t)k;
                rng.sample = s_i * cam.sqrt_spp + s_j;
                rng.begin_vertex(0);
                const Ray r = cam.get_ray(i, j, s_i, s_j);
                row_sum += ray_color_loop(cam, r, w);
            }
            double* pd = partials + (k * cam.sqrt_spp + s_i) * 3;
            pd[0] = row_sum[0], pd[1] = row_sum[1], pd[2] = row_sum[2];
        }
    }
    return RT_OK;
    GUARD_END
}
