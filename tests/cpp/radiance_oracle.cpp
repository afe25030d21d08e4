// tests/cpp/radiance_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The oracle's side of rt_world_radiance: the oracle's C ABI with the Disney
// and Portal materials (tests/cpp/portal_oracle.cpp, which includes
// tests/cpp/disney_oracle.cpp and through it oracle/rt_oracle_capi.cpp) plus
//   orcx_world_radiance -- Camera::ray_color (camera.rs:275-325) for a batch of
//     caller-given rays, so that the same rt.Scene builders drive the product
//     and the oracle and the radiances can be compared ray by ray;
//   orcx_camera_rays -- Camera::get_ray (camera.rs:247-273) of every pixel of a
//     1-spp frame, the rays a render would hand ray_color;
//   orcx_first_hit -- t of each ray's first world.hit over [1e-8, inf), for the
//     tests that build and describe their ray sets (which rays miss, where a
//     finite t_max cuts).
// Built at test time by tests/radiance_query.py (g++ -ffp-contract=off, once
// with -DORC_CRMATH and once without, with oracle/rt_oracle.cpp and
// oracle/rt_oracle_obj.cpp) and loaded through capi.Api(..., "orc_").
//
// rays8: n x {origin[3], dir[3], time, t_max}.  out5: n x {r, g, b, rays,
// panics}: (the sum over the samples, ascending from zero) * (1.0 / samples),
// the ray_color calls that reached world.hit, and the samples that panicked.
// Sample s of ray i runs under PathRng{seed, pixel = first_index + i,
// sample = s}; ray_color itself begins vertex k at its k-th call
// (oracle/rt_oracle.cpp).  The Camera holds max_depth and the background only:
// ray_color reads nothing else of it.
//
// t_max bounds the first world.hit only.  For a finite t_max the first hit is
// asked for on its own, world.hit(r, [1e-8, t_max]) at vertex 1: None is a
// miss, background_value(r) and one call; Some means the closest hit overall
// lies within t_max, so ray_color's own first hit over [1e-8, inf) is that hit
// -- a ConstantMedium's draw is counter-based (the medium stream of the same
// vertex), so the repeat draws the same -- and ray_color runs unchanged.
//
// A sample that panics counts in `panics` and adds nothing here: the
// recursion holds no "radiance so far" to hand back.  The tests require zero
// oracle panics of the ray sets they compare.
#include "portal_oracle.cpp"

namespace {
Camera camera_from_abi(rt_scene* s, const rt_camera* c) {
    Camera cam;
    cam.aspect_ratio = c->aspect_ratio;
    cam.image_width = c->image_width;
    cam.samples_per_pixel = c->samples_per_pixel;
    cam.max_depth = c->max_depth;
    cam.background = c->background_tex == -1 ? nullptr : s->tex[c->background_tex];
    cam.vertical_fov_in_degrees = c->vertical_fov_in_degrees;
    cam.look_from = v3(c->look_from);
    cam.look_at = v3(c->look_at);
    cam.vec_up = v3(c->vec_up);
    cam.defocus_angle_in_degrees = c->defocus_angle_in_degrees;
    cam.focus_distance = c->focus_distance;
    return cam;
}
struct RngScope {
    explicit RngScope(PathRng* r) { current_rng() = r; }
    ~RngScope() { current_rng() = nullptr; }
};
}  // namespace

extern "C" int32_t orcx_world_radiance(rt_scene* s, int32_t world, int32_t lights, int32_t bg_tex, uint32_t max_depth,
                                       uint32_t samples, uint64_t seed, uint32_t first_index, const double* rays8,
                                       uint64_t n, double* out5) {
    if (!s || (n && (!rays8 || !out5))) return fail(RT_EINVAL, "null");
    if (samples == 0) return fail(RT_EINVAL, "samples must be at least 1");
    if (n > (1ull << 32) - first_index) return fail(RT_EINVAL, "first_index + n must not pass 2^32");
    int32_t rc;
    if ((rc = s->check_obj(world)) != RT_OK) return rc;
    if (lights != -1 && (rc = s->check_obj(lights)) != RT_OK) return rc;
    if (bg_tex != -1 && !s->tex_ok(bg_tex)) return fail(RT_EHANDLE, "unknown background");
    GUARD_BEGIN
    Camera cam;
    cam.max_depth = max_depth;
    cam.background = bg_tex == -1 ? nullptr : s->tex[bg_tex];
    const Hittable& w = *s->obj[world];
    const Hittable* l = lights == -1 ? nullptr : s->obj[lights].get();
    PathRng rng;
    rng.seed = seed;
    RngScope scope(&rng);
    for (uint64_t i = 0; i < n; ++i) {
        const double* q = rays8 + 8 * i;
        double* o = out5 + 5 * i;
        const Ray r(Point3(q[0], q[1], q[2]), Vec3(q[3], q[4], q[5]), q[6]);
        Color sum;
        uint64_t calls = 0, panics = 0;
        rng.pixel = first_index + (uint32_t)i;
        for (uint32_t k = 0; k < samples; ++k) {
            rng.sample = k;
#ifndef ORC_NO_COUNTS
            const uint64_t before = work().ray_color_calls;
#endif
            try {
                Color c;
                bool missed = false;
                if (max_depth > 0 && q[7] < INF) {
                    rng.begin_vertex(1);
                    missed = !w.hit(r, Interval::range(1e-8, q[7]));
                }
                if (missed) {
                    c = cam.background_value(r);
                    ++calls;
                } else {
                    c = cam.ray_color(r, max_depth, w, l);
                }
                sum += c;
            } catch (const Panic&) {
                ++panics;
            }
#ifndef ORC_NO_COUNTS
            calls += work().ray_color_calls - before;
#endif
        }
        const Color mean = sum * (1.0 / (double)samples);
        o[0] = mean[0], o[1] = mean[1], o[2] = mean[2];
        o[3] = (double)calls;
        o[4] = (double)panics;
    }
    return RT_OK;
    GUARD_END
}

// The camera rays of a frame at one sample a pixel: rays8[(j * W + i) * 8 ..]
// = cam.get_ray(i, j, 0, 0) under PathRng{seed, pixel = j * W + i, sample 0,
// vertex 0}, t_max = +inf -- what Camera::render hands ray_color for that
// pixel (oracle/rt_oracle.cpp render).  n_rays must be W * H.
extern "C" int32_t orcx_camera_rays(rt_scene* s, const rt_camera* c, uint64_t seed, double* rays8, uint64_t n_rays) {
    if (!s || !c || !rays8) return fail(RT_EINVAL, "null");
    if (c->image_width == 0 || !(c->aspect_ratio > 0)) return fail(RT_EINVAL, "bad image size");
    if (c->background_tex != -1 && !s->tex_ok(c->background_tex)) return fail(RT_EHANDLE, "unknown background");
    GUARD_BEGIN
    Camera cam = camera_from_abi(s, c);
    cam.initialize();
    const uint32_t W = cam.image_width, H = cam.image_height;
    if (n_rays != (uint64_t)W * H) return fail(RT_EINVAL, "n_rays must be W * H");
    PathRng rng;
    rng.seed = seed;
    RngScope scope(&rng);
    for (uint32_t j = 0; j < H; ++j)
        for (uint32_t i = 0; i < W; ++i) {
            rng.pixel = j * W + i;
            rng.sample = 0;
            rng.begin_vertex(0);
            const Ray r = cam.get_ray(i, j, 0, 0);
            double* o = rays8 + 8 * ((uint64_t)j * W + i);
            o[0] = r.orig[0], o[1] = r.orig[1], o[2] = r.orig[2];
            o[3] = r.dir[0], o[4] = r.dir[1], o[5] = r.dir[2];
            o[6] = r.time;
            o[7] = INF;
        }
    return RT_OK;
    GUARD_END
}

// t of world.hit(r, [1e-8, inf)) for each ray -- the first hit of ray_color's
// sample 0, under PathRng{seed, pixel = first_index + i, sample 0, vertex 1}
// -- or -1 for a miss.  The rays' own t_max is not read.
extern "C" int32_t orcx_first_hit(rt_scene* s, int32_t world, uint64_t seed, uint32_t first_index, const double* rays8,
                                  uint64_t n, double* out_t) {
    if (!s || (n && (!rays8 || !out_t))) return fail(RT_EINVAL, "null");
    int32_t rc = s->check_obj(world);
    if (rc != RT_OK) return rc;
    GUARD_BEGIN
    const Hittable& w = *s->obj[world];
    PathRng rng;
    rng.seed = seed;
    RngScope scope(&rng);
    for (uint64_t i = 0; i < n; ++i) {
        const double* q = rays8 + 8 * i;
        rng.pixel = first_index + (uint32_t)i;
        rng.sample = 0;
        rng.begin_vertex(1);
        const auto rec = w.hit(Ray(Point3(q[0], q[1], q[2]), Vec3(q[3], q[4], q[5]), q[6]), Interval::range(1e-8, INF));
        out_t[i] = rec ? rec->t : -1.0;
    }
    return RT_OK;
    GUARD_END
}
