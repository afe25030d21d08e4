// tests/cpp/lights_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The oracle's side of rt_lights_pdf and rt_lights_sample: the oracle's C ABI
// (oracle/rt_oracle_capi.cpp, reached through the hit-query driver, whose
// orcx_world_hit the lights tests use too: a sampled direction must hit the
// lights object) plus two entry points that call Hittable::pdf_value and
// Hittable::random (hit.rs:46-60) on a scene's object for a batch of points,
// so that the same rt.Scene builders drive the product and the oracle and the
// results can be compared bit for bit (tests/lights_query.py builds this file
// with oracle/rt_oracle.cpp and oracle/rt_oracle_obj.cpp, -DORC_CRMATH, and
// loads it through capi.Api(..., "orc_")).
//
// orcx_lights_pdf: out[i] = lights.pdf_value(origin_i, dir_i).  The one panic
// pdf_value has -- Hittables::pdf_value's "The sum of pdf is NaN!"
// (hits.rs:52-67) -- is where rt_lights_pdf returns the NaN itself, so a Panic
// of an item becomes NaN.
//
// orcx_lights_sample: for origin i and sample s the thread's RNG is
// PathRng{seed, pixel = first_index + i, sample = s} at begin_vertex(1), the
// contract's main stream (oracle/rng_contract.hpp) from slot 0;
// out5[(i * samples + s) * 5 ..] = {dir[3], pdf, flags}: dir = random(origin),
// pdf = pdf_value(origin, dir).  A Panic of random (an expect that fails) makes
// the item zeros with flags = 1 (RT_LIGHT_PANIC); a Panic of pdf_value on a
// good direction makes pdf NaN, as above, without the flag.
#include "hit_query_oracle.cpp"

namespace {
double pdf_or_nan(const Hittable& l, const Point3& o, const Vec3& d) {
    try {
        return l.pdf_value(o, d);
    } catch (const Panic&) {
        return std::numeric_limits<double>::quiet_NaN();
    }
}
}  // namespace

extern "C" int32_t orcx_lights_pdf(rt_scene* s, int32_t lights, const double* origins3, const double* dirs3, uint64_t n,
                                   double* out) {
    if (!s || (n && (!origins3 || !dirs3 || !out))) return fail(RT_EINVAL, "null");
    int32_t rc = s->check_obj(lights);
    if (rc != RT_OK) return rc;
    GUARD_BEGIN
    const Hittable& l = *s->obj[lights];
    for (uint64_t i = 0; i < n; ++i) out[i] = pdf_or_nan(l, v3(origins3 + 3 * i), v3(dirs3 + 3 * i));
    return RT_OK;
    GUARD_END
}

extern "C" int32_t orcx_lights_sample(rt_scene* s, int32_t lights, uint64_t seed, uint32_t first_index, uint32_t samples,
                                      const double* origins3, uint64_t n, double* out5) {
    if (!s || (n && (!origins3 || !out5))) return fail(RT_EINVAL, "null");
    if (samples == 0) return fail(RT_EINVAL, "samples must be at least 1");
    if (n > (1ull << 32) - first_index) return fail(RT_EINVAL, "first_index + n must not pass 2^32");
    int32_t rc = s->check_obj(lights);
    if (rc != RT_OK) return rc;
    GUARD_BEGIN
    const Hittable& l = *s->obj[lights];
    for (uint64_t i = 0; i < n; ++i) {
        const Point3 o = v3(origins3 + 3 * i);
        for (uint32_t k = 0; k < samples; ++k) {
            double* q = out5 + (i * samples + k) * 5;
            for (int c = 0; c < 5; ++c) q[c] = 0.0;
            PathRng rng;
            rng.seed = seed;
            rng.pixel = first_index + (uint32_t)i;
            rng.sample = k;
            rng.begin_vertex(1);
            current_rng() = &rng;
            struct Reset {
                ~Reset() { current_rng() = nullptr; }
            } reset;
            try {
                const Vec3 d = l.random(o);
                q[0] = d.x(), q[1] = d.y(), q[2] = d.z();
            } catch (const Panic&) {
                q[4] = 1.0;
                continue;
            }
            q[3] = pdf_or_nan(l, o, Vec3(q[0], q[1], q[2]));
        }
    }
    return RT_OK;
    GUARD_END
}
