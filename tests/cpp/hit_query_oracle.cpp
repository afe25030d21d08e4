// tests/cpp/hit_query_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The oracle's side of rt_world_hit: the oracle's C ABI (oracle/rt_oracle_capi.cpp,
// included here to reach its rt_scene) plus one entry point that calls
// Hittable::hit (hit.rs:46-60) on a scene's object for a batch of rays, so that
// the same rt.Scene builders drive the product and the oracle and the records
// can be compared field by field (tests/test_world_hit_*.py build this file with
// oracle/rt_oracle.cpp and oracle/rt_oracle_obj.cpp, -DORC_CRMATH as
// liboracle_cr.so, and load it through capi.Api(..., "orc_")).
//
// rays8: n x {origin[3], dir[3], time, t_max}.  out12: n x {t, p[3], normal[3],
// u, v, mat, flags, 0} -- mat the index of rec.mat in the scene's material
// table by pointer, -1 when it is not there (a ConstantMedium's own Isotropic,
// an OBJ triangle's RemappedMaterial); flags as rt_hit_record's: 1 found,
// 2 front_face, 4 a ConstantMedium's hit.  The record's material tells the
// last: a medium answers with its own phase function, an Isotropic that no
// table holds (volume.rs:67-72).  A miss is twelve zeros but mat = -1.
// Per ray the thread's RNG is PathRng{seed, pixel = i, sample = 0, vertex = 1}:
// the one draw a ConstantMedium makes per test (volume.rs:58) is the contract's
// medium stream there (oracle/rng_contract.hpp).
#include "../../oracle/rt_oracle_capi.cpp"

extern "C" int32_t orcx_world_hit(rt_scene* s, int32_t world, uint64_t seed, const double* rays8, uint64_t n,
                                  double* out12) {
    if (!s || (n && (!rays8 || !out12))) return fail(RT_EINVAL, "null");
    if (n >= (1ull << 32)) return fail(RT_EINVAL, "n must be below 2^32");
    int32_t rc = s->check_obj(world);
    if (rc != RT_OK) return rc;
    GUARD_BEGIN
    const Hittable& w = *s->obj[world];
    for (uint64_t i = 0; i < n; ++i) {
        const double* q = rays8 + 8 * i;
        double* o = out12 + 12 * i;
        for (int k = 0; k < 12; ++k) o[k] = 0.0;
        o[9] = -1.0;
        PathRng rng;
        rng.seed = seed;
        rng.pixel = (uint32_t)i;
        rng.sample = 0;
        rng.begin_vertex(1);
        current_rng() = &rng;
        struct Reset {
            ~Reset() { current_rng() = nullptr; }
        } reset;
        const Ray r(Point3(q[0], q[1], q[2]), Vec3(q[3], q[4], q[5]), q[6]);
        const std::optional<HitRecord> rec = w.hit(r, Interval::range(1e-8, q[7]));
        if (!rec) continue;
        o[0] = rec->t;
        o[1] = rec->p.x(), o[2] = rec->p.y(), o[3] = rec->p.z();
        o[4] = rec->normal.x(), o[5] = rec->normal.y(), o[6] = rec->normal.z();
        o[7] = rec->u;
        o[8] = rec->v;
        int32_t mat = -1;
        for (size_t k = 0; k < s->mat.size(); ++k)
            if (s->mat[k].get() == rec->mat) {
                mat = (int32_t)k;
                break;
            }
        o[9] = (double)mat;
        const bool medium = mat < 0 && dynamic_cast<const Isotropic*>(rec->mat) != nullptr;
        o[10] = (double)(1u | (rec->front_face ? 2u : 0u) | (medium ? 4u : 0u));
    }
    return RT_OK;
    GUARD_END
}
