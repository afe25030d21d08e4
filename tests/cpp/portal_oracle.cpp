// tests/cpp/portal_oracle.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The oracle's side of the Portal material: the oracle's C ABI
// (oracle/rt_oracle_capi.cpp, reached through tests/cpp/disney_oracle.cpp so
// that one library holds both extensions: a test world may mix Portal and
// Disney materials) plus
//   orc::Portal : orc::Material -- an f64 C++ restatement of
//     material/portal.rs and of the part of utils/quaternion.rs it calls, on
//     the oracle's Vec3 / Ray, written from the reference's lines (cited), not
//     from rt_geom.h's quat_rotate or rt_shade.h;
//   orc_mat_portal -- the constructor under the oracle's prefix, so that one
//     rt.Scene script drives product and oracle (capi.Api(lib, "orc_", ...)).
// Built at test time by tests/portal_query.py (g++ -ffp-contract=off
// -DORC_CRMATH, with oracle/rt_oracle.cpp and oracle/rt_oracle_obj.cpp).
#include "disney_oracle.cpp"  // includes ../../oracle/rt_oracle_capi.cpp

namespace orc {

// utils/quaternion.rs:5-11
struct PortalQuat {
    double w, x, y, z;
    // quaternion.rs:84-91
    PortalQuat conjugate() const { return PortalQuat{w, -x, -y, -z}; }
    // impl Mul, quaternion.rs:94-103: every term, left to right
    PortalQuat mul(const PortalQuat& rhs) const {
        return PortalQuat{
            w * rhs.w - x * rhs.x - y * rhs.y - z * rhs.z,
            w * rhs.x + x * rhs.w + y * rhs.z - z * rhs.y,
            w * rhs.y - x * rhs.z + y * rhs.w + z * rhs.x,
            w * rhs.z + x * rhs.y - y * rhs.x + z * rhs.w,
        };
    }
    // quaternion.rs:72-82: self * qv * self.conjugate(), the quaternion as it is (never normalised)
    Vec3 rotate_vector(const Vec3& v) const {
        const PortalQuat qv{0.0, v.x(), v.y(), v.z()};
        const PortalQuat result = mul(qv).mul(conjugate());
        return Vec3(result.x, result.y, result.z);
    }
};

// material/portal.rs:9-31.  emitted is the trait default (BLACK)
struct Portal : Material {
    Color attenuation;
    Vec3 position_offset;
    PortalQuat rotation;
    Portal(const Color& a, const Vec3& off, const PortalQuat& q) : attenuation(a), position_offset(off), rotation(q) {}
    // portal.rs:28-30 with the closure of portal.rs:18-22
    std::optional<ScatterRecord> scatter(const Ray& r_in, const HitRecord& rec) const override {
        const Point3 origin = rec.p + position_offset;
        const Vec3 direction = rotation.rotate_vector(r_in.dir);
        return ray_record(attenuation, Ray(origin, direction, r_in.time));
    }
};

}  // namespace orc

// rt_mat_portal's contract (include/rt_mi355x.h): null offset = zero, null
// quaternion = Quaternion::identity (quaternion.rs:14-21); only finiteness is checked
extern "C" int32_t orc_mat_portal(rt_scene* s, const double attenuation[3], const double* offset3,
                                  const double* quat_wxyz) {
    if (!s || !attenuation) return fail(RT_EINVAL, "null");
    double a[3], o[3] = {0.0, 0.0, 0.0}, q[4] = {1.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) a[k] = attenuation[k];
    if (offset3)
        for (int k = 0; k < 3; ++k) o[k] = offset3[k];
    if (quat_wxyz)
        for (int k = 0; k < 4; ++k) q[k] = quat_wxyz[k];
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(a[k]) || !std::isfinite(o[k])) return fail(RT_EINVAL, "non-finite Portal parameter");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(q[k])) return fail(RT_EINVAL, "non-finite Portal parameter");
    return push_mat(s, std::make_shared<orc::Portal>(orc::Color(a[0], a[1], a[2]), orc::Vec3(o[0], o[1], o[2]),
                                                     orc::PortalQuat{q[0], q[1], q[2], q[3]}));
}
