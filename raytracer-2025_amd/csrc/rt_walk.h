// rt_walk.h -- world.hit as a resumable depth-first walk: the medium boundary
// walks, the walk state (Trav) and its parking, one step of the mesh / full
// tiers' walk (trace_step), the media phase, and the LDS set-up of a kernel
// over the walk.  The 4-wide node visits it calls are rt_walk4.h's.
#pragma once
#include "rt_builds.h"
#include "rt_geom.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_slab.h"
#include "rt_stack.h"

namespace rtk {

constexpr float NO_CULL = -__builtin_huge_valf();
// The flat tier tests the f32 box of a compound list element (a Transform, a
// ConstantMedium, a nested list) before entering it, with the ray's f32 form
// made on the spot: a ray that misses the box skips the element's whole
// walk -- for C3's smoke box the two boundary walks of media_phase.  (Testing
// every element's box, primitives included, with the f32 ray parked in LDS
// was 4.6 % slower: a wall's box test costs what its exact test does.)
template <int TIER>
constexpr bool flat_boxes() { return TIER == TIER_FULL_FLAT; }
template <int TIER>
constexpr bool unified_load() {
    return TIER == TIER_MESH || tier_full_bvh(TIER);
}
// the two doubles of a float4 read from a double record
__device__ __forceinline__ double f4_lo(float4 q) { return __hiloint2double(__float_as_int(q.y), __float_as_int(q.x)); }
__device__ __forceinline__ double f4_hi(float4 q) { return __hiloint2double(__float_as_int(q.w), __float_as_int(q.z)); }
template <int TIER>
constexpr bool flat_runs() { return TIER == TIER_FULL_FLAT; }

// The flat tier's list step tests an element's f32 box (list_boxes, rounded
// outward; the conservative slab of rt_slab.h) before the element: a ray
// that misses the box within [tmin, c] cannot hit the element closer than c
// (for a ConstantMedium: cannot enter its boundary there), so skipping it
// keeps the list's closest hit -- the role a BVH node's boxes play, without
// the BVH code.
__device__ __forceinline__ bool list_box_hit(const SceneView& S, uint32_t li, const RayF& rf, float tmin_f,
                                             float c_f) {
    const RT_GLOBAL float4* bp = reinterpret_cast<const RT_GLOBAL float4*>(S.list_boxes + li);
    const float4 b0 = bp[0], b1 = bp[1];
    const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b0.w, b1.x, b1.y};
    float e;
    return slab_f(lo, hi, rf, tmin_f, c_f, e);
}

// Closest t of a medium boundary (no media inside, no records) -- the two
// boundary.hit calls of volume.rs:44-48.
template <bool BVH, class Stack>
__device__ bool boundary_t(const SceneView& S, uint32_t root, const Ray& r0, double tmin, double tmax, Stack& stk,
                           uint32_t sp0, double& tbest) {
    Ray r = r0;
    RayF rf = make_rayf(r);
    double a = len2(r.d), inva = 1.0 / a;
    XfIds xfs;
    uint32_t nxf = 0;
    uint32_t sp = sp0;
    uint32_t cur = root;
    const float tmin_f = f32_down(tmin);
    Closest cl;
    cl.set(tmax);
    bool found = false;
    for (;;) {
        if (cur == REF_NONE) {
            cur = pop(stk, sp, sp0, cl.c_f);
            if (cur == REF_NONE) break;
        }
        uint32_t after = REF_NONE;  // as trace_step: a primitive list element is tested in the list step
        if (ref_kind(cur) == K_LIST) {
            const uint32_t li = ref_idx(S, cur);
            const uint32_t child = S.list_children[li];
            cur = REF_NONE;
            if (child == REF_NONE) continue;
            const uint32_t nxt = S.list_children[li + 1] != REF_NONE ? make_ref(K_LIST, li + 1) : REF_NONE;
            const uint32_t ck = ref_kind(child);
            if (ck == K_SPHERE || ck == K_QUAD || ck == K_TRI || ck == K_MSPHERE) {
                cur = child;
                after = nxt;
            } else {
                if (nxt != REF_NONE) stk.push(sp++, nxt, NO_CULL);
                cur = child;
                continue;
            }
        }
        const uint32_t kind = ref_kind(cur), idx = ref_idx(S, cur);
        cur = REF_NONE;
        double t;
        switch (kind) {
            case K_BVH:
                if constexpr (BVH) cur = visit4_boxes(S, idx, rf, tmin_f, cl.c_f, stk, sp);
                break;
            case K_SPHERE: {
                const double4 s = S.spheres[idx];
                if (sphere_t_inv(d3(s.x, s.y, s.z), s.w, r, a, inva, tmin, cl.c, t)) {
                    cl.set(t);
                    found = true;
                }
                break;
            }
            case K_MSPHERE: {
                const double4 s = S.msph_center[idx], m = S.msph_dir[idx];
                const D3 cc = d3(s.x, s.y, s.z) + r.time * d3(m.x, m.y, m.z);
                if (sphere_t_inv(cc, s.w, r, a, inva, tmin, cl.c, t)) {
                    cl.set(t);
                    found = true;
                }
                break;
            }
            case K_QUAD:
            case K_TRI:
                if (planar_t(S.planars[idx], kind == K_TRI, r, tmin, cl.c, t)) {
                    cl.set(t);
                    found = true;
                }
                break;
            case K_XFORM: {
                const DXform& X = S.xforms[idx];
                stk.push(sp++, make_ref(K_POPXF, 0), NO_CULL);
                xfs.set(nxf++, idx);
                r = xf_ray(X, r);
                rf = make_rayf(r);
                a = len2(r.d);
                inva = 1.0 / a;
                cur = X.child;
                break;
            }
            case K_POPXF: {
                --nxf;
                r = r0;
                for (uint32_t k = 0; k < nxf; ++k) r = xf_ray(S.xforms[xfs.get(k)], r);
                rf = make_rayf(r);
                a = len2(r.d);
                inva = 1.0 / a;
                break;
            }
            default: break;
        }
        if (after != REF_NONE) cur = after;
    }
    tbest = cl.c;
    return found;
}

// ConstantMedium::hit (volume.rs:37-73) of medium idx for ray r in the
// medium's frame, interval [tmin, tmax]: the two boundary hits are one
// boundary walk run twice (one copy of the walk in the code).
// The two boundary hits of a boundary made of one sphere or of planar_n
// consecutive quads / triangles (rt_scene.cpp planar_boundary) in one pass.  A
// planar test's t and inside decision do not depend on the interval (quad.rs:
// 71-102: the interval only accepts or rejects the t already computed), so
// each element is tested once over (-inf, inf) and its t kept; the first hit
// is the least t (Hittables::hit, hits.rs:34-46), the second the least t >=
// t1 + 0.0001 -- the values and decisions of the two walks of volume.rs:44-48,
// without the list walk and with one planar test per element instead of two.
__device__ __forceinline__ bool boundary_onepass(const SceneView& S, const DMedium& M, const Ray& r0, double& t1,
                                                double& t2) {
    const double NINF = -__builtin_huge_val(), PINF = __builtin_huge_val();
    Ray r = r0;  // into the frame of the Transforms around the elements, as the walk does
    for (uint32_t j = 0; j < M.bxf_n; ++j) r = xf_ray(S.xforms[j == 0 ? M.bxf[0] : M.bxf[1]], r);
    if (M.bsphere) {
        // sphere.rs:77-92 over (-inf, inf), then over [t1 + 0.0001, inf):
        // the same roots, chosen by each interval as sphere_t_inv chooses
        const double4 s4 = S.spheres[M.bsphere - 1];
        const double a = len2(r.d), inva = 1.0 / a;
        const D3 oc = d3(s4.x, s4.y, s4.z) - r.o;
        const double h = dot(r.d, oc);
        const double cc = len2(oc) - s4.w * s4.w;
        const double disc = h * h - a * cc;
        if (disc < 0.0) return false;
        const double sq = k_sqrt(disc);
        const double rn = div_a(h - sq, a, inva), rf = div_a(h + sq, a, inva);
        auto pick = [&](double lo, double& t) {
            if (rn >= lo && rn <= PINF) t = rn;
            else if (rf >= lo && rf <= PINF) t = rf;
            else return false;
            return true;
        };
        if (!pick(NINF, t1)) return false;
        return pick(fmin(t1 + 0.0001, PINF), t2);
    }
    double tv[RT_MED_PLANAR_MAX];
    bool any = false;
    t1 = PINF;
#pragma unroll
    for (uint32_t k = 0; k < RT_MED_PLANAR_MAX; ++k) {
        tv[k] = __builtin_nan("");
        double tt;
        if (k < M.planar_n && planar_t(S.planars[M.planar_first + k], (M.tri_mask >> k) & 1u, r, NINF, PINF, tt)) {
            tv[k] = tt;
            t1 = any ? fmin(t1, tt) : tt;
            any = true;
        }
    }
    if (!any) return false;
    const double lo = fmin(t1 + 0.0001, PINF);
    any = false;
    t2 = PINF;
#pragma unroll
    for (uint32_t k = 0; k < RT_MED_PLANAR_MAX; ++k) {
        if (tv[k] >= lo && tv[k] <= PINF) {  // NaN (no hit) fails both
            t2 = any ? fmin(t2, tv[k]) : tv[k];
            any = true;
        }
    }
    return any;
}

template <bool BVH, class Stack>
__device__ __forceinline__ bool medium_hit(const SceneView& S, uint32_t idx, const Ray& r, double tmin, double tmax,
                                           Stack& stk, uint32_t sp0, const Rng& rng, double& t) {
    const DMedium M = S.media[idx];
    const double NINF = -__builtin_huge_val(), PINF = __builtin_huge_val();
    double t1 = 0.0, t2 = 0.0, lo = NINF;
    if (M.planar_n || M.bsphere) {
        if (!boundary_onepass(S, M, r, t1, t2)) return false;
    } else {
#pragma nounroll
        for (int pass = 0; pass < 2; ++pass) {
            double tb;
            if (!boundary_t<BVH>(S, M.boundary, r, lo, PINF, stk, sp0, tb)) return false;
            if (pass == 0) {
                t1 = tb;
                lo = fmin(t1 + 0.0001, PINF);
            } else {
                t2 = tb;
            }
        }
    }
    if (t1 < tmin) t1 = tmin;
    if (t2 > tmax) t2 = tmax;
    if (t1 >= t2) return false;
    if (t1 < 0.0) t1 = 0.0;
    const double ray_length = len(r.d);
    const double inside = (t2 - t1) * ray_length;
    const double hd = M.neg_inv_density * k_log(rng.medium(M.medium_id));
    if (hd > inside) return false;
    t = t1 + hd / ray_length;  // volume.rs:65
    return t <= tmax;
}

// world.hit(r, [1e-8, inf)) (camera.rs:286) as a depth-first walk with one
// running closest t.  Lists are walked in order with the interval shrunk to
// the best hit so far (hits.rs:34-46 tests every child with the full interval
// and keeps the first minimum: the same closest hit up to exact t ties).
//
// The walk is resumable: Trav holds its whole state, trace_step advances it by
// one stack entry, so a lane whose walk ends can be shaded and handed its next
// ray while the other lanes of its wave keep walking (rt_path_kernel).
template <int TIER>
struct Trav {
    Ray r;  // the ray in the frame of the innermost Transform entered (FULL only)
    RayF rf;
    double a, inva;  // |d|^2 and its correctly rounded reciprocal
    Closest cl;
    uint32_t cur, sp, nxf;
    XfIds xfs;
    bool found;
    HitInfo hit;
    uint32_t nmed;  // FULL: media met by the walk, tested after it (media_phase)
    uint32_t pn;    // BASIC (4-wide): the number of spheres queued for the exact test
    // BASIC: rf with each axis' two planes in the order the ray meets them
    // (rt_slab.h RaySF), and per axis the byte offset from a node's lo row to
    // its near row in the LDS copy -- 0, or 48 (the hi row) where 1/d <= 0.
    // Members of every tier's Trav like pn and nmed: only the basic tier
    // sets or reads them, and the other tiers' code is what it was without
    // them.  RaySF needs the folded widening (the ray's own scaling is what
    // orders the planes), so the kernel builds with RT_SLAB_FOLD = 1 only;
    // RT_SLAB_FOLD = 0 remains a setting of the header's CPU property test.
    static_assert(RT_SLAB_FOLD == 1, "the basic tier's sign-ordered slab test (RaySF) needs RT_SLAB_FOLD = 1");
    RaySF sf;
    uint32_t so[3];
};
// The basic tier's sign-ordered ray fields (T.rf is read by the check build's
// guard only: visit4_rows)
__device__ __forceinline__ void trace_sorted_fields(const Ray& wr, Trav<TIER_BASIC>& T) {
    const double o[3] = {wr.o.x, wr.o.y, wr.o.z}, d[3] = {wr.d.x, wr.d.y, wr.d.z};
    T.sf = make_raysf(o, d);
#pragma unroll
    for (int k = 0; k < 3; ++k) T.so[k] = T.sf.pos[k] ? 0u : 3u * (uint32_t)sizeof(float4);
}

template <int TIER>
__device__ __forceinline__ void trace_begin(const SceneView& S, const Ray& wr, Trav<TIER>& T) {
    T.r = wr;
    T.rf = make_rayf(wr);
    T.a = len2(wr.d);
    T.inva = 1.0 / T.a;
    T.cl.c = __builtin_huge_val();
    T.cl.c_f = __builtin_huge_valf();
    T.cur = S.world_root;
    T.sp = 0;
    T.nxf = 0;
    T.found = false;
    T.hit.nxf = 0;
    T.nmed = 0;
    if constexpr (TIER == TIER_BASIC) {
        T.pn = 0;
        T.cur = bword(S, S.world_root);  // the 4-wide walk's cur is a walk word
        trace_sorted_fields(wr, T);
    }
}

// Mesh tier with shading batches: the same 8 words; the f32
// ray, |d|^2 and its reciprocal are made again from the world ray on resume.
template <class Park>
__device__ __forceinline__ void trace_park(const Trav<TIER_MESH>& T, Park pk) {
    constexpr uint32_t B = RT_BLOCK;
    const uint64_t c = (uint64_t)__double_as_longlong(T.cl.c), ht = (uint64_t)__double_as_longlong(T.hit.t);
    pk[0 * B] = T.cur;
    pk[1 * B] = T.sp | ((uint32_t)T.found << 16);
    pk[2 * B] = (uint32_t)c;
    pk[3 * B] = (uint32_t)(c >> 32);
    pk[4 * B] = __float_as_uint(T.cl.c_f);
    pk[5 * B] = (uint32_t)ht;
    pk[6 * B] = (uint32_t)(ht >> 32);
    pk[7 * B] = T.hit.ref;
}
template <class Park>
__device__ __forceinline__ void trace_unpark(const Ray& wr, Trav<TIER_MESH>& T, Park pk) {
    constexpr uint32_t B = RT_BLOCK;
    T.cur = pk[0 * B];
    const uint32_t w = pk[1 * B];
    T.sp = w & 0xffffu;
    T.found = (w >> 16) & 1u;
    T.cl.c = __hiloint2double((int)pk[3 * B], (int)pk[2 * B]);
    T.cl.c_f = __uint_as_float(pk[4 * B]);
    T.hit.t = __hiloint2double((int)pk[6 * B], (int)pk[5 * B]);
    T.hit.ref = pk[7 * B];
    T.rf = make_rayf(wr);
    T.a = len2(wr.d);
    T.inva = 1.0 / T.a;
}
// Basic tier with shading batches: a carried-over walk's state is parked in
// LDS across the shading round as four 8-byte rows -- {cur, sp | pn | found},
// c, {c_f, hit ref}, hit t: two ds_write2st64_b64 / ds_read2st64_b64 a park
// and a resume, not four of the 4-byte kind (C2 -0.2 %, A/B at 128 spp, 5
// reps, RMSE 0: profiles/r05/ab_park64_c2_128spp.json).  The ray-derived
// fields are made again on resume (trace_ray_fields), as for a new walk.
__device__ __forceinline__ void trace_park2(const Trav<TIER_BASIC>& T, RT_LDS uint2* pk) {
    constexpr uint32_t B = RT_BLOCK_BASIC;
    const uint64_t c = (uint64_t)__double_as_longlong(T.cl.c), ht = (uint64_t)__double_as_longlong(T.hit.t);
    pk[0 * B] = make_uint2(T.cur, T.sp | (T.pn << 8) | ((uint32_t)T.found << 16));
    pk[1 * B] = make_uint2((uint32_t)c, (uint32_t)(c >> 32));
    pk[2 * B] = make_uint2(__float_as_uint(T.cl.c_f), T.hit.ref);
    pk[3 * B] = make_uint2((uint32_t)ht, (uint32_t)(ht >> 32));
}
__device__ __forceinline__ void trace_unpark_state2(Trav<TIER_BASIC>& T, const RT_LDS uint2* pk) {
    constexpr uint32_t B = RT_BLOCK_BASIC;
    const uint2 w0 = pk[0 * B], w1 = pk[1 * B], w2 = pk[2 * B], w3 = pk[3 * B];
    T.cur = w0.x;
    T.sp = w0.y & 0xffu;
    T.pn = (w0.y >> 8) & 0xffu;
    T.found = (w0.y >> 16) & 1u;
    T.cl.c = __hiloint2double((int)w1.y, (int)w1.x);
    T.cl.c_f = __uint_as_float(w2.x);
    T.hit.ref = w2.y;
    T.hit.t = __hiloint2double((int)w3.y, (int)w3.x);
}
__device__ __forceinline__ void trace_ray_fields(const Ray& wr, Trav<TIER_BASIC>& T) {
    T.rf = make_rayf(wr);
    trace_sorted_fields(wr, T);
    T.a = len2(wr.d);
    T.inva = 1.0 / T.a;
}
// The world-frame ray as the walk reads it: a register copy, or (full-flat
// tier) the lane's LDS copy, read only where a walk step
// needs it (leaving a Transform, the media phase) so that it holds no
// registers across the walk.
struct RayReg {
    const Ray& r;
    __device__ __forceinline__ Ray get() const { return r; }
};
struct RayLds {
    const RT_LDS double* p;  // 7 doubles, RT_BLOCK apart: o, d, time
    __device__ __forceinline__ Ray get() const {
        Ray r;
        r.o = d3(p[0 * RT_BLOCK], p[1 * RT_BLOCK], p[2 * RT_BLOCK]);
        r.d = d3(p[3 * RT_BLOCK], p[4 * RT_BLOCK], p[5 * RT_BLOCK]);
        r.time = p[6 * RT_BLOCK];
        return r;
    }
};
__device__ __forceinline__ RayReg world_ray(const Ray& r) { return RayReg{r}; }
__device__ __forceinline__ const RayLds& world_ray(const RayLds& r) { return r; }

// A lane's media queue (full tiers) in the lane rows of the LDS arena:
// entry k = {medium, nxf, xf a, xf b} in rows 2k and 2k + 1 (uint2, RT_BLOCK
// apart), so that it shares the one per-lane base address of the stack and
// the parked path state (rt_path_kernel's lane arena)
struct MedQ {
    RT_LDS uint2* p;
    __device__ __forceinline__ void set(uint32_t k, uint4 v) const {
        p[(2 * k) * RT_BLOCK] = make_uint2(v.x, v.y);
        p[(2 * k + 1) * RT_BLOCK] = make_uint2(v.z, v.w);
    }
    __device__ __forceinline__ uint4 get(uint32_t k) const {
        const uint2 a = p[(2 * k) * RT_BLOCK], b = p[(2 * k + 1) * RT_BLOCK];
        return make_uint4(a.x, a.y, b.x, b.y);
    }
};

// One stack entry of the walk; false when the walk is over (T.found, T.hit hold the result).
template <int TIER, class WR>
__device__ __forceinline__ bool trace_step(const SceneView& S, const WR& wrr, Trav<TIER>& T, StackFor<TIER>& stk,
                                           const Rng& rng, MedQ med, Diag& dg) {
    static_assert(TIER != TIER_BASIC, "the basic tier walks with trace4_step");
    const auto wq = world_ray(wrr);
    constexpr bool FULL = tier_full(TIER);
    constexpr double tmin = 1e-8;
    const float tmin_f = f32_down(tmin);
    if (T.cur == REF_NONE) {
        T.cur = pop(stk, T.sp, 0, T.cl.c_f);
        if (T.cur == REF_NONE) return false;
    }
    const Ray& r = FULL ? T.r : wq.get();
    uint32_t cur = T.cur;
    T.cur = REF_NONE;
    auto record = [&](uint32_t ref, double tt) {
        T.found = true;
        T.hit.t = tt;
        T.hit.ref = ref;
        if constexpr (FULL) {
            T.hit.nxf = T.nxf;
            T.hit.xf = T.xfs;
        }
    };
    // A list step whose element is a primitive tests it right here and goes
    // on with the next element (no stack round trip, one step per element);
    // a compound element (BVH, Transform, medium, list) is walked next with
    // the rest of the list pushed.
    uint32_t after = REF_NONE;
    if (ref_kind(cur) == K_LIST) {
        const uint32_t li = ref_idx(S, cur);
        const uint32_t child = S.list_children[li];
        if (child == REF_NONE) return true;  // empty list
        if constexpr (flat_runs<TIER>()) {
            // the flat tier tests a run of planar elements (the Cornell walls,
            // a box's six faces) in one step, in list order, each against the
            // closest t so far -- what the run's single steps do
            const uint32_t ck0 = ref_kind(child);
            if (ck0 == K_QUAD || ck0 == K_TRI) {
                const uint32_t run = S.list_boxes[li].run, n = run & 0xffu, first = ref_idx(S, child);
                check_run(S, first, n);
                RT_DIAG_ONLY(dg.sphere_tests += n;)
                for (uint32_t k = 0; k < n; ++k) {
                    const bool tri = (run >> (8u + k)) & 1u;
                    double tt;
                    if (planar_t(S.planars[first + k], tri, r, tmin, T.cl.c, tt)) {
                        T.cl.set(tt);
                        record(make_ref(tri ? K_TRI : K_QUAD, first + k), tt);
                    }
                }
                T.cur = S.list_children[li + n] != REF_NONE ? make_ref(K_LIST, li + n) : REF_NONE;
                return true;
            }
        }
        const uint32_t nxt = S.list_children[li + 1] != REF_NONE ? make_ref(K_LIST, li + 1) : REF_NONE;
        if constexpr (flat_boxes<TIER>()) {
            const uint32_t ck = ref_kind(child);
            if (ck != K_SPHERE && ck != K_QUAD && ck != K_TRI && ck != K_MSPHERE) {
                const bool in_box = list_box_hit(S, li, make_rayf(r), tmin_f, T.cl.c_f);
                // a ConstantMedium element whose box the ray meets is queued
                // for the media phase right here (K_MEDIUM below), without a
                // step of its own and the pop of the rest of the list
                const bool queue = in_box && ck == K_MEDIUM && T.nmed < RT_MEDIA_CAP;
                if (queue) {
                    med.set(T.nmed, make_uint4(ref_idx(S, child), T.nxf, T.xfs.a, T.xfs.b));
                    ++T.nmed;
                }
                if (!in_box || queue) {
                    T.cur = nxt;
                    return true;
                }
            }
        }
        const uint32_t ck = ref_kind(child);
        if (ck == K_SPHERE || ck == K_QUAD || ck == K_TRI || (FULL && ck == K_MSPHERE)) {
            cur = child;
            after = nxt;
        } else {
            if (nxt != REF_NONE) stk.push(T.sp++, nxt, NO_CULL);
            T.cur = child;
            return true;
        }
    }
    const uint32_t kind = ref_kind(cur), idx = ref_idx(S, cur);
    const uint32_t this_ref = cur;
    double t;
    bool got = false;
    RT_DIAG_ONLY(if (kind == K_BVH) ++dg.node_visits; if (kind == K_SPHERE || kind == K_TRI || kind == K_QUAD) ++dg.sphere_tests;)
    if (unified_load<TIER>() && (kind == K_BVH || kind == K_SPHERE || kind == K_TRI || kind == K_QUAD)) {
        // One load for the step's record, whatever it is: a node's 7 rows, a
        // quad's / triangle's 128 B, a sphere's 32 B, read as 8 dwordx4 from
        // the record's address (the world blob is padded past every array).
        // In a wave whose lanes hold nodes and primitives both, the node
        // visit and the primitive test then wait on one memory latency, not
        // one after the other.
        const bool planar = kind == K_TRI || kind == K_QUAD;
        // (the array addresses as values, selected: a select between the
        // SceneView's members made the compiler index a scratch copy of it)
        const uint64_t a_node = (uint64_t)S.nodes4, a_planar = (uint64_t)S.planars, a_sphere = (uint64_t)S.spheres;
        uint64_t addr = a_node;
        uint32_t stride = 0u;
        if (kind == K_BVH) stride = (uint32_t)sizeof(DNode4);
        if (planar) addr = a_planar, stride = (uint32_t)sizeof(DPlanar);
        if (kind == K_SPHERE) addr = a_sphere, stride = (uint32_t)sizeof(double4);
        const RT_GLOBAL float4* q = reinterpret_cast<const RT_GLOBAL float4*>(addr + (uint64_t)idx * stride);
#ifdef RT_DIAG
        {  // how often a wave's lanes read one record (the scalar-load case)
            const uint64_t ra = addr + (uint64_t)idx * stride;
            const uint32_t lo = (uint32_t)ra, hi = (uint32_t)(ra >> 32);
            const bool same = lo == __builtin_amdgcn_readfirstlane(lo) && hi == __builtin_amdgcn_readfirstlane(hi);
            const unsigned long long act = __ballot(true), sm = __ballot(same);
            if (__lane_id() == (uint32_t)(__ffsll((long long)act) - 1)) {
                ++dg.u_steps;
                dg.u_active += (unsigned long long)__popcll(act);
                dg.u_same += (unsigned long long)__popcll(sm);
                if (sm == act) {
                    ++dg.u_uniform;
                    if (kind == K_BVH) ++dg.u_uniform_node;
                }
            }
            constexpr uint32_t TOPK[4] = {5u, 21u, 85u, 341u};
            if (kind == K_BVH) ++dg.l_node;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool top = kind == K_BVH && idx < TOPK[k];
                if (top) ++dg.l_top[k];
                if (__ballot(top) == act && __lane_id() == (uint32_t)(__ffsll((long long)act) - 1)) ++dg.u_top[k];
            }
        }
#endif
        // rows 0-3 hold a sphere (2) and half a planar record; the rest
        // only for the lanes whose record has them
        const float4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
        float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f), q5 = q4, q6 = q4, q7 = q4;
        if (planar || kind == K_BVH) q4 = q[4], q5 = q[5], q6 = q[6];
        if (planar) q7 = q[7];
        if (kind == K_BVH) {
            T.cur = visit4_boxes_rows(q0, q1, q2, q3, q4, q5, q6, T.rf, tmin_f, T.cl.c_f, stk, T.sp);
        } else if (kind == K_SPHERE) {
            got = sphere_t_inv(d3(f4_lo(q0), f4_hi(q0), f4_lo(q1)), f4_hi(q1), r, T.a, T.inva, tmin, T.cl.c, t);
        } else if (planar) {
            got = planar_t_v(d3(f4_lo(q0), f4_hi(q0), f4_lo(q1)), f4_hi(q1), d3(f4_lo(q2), f4_hi(q2), f4_lo(q3)),
                             d3(f4_hi(q3), f4_lo(q4), f4_hi(q4)), d3(f4_lo(q5), f4_hi(q5), f4_lo(q6)),
                             d3(f4_hi(q6), f4_lo(q7), f4_hi(q7)), kind == K_TRI, r, tmin, T.cl.c, t);
        }
        if (got) {
            T.cl.set(t);
            record(this_ref, t);
        }
        if (after != REF_NONE) T.cur = after;
        return true;
    }
    // (the flat tier's primitives -- it holds no BVH node -- and the full
    // tiers' other kinds: nodes, spheres and planars of the BVH tiers took the
    // unified load above)
    if (kind == K_SPHERE) {
        const double4 sp4 = S.spheres[idx];
        got = sphere_t_inv(d3(sp4.x, sp4.y, sp4.z), sp4.w, r, T.a, T.inva, tmin, T.cl.c, t);
    } else if constexpr (FULL) {
        switch (kind) {
            case K_MSPHERE: {
                const double4 s4 = S.msph_center[idx], m = S.msph_dir[idx];
                const D3 cc = d3(s4.x, s4.y, s4.z) + r.time * d3(m.x, m.y, m.z);
                got = sphere_t_inv(cc, s4.w, r, T.a, T.inva, tmin, T.cl.c, t);
                break;
            }
            case K_QUAD:
            case K_TRI: got = planar_t(S.planars[idx], kind == K_TRI, r, tmin, T.cl.c, t); break;
            case K_XFORM: {
                const DXform& X = S.xforms[idx];
                stk.push(T.sp++, make_ref(K_POPXF, 0), NO_CULL);
                T.xfs.set(T.nxf++, idx);
                T.r = xf_ray(X, T.r);
                T.rf = make_rayf(T.r);
                T.a = len2(T.r.d);
                T.inva = 1.0 / T.a;
                T.cur = X.child;
                break;
            }
            case K_POPXF: {
                --T.nxf;
                T.r = wq.get();
                for (uint32_t k = 0; k < T.nxf; ++k) T.r = xf_ray(S.xforms[T.xfs.get(k)], T.r);
                T.rf = make_rayf(T.r);
                T.a = len2(T.r.d);
                T.inva = 1.0 / T.a;
                break;
            }
            case K_MEDIUM: {
                // volume.rs:37-73.  The medium's hit is independent of the
                // other objects but for the interval's upper end, so it is
                // queued (with the Transforms around it) and tested after the
                // walk against the walk's closest t (media_phase); only a
                // lane whose queue is full tests it here.
                if (T.nmed < RT_MEDIA_CAP) {
                    med.set(T.nmed, make_uint4(idx, T.nxf, T.xfs.a, T.xfs.b));
                    ++T.nmed;
                } else {
                    got = medium_hit<TIER != TIER_FULL_FLAT>(S, idx, r, tmin, T.cl.c, stk, T.sp, rng, t);
                }
                break;
            }
            default: break;
        }
    }
    if (got) {
        T.cl.set(t);
        record(this_ref, t);
    }
    if (after != REF_NONE) T.cur = after;
    return true;
}

// The queued media of a finished walk (FULL tier), each in its own frame,
// against the walk's closest t; the walk's stack is free again.
template <int TIER, class WR>
__device__ __forceinline__ void media_phase(const SceneView& S, const WR& wrr, Trav<TIER>& T, StackFor<TIER>& stk,
                                            const Rng& rng, MedQ med) {
    const auto wq = world_ray(wrr);
    for (uint32_t k = 0; k < T.nmed; ++k) {
        const uint4 e = med.get(k);
        Ray r = wq.get();
        for (uint32_t j = 0; j < e.y; ++j) r = xf_ray(S.xforms[j == 0 ? e.z : e.w], r);
        double t;
        if (medium_hit<TIER != TIER_FULL_FLAT>(S, e.x, r, 1e-8, T.cl.c, stk, 0, rng, t)) {
            T.cl.set(t);
            T.found = true;
            T.hit.t = t;
            T.hit.ref = make_ref(K_MEDIUM, e.x);
            T.hit.nxf = e.y;
            T.hit.xf.a = e.z;
            T.hit.xf.b = e.w;
        }
    }
    T.nmed = 0;
}

constexpr uint32_t RT_PARK_WORDS = 8;
// The LDS set-up every kernel over the walk makes before its first ray
// (rt_path_kernel, rt_hit_kernel).  The lane arena (all tiers but the basic
// one) is one uint2 row per lane and row, RT_BLOCK apart: the stack's rows
// first, then (full tiers) the media queue's -- lane_rows_med is where those
// start; make_stack (rt_stack.h) binds a lane's stack to its rows and to its
// column of the global overflow buffer.
template <int TIER>
constexpr uint32_t lane_rows_med() {
    return TIER == TIER_BASIC ? 0u : lds_stack_entries(TIER);
}
// A lane's views of the block's walk arrays: its arena row, the media queue in
// it, its sphere queue and its stack.  The arrays themselves are each
// kernel's own (their sizes depend on what else the kernel parks in LDS).
template <int TIER>
struct WalkLds {
    RT_LDS uint2* lrow;
    MedQ med;
    RT_LDS uint16_t* pq;
    StackFor<TIER> stk;
};
template <int TIER>
__device__ __forceinline__ WalkLds<TIER> walk_lds(uint2* lane_lds, uint32_t* stack4_lds, uint16_t* pend_lds,
                                                  RT_GLOBAL uint2* stack_ovf) {
    constexpr uint32_t BLK = TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    RT_LDS uint2* const lrow = (RT_LDS uint2*)(lane_lds + threadIdx.x);
    return WalkLds<TIER>{lrow, MedQ{lrow + lane_rows_med<TIER>() * BLK}, (RT_LDS uint16_t*)(pend_lds + threadIdx.x),
                         make_stack<TIER>(lrow, (RT_LDS uint32_t*)(stack4_lds + threadIdx.x),
                                          stack_ovf + (uint64_t)blockIdx.x * BLK + threadIdx.x, gridDim.x * BLK)};
}

}  // namespace rtk

// boundary_t and trace_step call visit4_boxes and visit4_boxes_rows, templates
// over the stack type that are looked up where the walk is instantiated
#include "rt_walk4.h"
