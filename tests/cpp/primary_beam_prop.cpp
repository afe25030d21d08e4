// TEST HARNESS: property test of the basic tier's primary-ray beam test
// (raytracer-2025_amd/csrc/rt_primary.h, the source the gfx950 kernels compile).
// For a camera, a footprint of pixels and a sphere, beam_may_hit's verdict
// "cannot hit" must hold for every ray Camera::get_ray can make for that
// footprint: the exact f64 Sphere::hit (sphere_exact.cpp, sphere.rs:77-108)
// returns no root in [1e-8, inf) for any of them.  No violation is allowed: a
// sphere left out of a pixel's candidates that a primary ray would have hit
// changes the image.
// Cases: cameras as Camera::initilize makes them (random and far outside the
// world, offset by 4096, fov 1 to 120 degrees, lens radius 0 and up to the
// sphere spacing, focus distances 0.1 to 100), pixels of the frame's corners,
// edges and interior, footprints of one pixel and of the table kernel's tiles
// (row strides 1 to 3); spheres placed on a ray of the set at a grazing
// distance (a relative 0, 1e-12 ... 1 inside or outside the surface),
// around the camera (containing it, touching the lens), behind it, the
// book-1 ground (r = 1000), r = 0, r = 1e-3, and anywhere.  A sphere the
// verdict excludes is tried with rays through the lens' centre and eight rim
// points and the footprint's centre, corners and edge midpoints (81 rays),
// and 24 random ones, half of them from the rim.
// Prints "verdicts excluded rays hits_of_admitted violations"; exits 1 on a violation.
// primary_beam_prop [n [seed]]        the property
// primary_beam_prop table             the table's sizing and indexing under row shards
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../raytracer-2025_amd/csrc/rt_primary.h"

extern "C" double exact_sphere_t(const double c[3], double r, const double o[3], const double d[3], double tmin,
                                 double tmax);

struct V {
    double x, y, z;
};
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(double s, V a) { return {s * a.x, s * a.y, s * a.z}; }
static double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double len(V a) { return std::sqrt(dot(a, a)); }
static V unit(V a) { return (1.0 / len(a)) * a; }
static void put(double* d, V a) { d[0] = a.x, d[1] = a.y, d[2] = a.z; }
static V get(const double* d) { return {d[0], d[1], d[2]}; }

// Camera::initilize (camera.rs:204-245) as rt_render.cpp init_frame computes it
static rtk::BeamCam make_cam(V from, V at, V up, double vfov_deg, double focus, double lens_radius, uint32_t W,
                             uint32_t H) {
    const double h = std::tan(vfov_deg * (M_PI / 180.0) / 2.0);
    const double vh = 2.0 * h * focus, vw = vh * ((double)W / (double)H);
    const V w = unit(from - at), u = unit(cross(up, w)), v = cross(w, u);
    const V vu = vw * u, vv = vh * (-1.0 * v);
    const V du = (1.0 / W) * vu, dv = (1.0 / H) * vv;
    const V ul = ((from - focus * w) - 0.5 * vu) - 0.5 * vv;
    rtk::BeamCam C;
    put(C.center, from);
    put(C.pixel00, ul + 0.5 * (du + dv));
    put(C.du, du);
    put(C.dv, dv);
    put(C.disk_u, lens_radius * u);
    put(C.disk_v, lens_radius * v);
    C.defocus = lens_radius > 0.0 ? 1u : 0u;
    return C;
}

// the kernel's camera_ray: lens point (a, b) of the unit disk, target (x, y) in pixel units
static void camera_ray(const rtk::BeamCam& C, double a, double b, double x, double y, double o[3], double d[3]) {
    for (int k = 0; k < 3; ++k) {
        o[k] = C.defocus ? (C.center[k] + (a * C.disk_u[k])) + (b * C.disk_v[k]) : C.center[k];
        const double ps = (C.pixel00[k] + (x * C.du[k])) + (y * C.dv[k]);
        d[k] = ps - o[k];
    }
}

static int table_mode() {
    int bad = 0;
    auto expect = [&](bool ok, const char* what) {
        if (!ok) {
            std::printf("FAIL %s\n", what);
            ++bad;
        }
    };
    expect(rtk::PRIMARY_CAP == 8 && rtk::PRIMARY_NONE < rtk::PRIMARY_WALK && rtk::PRIMARY_MAX_SPHERES <= rtk::PRIMARY_NONE,
           "marks lie above every sphere index");
    const uint32_t Ws[4] = {1, 7, 48, 1920}, Hs[5] = {1, 5, 36, 47, 1080};
    for (uint32_t W : Ws)
        for (uint32_t H : Hs)
            for (uint32_t stride = 1; stride <= 3; ++stride) {
                uint64_t total_rows = 0;
                for (uint32_t off = 0; off < stride; ++off) {
                    // rt_render.cpp init_frame: the shard's rows
                    const uint32_t rows = off >= H ? 0 : (H - off + stride - 1) / stride;
                    total_rows += rows;
                    expect(rtk::primary_table_slots(W, rows) == (uint64_t)W * rows * 8u, "slots");
                    expect(rtk::primary_table_bytes(W, rows) == (uint64_t)W * rows * 16u, "bytes");
                    // every pixel of the shard has its own in-range, 8-aligned run of slots, in launch-pixel order
                    std::vector<uint8_t> seen((size_t)W * rows, 0);
                    for (uint32_t prow = 0; prow < rows; ++prow) {
                        const uint32_t py = rtk::primary_image_row(prow, off, stride);
                        expect(py < H && py % stride == off % stride, "image row of the shard");
                        expect(rtk::primary_shard_row(py, off, stride) == prow, "shard row round trip");
                        // the kernel's division by the rounded-up reciprocal (rt_queue.h udiv_inv)
                        const double inv = std::nextafter(1.0 / (double)stride, 2.0);
                        expect((uint32_t)((double)(py - off) * inv) == prow, "udiv_inv shard row");
                        for (uint32_t px = 0; px < W; ++px) {
                            const uint64_t i = rtk::primary_table_index(W, px, py, off, stride);
                            expect(i % 8u == 0 && i + 8u <= rtk::primary_table_slots(W, rows), "index in range");
                            expect(i / 8u == (uint64_t)prow * W + px, "launch-pixel order");
                            if (i / 8u < seen.size()) ++seen[i / 8u];
                        }
                    }
                    for (uint8_t s : seen) expect(s == 1, "each run used once");
                    // the table kernel's grid of tiles covers the launch, and only its last tiles overhang
                    const uint32_t tx = rtk::primary_tiles(W), ty = rtk::primary_tiles(rows);
                    expect((uint64_t)tx * rtk::PRIMARY_TILE >= W && (tx == 0 || (uint64_t)(tx - 1) * rtk::PRIMARY_TILE < W), "tiles x");
                    expect((uint64_t)ty * rtk::PRIMARY_TILE >= rows && (ty == 0 || (uint64_t)(ty - 1) * rtk::PRIMARY_TILE < rows), "tiles y");
                }
                expect(total_rows == H, "the shards' rows partition the frame");
            }
    std::printf("table %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "table") == 0) return table_mode();
    const long n = argc > 1 ? std::atol(argv[1]) : 300000;
    std::mt19937_64 rng(argc > 2 ? std::atoll(argv[2]) : 2025);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    auto pick = [&](int k) { return (int)(U(rng) * k); };
    auto loguni = [&](double lo, double hi) { return std::exp(std::log(lo) + U(rng) * std::log(hi / lo)); };
    auto rand_unit = [&]() {
        const double z = 1 - 2 * U(rng), r = std::sqrt(std::fmax(0.0, 1 - z * z)), p = 2 * M_PI * U(rng);
        return V{r * std::cos(p), r * std::sin(p), z};
    };
    long verdicts = 0, excluded = 0, rays = 0, admitted_hits = 0, bad = 0;
    for (long i = 0; i < n; ++i) {
        // ---- the camera
        const int ck = pick(6);
        V from, at;
        double focus, lens, fov;
        uint32_t W = 64, H = 36;
        if (ck == 0) {  // book 1
            from = {13, 2, 3}, at = {0, 0, 0}, focus = 10.0, lens = 10.0 * std::tan(0.3 * M_PI / 180.0), fov = 20;
            W = 1920, H = 1080;
        } else {
            from = ck == 1 ? 1e4 * rand_unit() : ck == 2 ? V{4096 + 20 * U(rng), 5 * U(rng), 4096 + 20 * U(rng)}
                                                         : V{30 * (U(rng) - 0.5), 10 * U(rng), 30 * (U(rng) - 0.5)};
            at = from + loguni(0.1, 100) * rand_unit();
            if (ck == 1) at = 5.0 * rand_unit();  // far outside the world, looking at it
            focus = pick(2) ? len(from - at) : loguni(0.1, 100);
            const int lk = pick(4);
            lens = lk == 0 ? 0.0 : lk == 1 ? loguni(1e-3, 0.1) : lk == 2 ? loguni(0.1, 1.0) : focus * std::tan(5.0 * M_PI / 180.0);
            fov = pick(3) == 0 ? loguni(1, 20) : 20 + 100 * U(rng);
            const int sk = pick(3);
            W = sk == 0 ? 48 : sk == 1 ? 64 : 1920, H = sk == 0 ? 48 : sk == 1 ? 36 : 1080;
        }
        V up = {0, 1, 0};
        if (std::fabs(dot(unit(from - at), up)) > 0.99) up = {1, 0, 0};
        const rtk::BeamCam C = make_cam(from, at, up, fov, focus, lens, W, H);
        // ---- the footprint: a pixel, or a tile of the table kernel
        const bool tile = pick(4) == 0;
        auto edge = [&](uint32_t nn) { const int e = pick(4); return e == 0 ? 0u : e == 1 ? nn - 1 : (uint32_t)pick((int)nn); };
        double fx, fy, hx, hy;
        if (!tile) {
            fx = edge(W), fy = edge(H), hx = hy = 0.5;
        } else {
            const uint32_t stride = 1 + pick(3), off = pick((int)stride), rows = off >= H ? 0 : (H - off + stride - 1) / stride;
            const uint32_t x0 = 16 * (uint32_t)pick((int)rtk::primary_tiles(W)), x1 = std::min(x0 + 16, W);
            const uint32_t r0 = 16 * (uint32_t)pick((int)rtk::primary_tiles(rows ? rows : 1)), r1 = std::min(r0 + 16, rows ? rows : 1);
            const double ylo = off + (double)r0 * stride, yhi = off + (double)(r1 - 1) * stride;
            fx = 0.5 * ((double)x0 + (double)(x1 - 1)), hx = 0.5 * (x1 - x0);
            fy = 0.5 * (ylo + yhi), hy = 0.5 * (yhi - ylo) + 0.5;
        }
        const rtk::Beam B = rtk::make_beam(C, fx, fy, hx, hy);
        // the lens and footprint points the excluded spheres are tried with
        double lp[9][2] = {{0, 0}};
        for (int k = 0; k < 8; ++k) lp[k + 1][0] = std::cos(k * M_PI / 4), lp[k + 1][1] = std::sin(k * M_PI / 4);
        const double fp[9][2] = {{0, 0}, {-1, -1}, {1, -1}, {-1, 1}, {1, 1}, {-1, 0}, {1, 0}, {0, -1}, {0, 1}};
        for (int sN = 0; sN < 8; ++sN) {
            // ---- the sphere
            double c[3], r;
            const int kind = pick(10);
            // a ray of the set and a point on it
            const double th = 2 * M_PI * U(rng), rr = pick(3) == 0 ? 1.0 : std::sqrt(U(rng));
            const double qx = pick(3) == 0 ? (pick(2) ? 1.0 : -1.0) : 2 * U(rng) - 1, qy = pick(3) == 0 ? (pick(2) ? 1.0 : -1.0) : 2 * U(rng) - 1;
            double o[3], d[3];
            camera_ray(C, rr * std::cos(th), rr * std::sin(th), fx + qx * hx, fy + qy * hy, o, d);
            const double t = pick(4) == 0 ? loguni(1e-6, 1e-2) : loguni(1e-2, 50);
            const V P = get(o) + t * get(d);
            const V dir = unit(get(d));
            V nrm = cross(dir, rand_unit());
            nrm = unit(nrm);
            static const double graze[9] = {0.0, 1e-12, -1e-12, 1e-6, -1e-6, 1e-3, -1e-3, 0.1, 1.0};
            if (kind <= 3) {  // grazing a ray of the set
                r = kind == 0 ? 0.2 : kind == 1 ? 1.0 : kind == 2 ? loguni(1e-3, 50) : 1000.0;
                put(c, P + (r * (1.0 + graze[pick(9)])) * nrm);
            } else if (kind == 4) {  // just outside the beam: a few footprints / lens radii off the ray
                r = loguni(1e-2, 2);
                put(c, P + (r + loguni(1e-4, 10) * (len(get(C.du)) * hx + len(get(C.dv)) * hy + lens)) * nrm);
            } else if (kind == 5) {  // around the camera: containing it, touching the lens
                r = loguni(1e-3, 100);
                put(c, from + (r * (pick(2) ? U(rng) : 1.0 + graze[pick(9)]) + (pick(2) ? lens : 0.0)) * rand_unit());
            } else if (kind == 6) {  // behind the camera
                r = loguni(1e-2, 10);
                put(c, from + (-1.0 * (r * (1.0 + graze[pick(9)]) + loguni(1e-6, 10))) * dir + (U(rng) * r) * nrm);
            } else if (kind == 7) {  // the book-1 ground under the camera's world
                r = 1000.0;
                put(c, V{from.x * (ck == 1 ? 0 : 1), -1000.0 - (pick(2) ? 0.0 : loguni(1e-6, 10)), from.z * (ck == 1 ? 0 : 1)});
            } else if (kind == 8) {  // r = 0 and r = 1e-3, on a ray of the set
                r = pick(2) ? 0.0 : 1e-3;
                put(c, P + (r * graze[pick(9)]) * nrm);
            } else {  // anywhere
                r = loguni(1e-2, 20);
                put(c, from + loguni(0.1, 200) * rand_unit());
            }
            const double s4[4] = {c[0], c[1], c[2], r};
            const bool may = rtk::beam_may_hit(B, s4);
            ++verdicts;
            if (may) {
                if (r == 0.0) continue;
                admitted_hits += exact_sphere_t(c, r, o, d, 1e-8, INFINITY) >= 0;
                continue;
            }
            ++excluded;
            if (r == 0.0) {
                std::printf("VIOLATION r = 0 excluded\n");
                ++bad;
            }
            // every try: the fixed lens x footprint points, then random rays
            for (int k = 0; k < 81 + 24; ++k) {
                double a, b, x, y;
                if (k < 81) {
                    a = lp[k / 9][0], b = lp[k / 9][1], x = fp[k % 9][0], y = fp[k % 9][1];
                } else {
                    const double tt = 2 * M_PI * U(rng), r2 = pick(2) ? 1.0 : std::sqrt(U(rng));
                    a = r2 * std::cos(tt), b = r2 * std::sin(tt), x = 2 * U(rng) - 1, y = 2 * U(rng) - 1;
                }
                double o2[3], d2[3];
                camera_ray(C, a, b, fx + x * hx, fy + y * hy, o2, d2);
                ++rays;
                const double tx = exact_sphere_t(c, r, o2, d2, 1e-8, INFINITY);
                if (tx >= 0) {
                    if (bad < 10)
                        std::printf("VIOLATION cam %d kind %d tile %d: c=(%.17g %.17g %.17g) r=%.17g o=(%.17g %.17g %.17g) "
                                    "d=(%.17g %.17g %.17g) t=%.17g foot=(%.17g %.17g %.17g %.17g) lens=%.17g\n",
                                    ck, kind, (int)tile, c[0], c[1], c[2], r, o2[0], o2[1], o2[2], d2[0], d2[1], d2[2], tx, fx, fy,
                                    hx, hy, lens);
                    ++bad;
                    break;
                }
            }
        }
    }
    std::printf("%ld %ld %ld %ld %ld\n", verdicts, excluded, rays, admitted_hits, bad);
    return bad ? 1 : 0;
}
