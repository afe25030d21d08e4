// rt_kernel_common.hip -- what every build has once beside the path tiers
// and the hit queries: the output stage (reduce, to_rgb, deinterleave), the
// math and walk self-tests, the frame plan's entry points and the frame
// launcher, which calls the tiers through rt_path_entry.h.
#include <hip/hip_runtime.h>

#include "../../include/rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_slab.h"
#include "rt_sphere_filter.h"
#include "rt_primary.h"
#include "rt_plan.h"
#include "rt_queue.h"
#include "rt_frame.h"
#include "rt_path_entry.h"

namespace rtk {
// Color::to_rgb (utils/color.rs:14-36): optional ACES fit, clamp, then the sRGB
// OETF and f64 -> u8 (palette restated as in oracle/rt_oracle.cpp to_rgb).
// No contraction, so the arithmetic is the host's; pow is ocml's.  Held to
// the exact byte of the real-valued function on every f32 input that is not
// within a relative 2^-40 of a byte boundary (tests/test_to_rgb_gpu.py).
__device__ __forceinline__ uint8_t srgb_u8(double x, int toon) {
#pragma clang fp contract(off)
    if (toon == 1) {
        const double m = (x * (2.51 * x + 0.03)) / (x * (2.43 * x + 0.59) + 0.14);
        x = m < 0.0 ? 0.0 : (m > 1.0 ? 1.0 : m);
    }
    const double sv = x <= 0.0031308 ? 12.92 * x : 1.055 * pow(x, 1.0 / 2.4) - 0.055;
    const double q = round(sv * 255.0);
    return (uint8_t)(q < 0.0 ? 0.0 : (q > 255.0 ? 255.0 : q));
}

// Sums the S stratum rows of each pixel in s_i order -- a row = its one
// whole-row sum (pixels below whole_px), or its `parts` part sums added in
// part order (the tail rows); the slots in queue order (Frame) -- *
// pixel_sample_scale, to linear f32 (camera.rs:193), and -- when srgb is
// given -- the pixel's to_rgb bytes from the f64 sum, as the reference
// converts its f64 color.  One lane per (pixel, channel), 21 pixels a wave:
// a pixel's sums are contiguous in the slot order, so a wave's load reads 21
// runs of 24 B and its next loads the same lines (one lane per pixel read 64
// lines per load, three times: 1.8 ms for C2's 3.8 GB against 0.8 at HBM rate).
constexpr uint32_t REDUCE_PX_PER_WAVE = 21;
__global__ void __launch_bounds__(256) rt_reduce_kernel(const double* __restrict__ partial, uint32_t p_lo, uint32_t npix,
                                                       uint32_t S, uint32_t parts, uint32_t whole_px, uint32_t parts2,
                                                       uint32_t fine_px, double scale, float* __restrict__ out,
                                                       uint8_t* __restrict__ srgb, int toon) {
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;
    if (lane >= 3u * REDUCE_PX_PER_WAVE) return;
    const uint32_t p = p_lo + wave * REDUCE_PX_PER_WAVE + lane / 3u, c = lane % 3u;  // pixels [p_lo, npix)
    if (p >= npix) return;
    // pixels [0, whole_px): one sum per stratum row; [whole_px, fine_px):
    // `parts`; [fine_px, npix): `parts2` (the fine rows)
    const bool whole = p < whole_px, fine = p >= fine_px;
    const uint32_t np = whole ? 1u : (fine ? parts2 : parts);
    const uint64_t part_first = (uint64_t)whole_px * S + (uint64_t)(fine_px - whole_px) * S * parts;
    const uint64_t first = whole ? (uint64_t)p * S
                         : fine  ? part_first + (uint64_t)(p - fine_px) * S * parts2
                                 : (uint64_t)whole_px * S + (uint64_t)(p - whole_px) * S * parts;
    const double* src = partial + first * 3 + c;
    double acc = 0.0;
    for (uint32_t k = 0; k < S; ++k) {
        const double* row = src + (uint64_t)k * np * 3;
        double rr = row[0];
        for (uint32_t j = 1; j < np; ++j) rr += row[j * 3];
        acc += rr;
    }
    const double v = acc * scale;
    out[(uint64_t)p * 3 + c] = (float)v;
    if (srgb) srgb[(uint64_t)p * 3 + c] = srgb_u8(v, toon);
}

// The same sums, staged through LDS: one wave per group of
// `pw` consecutive pixels of one region (whole rows: np = 1; tail rows: np =
// parts; fine rows: np = parts2), whose part sums are contiguous in slot
// order.  The wave copies the group's doubles into LDS with whole-line loads
// (each lane 8 B, 64 lanes 512 B a step), adds each (pixel, s_i, channel)'s
// parts in part order into the slot of part 0, then each (pixel, channel)'s
// S row sums in s_i order -- rt_reduce_kernel's additions in its order, so
// the same bits -- where that kernel's lanes read 21 pixels' 24-B runs per
// load and re-read each line from the cache several times.
constexpr uint32_t REDUCE_LDS_DOUBLES = 2048;  // 16 KiB per wave
__global__ void __launch_bounds__(64) rt_reduce_lds_kernel(const double* __restrict__ partial, uint32_t p_begin,
                                                          uint32_t p_end, uint64_t slot0, uint32_t S, uint32_t np,
                                                          uint32_t pw, double scale, float* __restrict__ out,
                                                          uint8_t* __restrict__ srgb, int toon) {
    __shared__ double buf[REDUCE_LDS_DOUBLES];
    const uint32_t lane = threadIdx.x;
    const uint32_t p0 = p_begin + blockIdx.x * pw;
    if (p0 >= p_end) return;
    const uint32_t n = min(pw, p_end - p0);
    const uint32_t row = np * 3u;          // doubles per stratum row
    const uint32_t per_px = S * row;       // doubles per pixel
    const uint32_t total = n * per_px;     // <= REDUCE_LDS_DOUBLES (host)
    const double* src = partial + (slot0 + (uint64_t)(p0 - p_begin) * S * np) * 3u;
    // (8 loads in flight per lane before their LDS stores)
    uint32_t i0 = lane;
    for (; i0 + 7u * 64u < total; i0 += 8u * 64u) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = src[i0 + u * 64u];
#pragma unroll
        for (int u = 0; u < 8; ++u) buf[i0 + u * 64u] = v[u];
    }
    for (; i0 < total; i0 += 64u) buf[i0] = src[i0];
    __syncthreads();
    if (np > 1u) {
        // (pixel, s_i, channel): its parts in order, into part 0's slot
        for (uint32_t i = lane; i < n * S * 3u; i += 64u) {
            const uint32_t c = i % 3u, ps = i / 3u;  // ps = pixel * S + s_i
            double* r = buf + ps * row + c;
            double rr = r[0];
            for (uint32_t j = 1; j < np; ++j) rr += r[j * 3u];
            r[0] = rr;
        }
        __syncthreads();
    }
    for (uint32_t i = lane; i < n * 3u; i += 64u) {
        const uint32_t c = i % 3u, px = i / 3u;
        const double* r = buf + px * per_px + c;
        double acc = 0.0;
        for (uint32_t k = 0; k < S; ++k) acc += r[k * row];
        const double v = acc * scale;
        const uint64_t o = (uint64_t)(p0 + px) * 3u + c;
        out[o] = (float)v;
        if (srgb) srgb[o] = srgb_u8(v, toon);
    }
}

// Math self-test (rt_math_selftest): the kernel's f64 functions (impl 0,
// rt_crmath.h) or ROCm's device libm (impl 1, ocml) on n arguments.
__global__ void __launch_bounds__(256) rt_math_kernel(int fn, int impl, const double* __restrict__ a,
                                                     const double* __restrict__ b, double* __restrict__ out,
                                                     uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double x = a[i], y = b ? b[i] : 0.0;
    double r = 0.0, s = 0.0, c = 0.0;
    if (impl == 0) {
        switch (fn) {
            case 0: r = rtcr::sin(x); break;
            case 1: r = rtcr::cos(x); break;
            case 2: rtcr::sincos(x, &s, &c), r = s; break;
            case 3: rtcr::sincos(x, &s, &c), r = c; break;
            case 4: r = rtcr::log(x); break;
            case 5: r = rtcr::acos(x); break;
            case 6: r = rtcr::atan2(x, y); break;
            case 8: rtcr::sincos_2pi(x, &s, &c), r = s; break;
            case 9: rtcr::sincos_2pi(x, &s, &c), r = c; break;
            case 10: r = rtcr::pow_2m4(x); break;
            default: r = k_sqrt(x); break;  // the path's square root (RT_FAST_SQRT)
        }
    } else {
        switch (fn) {
            case 0: r = ::sin(x); break;
            case 1: r = ::cos(x); break;
            case 2: ::sincos(x, &s, &c), r = s; break;
            case 3: ::sincos(x, &s, &c), r = c; break;
            case 4: r = ::log(x); break;
            case 5: r = ::acos(x); break;
            case 6: r = ::atan2(x, y); break;
            case 8: ::sincos(2.0 * PI * x, &s, &c), r = s; break;
            case 9: ::sincos(2.0 * PI * x, &s, &c), r = c; break;
            case 10: r = ::pow(0.0625, x); break;
            default: r = ::sqrt(x); break;
        }
    }
    out[i] = r;
}

// Walk self-test (rt_walk_selftest): the f32 stages of the closest-hit walk --
// the very functions the path kernels call -- one case per thread, in_w
// doubles in and out_w out per case (rtk_walk_widths).  f32 quantities
// travel as doubles that hold an f32 exactly, so the casts below are exact.
__global__ void __launch_bounds__(256) rt_walk_kernel(int fn, int in_w, int out_w, const double* __restrict__ in,
                                                     double* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = in + i * (uint64_t)in_w;
    double* q = out + i * (uint64_t)out_w;
    switch (fn) {
        case 0: {  // o[3], d[3], lo[3], hi[3], tmin_f, c_f -> hit, entry
            const double o[3] = {p[0], p[1], p[2]}, d[3] = {p[3], p[4], p[5]};
            const float lo[3] = {(float)p[6], (float)p[7], (float)p[8]}, hi[3] = {(float)p[9], (float)p[10], (float)p[11]};
            const RayF R = make_rayf(o, d);
            float entry = 0.0f;
            const bool hit = slab_f(lo, hi, R, (float)p[12], (float)p[13], entry);
            q[0] = hit ? 1.0 : 0.0;
            q[1] = (double)entry;
            break;
        }
        case 1: {  // o[3], d[3], cx, cy, cz, r, g, c_f -> keep, c_f'
            const double o[3] = {p[0], p[1], p[2]}, d[3] = {p[3], p[4], p[5]};
            const SphF F = make_sphf(o, d);
            float c_f = (float)p[11];
            const bool keep = sphere_filter((float)p[6], (float)p[7], (float)p[8], (float)p[9], (float)p[10], F, c_f, true);
            q[0] = keep ? 1.0 : 0.0;
            q[1] = (double)c_f;
            break;
        }
        case 2: q[0] = (double)rcp_f32((float)p[0]); break;
        case 3: {
            float r;
            sqrt_f32((float)p[0], r);
            q[0] = (double)r;
            break;
        }
        case 4: {
            Closest cl;
            cl.set(p[0]);
            q[0] = (double)cl.c_f;
            break;
        }
        case 5: {
            Closest cl;
            cl.c = 0.0;
            cl.c_f = (float)p[1];
            cl.lower(p[0]);
            q[0] = (double)cl.c_f;
            break;
        }
        default: q[0] = (double)f32_down(p[0]); break;
    }
}

// The primary-ray candidate table of one launch (rt_primary.h): for every
// launch pixel the spheres a camera ray of that pixel may hit, by the
// conservative beam test.  One 256-thread block per tile of 16 x 16 launch
// pixels: the block first tests every sphere against the tile's beam (the
// footprint of all its pixels) into a bit set in LDS, then each thread tests
// the tile's spheres against its own pixel's beam, in index order, and stores
// the pixel's eight slots as one 16-byte word.  K.cand of the launch
// parameters is the table: rows * W uint4, which the grid's tiles cover --
// a thread whose pixel lies outside the launch's W x rows stores nothing.
__global__ void __launch_bounds__(PRIMARY_TILE * PRIMARY_TILE) rt_primary_kernel(const KParams* __restrict__ P) {
    const SceneView& S = P->S;
    const Frame& F = P->F;
    constexpr uint32_t BLK = PRIMARY_TILE * PRIMARY_TILE;
    __shared__ uint32_t bits[PRIMARY_MAX_SPHERES / 32u];
    const uint32_t n = min(S.n_ref[K_SPHERE], PRIMARY_MAX_SPHERES), words = (n + 31u) / 32u;
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < words; k += BLK) bits[k] = 0u;
    __syncthreads();
    BeamCam C;
    auto cp3 = [](double* dst, const D3& v) { dst[0] = v.x, dst[1] = v.y, dst[2] = v.z; };
    cp3(C.center, F.center), cp3(C.disk_u, F.disk_u), cp3(C.disk_v, F.disk_v);
    cp3(C.pixel00, F.pixel00), cp3(C.du, F.du), cp3(C.dv, F.dv);
    C.defocus = F.defocus;
    // the tile: launch pixels [x0, x1) x shard rows [r0, r1) (the grid has no empty tile)
    const uint32_t x0 = blockIdx.x * PRIMARY_TILE, r0 = blockIdx.y * PRIMARY_TILE;
    const uint32_t x1 = min(x0 + PRIMARY_TILE, F.W), r1 = min(r0 + PRIMARY_TILE, F.rows);
    const double y_lo = (double)primary_image_row(r0, F.row_offset, F.row_stride);
    const double y_hi = (double)primary_image_row(r1 - 1u, F.row_offset, F.row_stride);
    const Beam tile = make_beam(C, 0.5 * ((double)x0 + (double)(x1 - 1u)), 0.5 * (y_lo + y_hi),
                                0.5 * (double)(x1 - x0), 0.5 * (y_hi - y_lo) + 0.5);
    for (uint32_t i = tid; i < n; i += BLK) {
        const double4 s4 = S.spheres[i];
        const double s[4] = {s4.x, s4.y, s4.z, s4.w};
        if (beam_may_hit(tile, s)) atomicOr(&bits[i >> 5], 1u << (i & 31u));
    }
    __syncthreads();
    const uint32_t px = x0 + tid % PRIMARY_TILE, prow = r0 + tid / PRIMARY_TILE;
    if (px >= F.W || prow >= F.rows) return;
    const Beam beam = make_beam(C, (double)px, (double)primary_image_row(prow, F.row_offset, F.row_stride), 0.5, 0.5);
    // the pixel's slots, slot k in bits 16 k .. 16 k + 15 of {lo, hi}
    constexpr uint64_t NONE4 = 0x0001000100010001ull * PRIMARY_NONE;
    uint64_t lo = NONE4, hi = NONE4;
    uint32_t cnt = 0;
    for (uint32_t w = 0; w < words; ++w) {
        uint32_t m = bits[w];
        while (m) {
            const uint32_t i = w * 32u + (uint32_t)__ffs((int)m) - 1u;
            m &= m - 1u;
            const double4 s4 = S.spheres[i];
            const double s[4] = {s4.x, s4.y, s4.z, s4.w};
            if (beam_may_hit(beam, s)) {
                const uint32_t sh = (cnt & 3u) * 16u;
                if (cnt < 4u) lo = (lo & ~(0xffffull << sh)) | ((uint64_t)i << sh);
                else if (cnt < PRIMARY_CAP) hi = (hi & ~(0xffffull << sh)) | ((uint64_t)i << sh);
                ++cnt;
            }
        }
    }
    if (cnt > PRIMARY_CAP) lo = (lo & ~0xffffull) | PRIMARY_WALK;
    RT_GLOBAL uint4* dst = (RT_GLOBAL uint4*)P->cand + ((uint64_t)prow * F.W + px);
    *dst = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}

// to_rgb of a linear f32 framebuffer already on the device (e.g. the gathered
// multi-GPU frame).
__global__ void __launch_bounds__(256) rt_to_rgb_kernel(const float* __restrict__ lin, uint8_t* __restrict__ srgb,
                                                       uint64_t n, int toon) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) srgb[i] = srgb_u8((double)lin[i], toon);
}
// Frame row j of a gathered shard came from part j % parts, as that part's
// compact row j / parts.  One thread per float of the frame.
__global__ void __launch_bounds__(256) rt_deinterleave_kernel(const float* __restrict__ staging, uint64_t slice,
                                                              float* __restrict__ out, uint32_t rows, uint32_t W,
                                                              uint32_t parts) {
    const uint64_t row_floats = (uint64_t)W * 3;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)rows * row_floats) return;
    const uint32_t j = (uint32_t)(i / row_floats);
    const uint64_t x = i - (uint64_t)j * row_floats;
    out[i] = staging[(uint64_t)(j % parts) * slice + (uint64_t)(j / parts) * row_floats + x];
}
// The same for a gathered shard's to_rgb bytes.
__global__ void __launch_bounds__(256) rt_deinterleave_u8_kernel(const uint8_t* __restrict__ staging, uint64_t slice,
                                                                 uint8_t* __restrict__ out, uint32_t rows, uint32_t W,
                                                                 uint32_t parts) {
    const uint64_t row_bytes = (uint64_t)W * 3;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)rows * row_bytes) return;
    const uint32_t j = (uint32_t)(i / row_bytes);
    const uint64_t x = i - (uint64_t)j * row_bytes;
    out[i] = staging[(uint64_t)(j % parts) * slice + (uint64_t)(j / parts) * row_bytes + x];
}
}  // namespace rtk

extern "C" int rtk_tier_for(uint32_t features) { return rtk::plan::tier_for(features); }

extern "C" int rtk_block_threads(int tier) { return tier == rtk::TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK; }

extern "C" uint32_t rtk_stack_entries(int tier) {
    return tier == rtk::TIER_BASIC ? RT_STACK_BASIC : RT_STACK_MAX;
}

static void fill_kparams(rtk::KParams& K, const rtk::SceneView* view, const rtk_frame_desc* fd, uint32_t* queue,
                         double* partial, unsigned long long* stats, int tier, int grid, void* stack_ovf,
                         uint32_t static_entries) {
    K.S = *view;
    rtk::Frame& F = K.F;
    F.W = fd->W;
    F.rows = fd->rows;
    F.row_offset = fd->row_offset;
    F.row_stride = fd->row_stride;
    F.S = fd->S;
    F.max_depth = fd->max_depth;
    F.key0 = (uint32_t)fd->seed;
    F.key1 = (uint32_t)(fd->seed >> 32);
    F.total_items = fd->W * fd->rows * fd->S;
    F.parts = fd->parts > 1 ? fd->parts : 1u;  // the host's rtk_row_parts: no part empty
    F.part_len = (fd->S + F.parts - 1) / F.parts;
    F.parts2 = fd->parts2 > 1 ? fd->parts2 : F.parts;
    F.part_len2 = (fd->S + F.parts2 - 1) / F.parts2;
    const uint32_t whole_rows = F.parts > 1 ? (fd->whole_rows < fd->rows ? fd->whole_rows : fd->rows) : fd->rows;
    // the shard's rows from fine_row on are the fine rows (none: rows)
    const uint32_t fine_row = fd->fine_row < whole_rows ? whole_rows : (fd->fine_row < fd->rows ? fd->fine_row : fd->rows);
    F.whole_items = fd->W * whole_rows * fd->S;
    F.fine_item0 = fd->W * fine_row * fd->S;
    F.fine_q0 = F.whole_items + (F.fine_item0 - F.whole_items) * F.parts;
    F.queue_total = F.fine_q0 + (F.total_items - F.fine_item0) * F.parts2;
    F.static_entries = static_entries;
    F.chunk_min = fd->chunk_min;
    F.chunk_min_whole = fd->chunk_min_whole;
    auto inv_up = [](uint32_t d) { return std::nextafter(1.0 / (double)d, 2.0); };
    F.inv_parts = inv_up(F.parts);
    F.inv_parts2 = inv_up(F.parts2);
    F.S_f = (float)F.S;
    F.part_len_f = (float)F.part_len;
    F.part_len2_f = (float)F.part_len2;
    F.inv_S_f = 1.0f / F.S_f;
    F.inv_part_len_f = 1.0f / F.part_len_f;
    F.inv_part_len2_f = 1.0f / F.part_len2_f;
    F.inv_S = inv_up(F.S);
    F.inv_W = inv_up(F.W);
    F.chunk_cap = fd->chunk_cap ? fd->chunk_cap : (tier == rtk::TIER_MESH ? RT_QUEUE_CHUNK_MESH : RT_QUEUE_CHUNK);
    F.inv_guide = 1.0f / (float)((uint64_t)grid * (rtk_block_threads(tier) / 64) * (fd->guide ? fd->guide : RT_QUEUE_GUIDE));
    F.defocus = fd->defocus;
    F.recip_sqrt_spp = fd->recip_sqrt_spp;
    F.pixel_sample_scale = fd->pixel_sample_scale;
    F.center = rtk::D3{fd->center[0], fd->center[1], fd->center[2]};
    F.pixel00 = rtk::D3{fd->pixel00[0], fd->pixel00[1], fd->pixel00[2]};
    F.du = rtk::D3{fd->du[0], fd->du[1], fd->du[2]};
    F.dv = rtk::D3{fd->dv[0], fd->dv[1], fd->dv[2]};
    F.disk_u = rtk::D3{fd->disk_u[0], fd->disk_u[1], fd->disk_u[2]};
    F.disk_v = rtk::D3{fd->disk_v[0], fd->disk_v[1], fd->disk_v[2]};
    K.queue = queue;
    K.partial = partial;
    K.stats = stats;
    K.stack_ovf = (RT_GLOBAL uint2*)stack_ovf;
    K.cand = (const RT_GLOBAL uint4*)fd->primary;
    K.inv_stride = inv_up(F.row_stride);
}

static hipError_t launch_reduce(const rtk_frame_desc* fd, const rtk::Frame& F, double* partial, float* out,
                                uint8_t* srgb, int toon, hipStream_t stream) {
    const uint32_t npix = fd->W * fd->rows;
    // the three regions of the slot order (rtk::Frame): whole rows, tail
    // parts, fine parts; a region whose pixel does not fit the wave's LDS
    // (S x np x 24 B > 16 KiB, e.g. C5's 64 x 16 tail parts) takes the
    // direct kernel for that region
    const uint32_t whole_px = F.whole_items / fd->S, fine_px = F.fine_item0 / fd->S;
    const struct { uint32_t b, e, np; } reg[3] = {
        {0u, whole_px, 1u}, {whole_px, fine_px, F.parts}, {fine_px, npix, F.parts2}};
    uint64_t slot = 0;
    for (const auto& r : reg) {
        if (r.e > r.b) {
            const uint64_t dpp = (uint64_t)fd->S * r.np * 3u;  // doubles per pixel
            if (dpp <= rtk::REDUCE_LDS_DOUBLES) {
                const uint32_t pw = (uint32_t)std::min<uint64_t>(64u, rtk::REDUCE_LDS_DOUBLES / dpp);
                const uint32_t groups = (r.e - r.b + pw - 1u) / pw;
                hipLaunchKernelGGL(rtk::rt_reduce_lds_kernel, dim3(groups), dim3(64), 0, stream, partial, r.b,
                                   r.e, slot, fd->S, r.np, pw, fd->pixel_sample_scale, out, srgb, toon);
            } else {
                const uint32_t waves = (r.e - r.b + rtk::REDUCE_PX_PER_WAVE - 1) / rtk::REDUCE_PX_PER_WAVE;
                hipLaunchKernelGGL(rtk::rt_reduce_kernel, dim3((waves + 3) / 4), dim3(256), 0, stream, partial,
                                   r.b, r.e, fd->S, F.parts, whole_px, F.parts2, fine_px,
                                   fd->pixel_sample_scale, out, srgb, toon);
            }
        }
        slot += (uint64_t)(r.e - r.b) * fd->S * r.np;
    }
    return hipGetLastError();
}

extern "C" hipError_t rtk_launch_frame(const rtk::SceneView* view, const rtk_frame_desc* fd, uint32_t* queue,
                                       double* partial, unsigned long long* stats, float* out, uint8_t* srgb,
                                       int toon, hipStream_t stream, int tier, int grid, void* params_dev,
                                       void* stack_ovf) {
    rtk::KParams K;
    fill_kparams(K, view, fd, queue, partial, stats, tier, grid, stack_ovf,
                 (uint32_t)grid * (uint32_t)rtk_block_threads(tier));
    rtk::KParams* Pd = (rtk::KParams*)params_dev;
    hipError_t e = hipMemcpyAsync(Pd, &K, sizeof K, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(queue, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (fd->ev_start) (void)hipEventRecord((hipEvent_t)fd->ev_start, stream);
    // the basic tier's batch variant reads its primary-ray candidates from the
    // launch's table: filled here, inside the span the events time
    const bool batch = tier == rtk::TIER_BASIC && view->n_nodes4 <= rtk::NODE_LDS_CAP_BATCH;
    if (batch && fd->primary && fd->W && fd->rows) {
        hipLaunchKernelGGL(rtk::rt_primary_kernel, dim3(rtk::primary_tiles(fd->W), rtk::primary_tiles(fd->rows)),
                           dim3(rtk::PRIMARY_TILE * rtk::PRIMARY_TILE), 0, stream, Pd);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // the basic tier: shading batches over trees that leave room for the
    // park area, whole-wave shading over the rest (rt_path_kernel WIDE)
    e = tier == rtk::TIER_BASIC  ? (view->n_nodes4 > rtk::NODE_LDS_CAP_BATCH ? rtk_launch_path_0w(grid, stream, Pd)
                                                                            : rtk_launch_path_0(grid, stream, Pd))
        : tier == rtk::TIER_MESH ? rtk_launch_path_1(grid, stream, Pd)
        : tier == rtk::TIER_FULL ? rtk_launch_path_2(grid, stream, Pd)
        : tier == rtk::TIER_FULL_FLAT ? rtk_launch_path_3(grid, stream, Pd)
        : tier == rtk::TIER_FULL_GL ? rtk_launch_path_4(grid, stream, Pd)
                                    : rtk_launch_path_5(grid, stream, Pd);
    if (e != hipSuccess) return e;
    if (fd->ev_stop) (void)hipEventRecord((hipEvent_t)fd->ev_stop, stream);
    return launch_reduce(fd, K.F, partial, out, srgb, toon, stream);
}

extern "C" hipError_t rtk_launch_deinterleave(const float* staging, size_t slice, float* out, uint32_t rows, uint32_t W,
                                              uint32_t parts, hipStream_t stream) {
    const uint64_t n = (uint64_t)rows * W * 3;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rtk::rt_deinterleave_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, staging,
                       (uint64_t)slice, out, rows, W, parts);
    return hipGetLastError();
}

extern "C" hipError_t rtk_launch_deinterleave_u8(const uint8_t* staging, size_t slice, uint8_t* out, uint32_t rows,
                                                 uint32_t W, uint32_t parts, hipStream_t stream) {
    const uint64_t n = (uint64_t)rows * W * 3;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rtk::rt_deinterleave_u8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, staging,
                       (uint64_t)slice, out, rows, W, parts);
    return hipGetLastError();
}

extern "C" hipError_t rtk_launch_math(int fn, int impl, const double* a, const double* b, double* out, uint64_t n,
                                      hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rtk::rt_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fn, impl, a, b, out,
                       n);
    return hipGetLastError();
}

// doubles per case of walk self-test fn (0 for an unknown fn)
extern "C" int rtk_walk_widths(int fn, int* in_w, int* out_w) {
    static const int IN[7] = {14, 12, 1, 1, 1, 2, 1}, OUT[7] = {2, 2, 1, 1, 1, 1, 1};
    if (fn < 0 || fn > 6) return 0;
    *in_w = IN[fn];
    *out_w = OUT[fn];
    return 1;
}

extern "C" hipError_t rtk_launch_walk(int fn, const double* in, double* out, uint64_t n, hipStream_t stream) {
    int in_w = 0, out_w = 0;
    if (!rtk_walk_widths(fn, &in_w, &out_w)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rtk::rt_walk_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fn, in_w, out_w, in,
                       out, n);
    return hipGetLastError();
}

extern "C" hipError_t rtk_launch_to_rgb(const float* lin, uint8_t* srgb, uint64_t n, int toon, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rtk::rt_to_rgb_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, lin, srgb, n, toon);
    return hipGetLastError();
}

// the frame plan (rt_plan.h), for rt_render.cpp
extern "C" uint32_t rtk_row_parts(uint32_t S, uint32_t part_samples) { return rtk::plan::row_parts(S, part_samples); }

extern "C" uint32_t rtk_tail_rows(uint32_t W, uint32_t H, uint32_t S, uint32_t parts, uint64_t budget_bytes,
                                  uint32_t permille) {
    return rtk::plan::tail_rows(W, H, S, parts, budget_bytes, permille);
}

extern "C" void rtk_tail_split(uint32_t W, uint32_t H, uint32_t S, uint32_t parts, uint32_t parts2,
                               uint64_t budget_bytes, uint32_t permille, uint32_t fine_permille, uint32_t* tail,
                               uint32_t* fine) {
    rtk::plan::tail_split(W, H, S, parts, parts2, budget_bytes, permille, fine_permille, tail, fine);
}

extern "C" uint32_t rtk_shard_whole_rows(uint32_t H, uint32_t tail, uint32_t row_offset, uint32_t row_stride,
                                         uint32_t rows) {
    return rtk::plan::shard_whole_rows(H, tail, row_offset, row_stride, rows);
}

extern "C" size_t rtk_params_bytes(void) { return sizeof(rtk::KParams); }


extern "C" int rtk_path_kernel_occupancy(int tier, int* blocks_per_cu) {
    return tier == rtk::TIER_BASIC  ? rtk_occupancy_0(blocks_per_cu)
         : tier == rtk::TIER_MESH ? rtk_occupancy_1(blocks_per_cu)
         : tier == rtk::TIER_FULL ? rtk_occupancy_2(blocks_per_cu)
         : tier == rtk::TIER_FULL_FLAT ? rtk_occupancy_3(blocks_per_cu)
         : tier == rtk::TIER_FULL_GL ? rtk_occupancy_4(blocks_per_cu)
                                     : rtk_occupancy_5(blocks_per_cu);
}
