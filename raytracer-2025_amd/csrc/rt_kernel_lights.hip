// rt_kernel_lights.hip -- rt_lights_pdf's and rt_lights_sample's kernels and
// their host entry points.  An object of its own in the product build, as the
// other queries' are: no path-kernel object sees a further caller of the
// lights' device functions (rt_lights.h).
#include <hip/hip_runtime.h>

#include "../../include/rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_builds.h"
#include "rt_geom.h"
#include "rt_lights.h"

namespace rtk {

// ------------------------------------------------------------------ lights queries
// rt_lights_pdf: lights.pdf_value(origin, direction) (hit.rs:46-60 through
// HittablePDF::value, pdf.rs:66-88) for n caller-given (origin, direction)
// pairs; rt_lights_sample: lights.random(origin) and the pdf_value of that
// draw, `samples` times an origin.  Nothing here walks the world: no LDS, no
// traversal stack, and of the scene only what rt_lights.h reads (the lights'
// list children, transforms, planars and spheres).
//
// Both kernels call the general pair, light_pdf_tree<RT_LIGHT_DEPTH> and
// light_random_tree<RT_LIGHT_DEPTH>, on S.lights_root whatever the world's
// tier.  On a flat list or a single primitive the general pair does the
// operations of the flat-list pair (light_pdf / light_random, tiers 2 and 3)
// in the same order -- the children's values summed in list order from 0.0 and
// divided by the count; the child choice drawn first, then the primitive's two
// -- and under -ffp-contract=off no operation is fused or reassociated, so the
// results are the render's bits on every tier.
//
// Memory.  An item's inputs are packed 24-B triples and the sample record is
// 40 B; neither is a vector width, and both are only 8-B aligned.  A lane
// reads its own triple as three 8-B loads and writes its record as five 8-B
// stores (the flags and the reserved word as one): the 64 lanes of a wave
// cover 1 536 contiguous bytes of each input and 2 560 of the output, so every
// 128-B line a wave touches is used whole, and the three (five) instructions
// of a wave hit the same lines while they are in the CU's cache.  Measured
// (profiles/r21/lights_rate.json): the sample kernel is bound by
// its arithmetic (two Philox blocks, a correctly rounded sqrt and a division
// or more a draw) at 12-16 % of the HBM rate; the pdf kernel moves its 56 B an
// item at half the HBM peak in this form.  A transposition through LDS into
// 16-B accesses was not built: the unit uses no LDS.
struct LightsParams {
    SceneView S;
    const double* origins;  // n x 3
    const double* dirs;     // n x 3 (pdf query)
    double* pdf_out;        // n (pdf query)
    rt_light_sample* out;   // n x samples (sample query)
    uint64_t items;         // pdf: n; sample: n * samples < 2^40
    uint32_t samples;       // >= 1
    uint32_t first_index;   // the Rng pixel of origin 0; first_index + n <= 2^32
    uint32_t key0, key1;
};

__global__ void __launch_bounds__(RT_BLOCK) rt_lights_pdf_kernel(const LightsParams P) {
    const SceneView& S = P.S;
    const uint64_t stride = (uint64_t)gridDim.x * RT_BLOCK;
    for (uint64_t j = (uint64_t)blockIdx.x * RT_BLOCK + threadIdx.x; j < P.items; j += stride) {
        const double* po = P.origins + 3 * j;
        const double* pd = P.dirs + 3 * j;
        const D3 o = d3(po[0], po[1], po[2]);
        const D3 d = d3(pd[0], pd[1], pd[2]);
        // (Hittables::pdf_value's panic on a NaN sum is the NaN returned)
        bool panic = false;
        P.pdf_out[j] = light_pdf_tree<RT_LIGHT_DEPTH>(S, S.lights_root, o, d, panic);  // j < n: nothing past out[n - 1]
    }
}

__global__ void __launch_bounds__(RT_BLOCK) rt_lights_sample_kernel(const LightsParams P) {
    const SceneView& S = P.S;
    Rng rng;
    rng.k0 = P.key0;
    rng.k1 = P.key1;
    const uint64_t stride = (uint64_t)gridDim.x * RT_BLOCK;
    for (uint64_t j = (uint64_t)blockIdx.x * RT_BLOCK + threadIdx.x; j < P.items; j += stride) {
        const uint64_t i = j / P.samples;  // < 2^32 - first_index
        const double* po = P.origins + 3 * i;
        const D3 o = d3(po[0], po[1], po[2]);
        rng.pixel = P.first_index + (uint32_t)i;
        rng.sample = (uint32_t)(j - i * P.samples);
        rng.begin(1);
        uint32_t ovf = 0;  // (a lights tree draws at most 6 of the vertex's 16 slots)
        bool ok = true;
        D3 dir = light_random_tree<RT_LIGHT_DEPTH>(S, S.lights_root, o, rng, ovf, ok);
        double pdf = 0.0;
        uint64_t flags = 0;
        if (ok) {
            bool panic = false;
            pdf = light_pdf_tree<RT_LIGHT_DEPTH>(S, S.lights_root, o, dir, panic);
        } else {  // one of random's expects failed: zeros and the flag
            dir = d3(0.0, 0.0, 0.0);
            flags = RT_LIGHT_PANIC;
        }
        // the record as five 8-B words: dir, pdf, {flags, reserved = 0}
        double* q = reinterpret_cast<double*>(P.out + j);  // j < n * samples: nothing past the last record
        q[0] = dir.x;
        q[1] = dir.y;
        q[2] = dir.z;
        q[3] = pdf;
        reinterpret_cast<uint64_t*>(q)[4] = flags;
    }
}

static_assert(sizeof(rt_light_sample) == 40 && offsetof(rt_light_sample, pdf) == 24 &&
                  offsetof(rt_light_sample, flags) == 32 && offsetof(rt_light_sample, reserved) == 36,
              "rt_lights_sample_kernel writes the record as five 8-B words");

static dim3 lights_grid(uint64_t items, int grid) {
    const uint64_t blocks = (items + RT_BLOCK - 1) / RT_BLOCK;
    return dim3((unsigned)(blocks < (uint64_t)grid ? blocks : (uint64_t)grid));
}

}  // namespace rtk

// lights.pdf_value of n (origin, direction) pairs (rt_lights_pdf): device
// arrays of n x 3 doubles in, n doubles out; at most `grid` blocks of RT_BLOCK.
// view->lights_root names a lights object (the caller's check).
extern "C" hipError_t rtk_launch_lights_pdf(const rtk::SceneView* view, const double* origins3, const double* dirs3,
                                            double* out, uint64_t n, int grid, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (grid < 1 || view->lights_root == rtk::REF_NONE) return hipErrorInvalidValue;
    rtk::LightsParams P{};
    P.S = *view;
    P.origins = origins3;
    P.dirs = dirs3;
    P.pdf_out = out;
    P.items = n;
    P.samples = 1;
    hipLaunchKernelGGL(rtk::rt_lights_pdf_kernel, rtk::lights_grid(n, grid), dim3(RT_BLOCK), 0, stream, P);
    return hipGetLastError();
}

// `samples` draws of lights.random for each of n origins, with their
// pdf_value (rt_lights_sample): n x 3 doubles in, n x samples records out.
// first_index + n <= 2^32 and n * samples < 2^40 (the caller's checks, made
// again here: an item's origin index is cut to the Rng's 32-bit pixel).
extern "C" hipError_t rtk_launch_lights_sample(const rtk::SceneView* view, const double* origins3, rt_light_sample* out,
                                               uint64_t n, uint64_t seed, uint32_t first_index, uint32_t samples, int grid,
                                               hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (grid < 1 || samples == 0 || view->lights_root == rtk::REF_NONE || n > (1ull << 32) - first_index ||
        n >= (1ull << 40) / samples + ((1ull << 40) % samples != 0))
        return hipErrorInvalidValue;
    rtk::LightsParams P{};
    P.S = *view;
    P.origins = origins3;
    P.out = out;
    P.items = n * samples;
    P.samples = samples;
    P.first_index = first_index;
    P.key0 = (uint32_t)seed;
    P.key1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(rtk::rt_lights_sample_kernel, rtk::lights_grid(P.items, grid), dim3(RT_BLOCK), 0, stream, P);
    return hipGetLastError();
}
