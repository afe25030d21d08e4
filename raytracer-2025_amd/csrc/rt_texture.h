// rt_texture.h -- Texture::value on the device, and the sky gradient.
#pragma once
#include "rt_kernel.h"
#include "rt_math.h"

namespace rtk {

// ------------------------------------------------------------------ textures
// texture.rs: SolidColor 33-36, CheckerTexture 60-73, ImageTexture 165-174,
// NoiseTexture 191-196 (+ perlin.rs), book-1 sky.
// Full tiers: the block's LDS copy of the world's first Perlin table (9 KiB,
// copied at launch), read by NoiseTexture instead of global memory: the
// marble's 7 octaves are 14 dependent table reads per shade, and a shading
// batch with one marble hit waits for all of them.
__shared__ DPerlin g_perlin_lds;

template <class PP>
__device__ double perlin_noise(PP P, D3 p) {
    const double fx = floor(p.x), fy = floor(p.y), fz = floor(p.z);
    const int64_t i = (int64_t)fx, j = (int64_t)fy, k = (int64_t)fz;
    const double u = p.x - fx, v = p.y - fy, w = p.z - fz;
    const double uu = u * u * (3.0 - 2.0 * u), vv = v * v * (3.0 - 2.0 * v), ww = w * w * (3.0 - 2.0 * w);
    double accum = 0.0;
    for (int di = 0; di < 2; ++di)
        for (int dj = 0; dj < 2; ++dj)
            for (int dk = 0; dk < 2; ++dk) {
                const int idx = P->perm[0][(uint64_t)(i + di) & 255] ^ P->perm[1][(uint64_t)(j + dj) & 255] ^
                                P->perm[2][(uint64_t)(k + dk) & 255];
                const D3 c = d3(P->randvec[idx][0], P->randvec[idx][1], P->randvec[idx][2]);
                const D3 wv = d3(u - di, v - dj, w - dk);
                accum += (di * uu + (1 - di) * (1.0 - uu)) * (dj * vv + (1 - dj) * (1.0 - vv)) *
                         (dk * ww + (1 - dk) * (1.0 - ww)) * dot(c, wv);
            }
    return accum;
}

__device__ void image_pixel(const SceneView& S, const DTexture& t, int64_t x, int64_t y, float out[4]) {
    x = x < 0 ? 0 : (x > t.a - 1 ? t.a - 1 : x);
    y = y < 0 ? 0 : (y > t.b - 1 ? t.b - 1 : y);
    const RT_GLOBAL float* px = S.texels + t.data + ((uint64_t)y * t.a + x) * 4;
    out[0] = px[0];
    out[1] = px[1];
    out[2] = px[2];
    out[3] = px[3];
}

// ImageTexture::get_pixel (texture.rs:109-158): nearest or bilinear, u / v
// wrapped by x - floor(x), v flipped; t.b != 0 (a loaded image)
__device__ __forceinline__ void image_rgba(const SceneView& S, const DTexture& t, double u, double v, float px[4]) {
    const double uu = u - floor(u);
    const double vv = 1.0 - (v - floor(v));
    if (!t.c) {
        const uint32_t i = (uint32_t)(uu * (double)t.a), j = (uint32_t)(vv * (double)t.b);
        image_pixel(S, t, i, j, px);
        return;
    }
    const double x = uu * (double)t.a - 0.5, y = vv * (double)t.b - 0.5;
    const uint32_t x0 = (uint32_t)fmax(floor(x), 0.0), y0 = (uint32_t)fmax(floor(y), 0.0);
    const uint32_t x1 = min(x0 + 1, (uint32_t)t.a - 1), y1 = min(y0 + 1, (uint32_t)t.b - 1);
    const float dx = (float)(x - (double)x0), dy = (float)(y - (double)y0);
    float p00[4], p10[4], p01[4], p11[4];
    image_pixel(S, t, x0, y0, p00);
    image_pixel(S, t, x1, y0, p10);
    image_pixel(S, t, x0, y1, p01);
    image_pixel(S, t, x1, y1, p11);
    for (int c = 0; c < 4; ++c) {
        const float v0 = p00[c] * (1.0f - dx) + p10[c] * dx;
        const float v1 = p01[c] * (1.0f - dx) + p11[c] * dx;
        px[c] = v0 * (1.0f - dy) + v1 * dy;
    }
}
// ImageTexture::alpha (texture.rs:99-106): 1 for a missing image
__device__ __forceinline__ double tex_alpha(const SceneView& S, int tid, double u, double v) {
    const DTexture& t = S.textures[tid];
    if (t.b == 0) return 1.0;
    float px[4];
    image_rgba(S, t, u, v, px);
    return (double)px[3];
}

// the sky gradient (rt_tex_sky_gradient, include/rt_mi355x.h) at the unit direction's y
__device__ __forceinline__ D3 sky_value(const double* c0, const double* c1, double py) {
    const double a = 0.5 * (py + 1.0);
    return (1.0 - a) * d3(c0[0], c0[1], c0[2]) + a * d3(c1[0], c1[1], c1[2]);
}
__device__ __forceinline__ D3 sky_value(const DTexture& t, double py) { return sky_value(t.color, t.color2, py); }

template <bool FULL, bool PL = false>  // PL: NoiseTexture reads the LDS copy of the first Perlin table
__device__ D3 tex_value(const SceneView& S, int tid, double u, double v, D3 p) {
    for (int guard = 0; guard < 16; ++guard) {
        const DTexture& t = S.textures[tid];
        switch (t.type) {
            case T_SOLID: return d3(t.color[0], t.color[1], t.color[2]);
            case T_SKY: return sky_value(t, p.y);
            case T_CHECKER: {
                const int32_t xi = (int32_t)floor(t.scale * p.x), yi = (int32_t)floor(t.scale * p.y),
                              zi = (int32_t)floor(t.scale * p.z);
                tid = ((xi + yi + zi) % 2 == 0) ? t.a : t.b;
                continue;
            }
            default: break;
        }
        if constexpr (FULL) {
          switch (t.type) {
            case T_IMAGE: {
                if (t.b == 0) return d3(0.0, 1.0, 1.0);  // texture.rs:167-169
                float px[4];
                image_rgba(S, t, u, v, px);
                return d3(px[0], px[1], px[2]);
            }
            case T_NOISE: {
                const bool lds = PL && t.data == 0;
                double accum = 0.0, weight = 1.0;
                D3 tp = p;
                for (int o = 0; o < 7; ++o) {
                    accum += weight * (lds ? perlin_noise((const RT_LDS DPerlin*)&g_perlin_lds, tp)
                                           : perlin_noise(S.perlin + t.data, tp));
                    tp = 2.0 * tp;
                    weight = 0.5 * weight;
                }
                const double turb = fabs(accum);
                return (1.0 + k_sin(t.scale * p.z + 10.0 * turb)) * d3(0.5, 0.5, 0.5);
            }
            default: break;
          }
        }
        return d3(0.0, 0.0, 0.0);
    }
    return d3(0.0, 0.0, 0.0);
}

}  // namespace rtk
