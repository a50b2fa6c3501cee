// cpt_bloom.hpp — bloom for presented frames: the bright pass, the pyramid's
// down-step and up-step, the accumulation's order and the composite in front of the tone curve,
// shared by the device (cpt_bloom.hip) and the host (cpt_bloom_host, cpt_present_bloom_host).
//
// cpt_present.hpp's rules: f32 `+ - * /`, comparisons and integer operations only, each expression
// rounded as written (no contraction, no transcendental), so the device, the host hooks and the
// numpy restatement in tests/bloom_model.py agree bit for bit and byte for byte.  Every value is
// defined per texel from the level before it.  lesser, positive, source_colour, filter::luma,
// tone and transfer_byte are cpt_present.hpp's.  The reference has no counterpart.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cpt.h"
#include "cpt_present.hpp"

namespace cpt {
namespace bloom {

using present::Rgb;

constexpr int MAX_LEVELS = CPT_BLOOM_MAX_LEVELS;

// The levels of a W x H frame: level 0 is the frame, level l has (w[l-1] + 1) / 2 columns and rows
// alike; off[l]: where level l starts in the one plane that holds levels 1..MAX_LEVELS, in texels.
struct Pyramid {
    int w[MAX_LEVELS + 1], h[MAX_LEVELS + 1];
    size_t off[MAX_LEVELS + 2];
};

__host__ __device__ inline Pyramid pyramid_of(int W, int H) {
    Pyramid p;
    p.w[0] = W;
    p.h[0] = H;
    p.off[0] = p.off[1] = 0;
    for (int l = 1; l <= MAX_LEVELS; ++l) {
        p.w[l] = (p.w[l - 1] + 1) / 2;
        p.h[l] = (p.h[l - 1] + 1) / 2;
        p.off[l + 1] = p.off[l] + (size_t)p.w[l] * p.h[l];
    }
    return p;
}

__host__ __device__ inline int clampi(int v, int last) { return v < 0 ? 0 : v > last ? last : v; }

// x of a pixel, tone's own first step per component: finite and >= 0 for every input.
__host__ __device__ inline Rgb exposed(int source, float sx, float sy, float sz, float sw, float e) {
#pragma clang fp contract(off)
    Rgb c;
    present::source_colour(source, sx, sy, sz, sw, c);
    return Rgb{present::lesser(c.r * e, present::EXPOSED_MAX), present::lesser(c.g * e, present::EXPOSED_MAX),
               present::lesser(c.b * e, present::EXPOSED_MAX)};
}

// The bright pass b of an exposed pixel x: the share of its luminance above the threshold.
__host__ __device__ inline Rgb bright(const Rgb& x, float threshold) {
#pragma clang fp contract(off)
    const float l = filter::luma(filter::Px{x.r, x.g, x.b, 0.0f});
    const float k = l > 0.0f ? present::positive(l - threshold) / l : 0.0f;
    return Rgb{x.r * k, x.g * k, x.b * k};
}

__host__ __device__ inline float tap4(float t0, float t1, float t2, float t3) {
#pragma clang fp contract(off)
    return (t0 + 3.0f * t1) + (3.0f * t2 + t3);
}

// Texel (X, Y) of the level below a w x h level `T` (T(x, y): an Rgb of it): columns 2X - 1 ..
// 2X + 2 and rows alike, each clamped into the level; the four rows summed first.
template <class Fetch>
__host__ __device__ inline Rgb down(const Fetch& T, int w, int h, int X, int Y) {
#pragma clang fp contract(off)
    float r[4], g[4], b[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = clampi(2 * Y - 1 + j, h - 1);
        Rgb t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) t[i] = T(clampi(2 * X - 1 + i, w - 1), y);
        r[j] = tap4(t[0].r, t[1].r, t[2].r, t[3].r);
        g[j] = tap4(t[0].g, t[1].g, t[2].g, t[3].g);
        b[j] = tap4(t[0].b, t[1].b, t[2].b, t[3].b);
    }
    return Rgb{tap4(r[0], r[1], r[2], r[3]) * 0.015625f, tap4(g[0], g[1], g[2], g[3]) * 0.015625f,
               tap4(b[0], b[1], b[2], b[3]) * 0.015625f};
}

// up(T) at texel (x, y) of the level above the wc x hc level `T`: the texel's parent weighs 3 and
// the neighbour on the texel's side 1, per axis.
template <class Fetch>
__host__ __device__ inline Rgb up(const Fetch& T, int wc, int hc, int x, int y) {
#pragma clang fp contract(off)
    const int px = x >> 1, py = y >> 1;
    const int qx = clampi(px + ((x & 1) ? 1 : -1), wc - 1), qy = clampi(py + ((y & 1) ? 1 : -1), hc - 1);
    const Rgb a = T(px, py), b = T(qx, py), c = T(px, qy), d = T(qx, qy);
    const float hr0 = 3.0f * a.r + b.r, hg0 = 3.0f * a.g + b.g, hb0 = 3.0f * a.b + b.b;
    const float hr1 = 3.0f * c.r + d.r, hg1 = 3.0f * c.g + d.g, hb1 = 3.0f * c.b + d.b;
    return Rgb{(3.0f * hr0 + hr1) * 0.0625f, (3.0f * hg0 + hg1) * 0.0625f, (3.0f * hb0 + hb1) * 0.0625f};
}

__host__ __device__ inline Rgb sum(const Rgb& a, const Rgb& b) {
#pragma clang fp contract(off)
    return Rgb{a.r + b.r, a.g + b.g, a.b + b.b};
}

// A pixel's four output bytes (B, G, R, 255) from its exposed x and its glow g = up(U_1).
__host__ __device__ inline uint32_t pixel_word(const Rgb& x, const Rgb& g, float intensity, int curve, float white, int transfer,
                                               const float* T) {
#pragma clang fp contract(off)
    const float xr = x.r + intensity * g.r, xg = x.g + intensity * g.g, xb = x.b + intensity * g.b;
    const uint32_t r = present::transfer_byte(present::tone(xr, 1.0f, curve, white), transfer, T);
    const uint32_t gg = present::transfer_byte(present::tone(xg, 1.0f, curve, white), transfer, T);
    const uint32_t b = present::transfer_byte(present::tone(xb, 1.0f, curve, white), transfer, T);
    return b | (gg << 8) | (r << 16) | 0xFF000000u;
}

__host__ __device__ inline bool levels_ok(int levels) { return levels >= 1 && levels <= MAX_LEVELS; }
// finite and >= 0 (NaN fails both comparisons' conjunction)
__host__ __device__ inline bool amount_ok(float v) { return v >= 0.0f && filter::finite(v); }

}  // namespace bloom

// The launches of cpt_bloom.hip.  `pyr`: levels 1..MAX_LEVELS of the W x H frame in one plane of
// float4 texels (rgb, 0) at Pyramid::off; `words`: cpt_present's histogram and exposure word.
// launch_bloom builds U_1..U_levels of the source plane at the exposure the word holds.
hipError_t launch_bloom(const float4* src, int W, int H, int source, float threshold, int levels, const uint32_t* words, float4* pyr,
                        hipStream_t stream);
// launch_present_bloom: launch_present (cpt_present.hip) with intensity * up(U_1) added in front of the tone curve.
hipError_t launch_present_bloom(const float4* src, const float4* pyr, int W, int H, int source, int tone, float white, int transfer,
                                float intensity, const uint32_t* words, uint8_t* bgra, hipStream_t stream);

}  // namespace cpt
