// cpt_filter.hpp — the variance-guided a-trous filter of an adaptive render's final frame
// (DESIGN.md §19), shared by the device (cpt_filter.hip) and the host (cpt_filter_level_host,
// cpt_filter_prepare_host), and its variant for frames without moments (DESIGN.md §25,
// cpt_filter_frame_spatial): level 0 from a spatial variance estimate, levels guided by the G-buffer.
//
// An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with SVGF's variance guidance:
// level l runs a 5x5 B3-spline stencil at step 1 << l over the mean image, edge-stopped by the
// first-hit normal and by luminance differences scaled with the pixel's own variance of the mean,
// and propagates that variance.
//
// f32 `+ - * /` only, each expression rounded as written (no contraction, no transcendental; `/`
// is the correctly rounded operation of the build), so the device, the host
// hooks and the numpy restatements in tests/filter_model.py and tests/filter_spatial_model.py agree
// bit for bit.  The reference has no
// counterpart: its only filter is the per-pass Denoising + Mix (path_tracer.cu:177-254).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_adaptive.hpp"

namespace cpt {
namespace filter {

constexpr int MAX_LEVELS = 8;
constexpr int MAX_SHARPNESS_LOG2 = 10;

struct Px { float r, g, b, v; };   // a pixel of a plane: the mean's rgb and the variance of the mean

__host__ __device__ inline bool finite(float x) {
#pragma clang fp contract(off)
    return x - x == 0.0f;   // inf - inf and NaN - NaN are NaN
}

__host__ __device__ inline float luma(const Px& c) {
#pragma clang fp contract(off)
    return (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b;
}

// Level 0 of a pixel from its accumulator S = (rgb sums, count) and its moments (m1, m2, k of the
// batch means' luminance, cpt_adaptive.hpp): the mean, and the variance of the mean decide() forms
// under its square root.  An invalid pixel (no pass, fewer than two batch means, or a value that
// is not finite) keeps what was computed (0 where the count is 0) through every level and is no
// tap of any other pixel.
__host__ __device__ inline bool prepare(float sx, float sy, float sz, float n, float m1, float m2, float k, Px& out) {
#pragma clang fp contract(off)
    const Px c{sx / n, sy / n, sz / n, (adaptive::max_keep_nan(k * m2 - m1 * m1, 0.0f) / (k * (k - 1.0f))) / k};
    const bool valid = n > 0.0f && k >= 2.0f && finite(c.r) && finite(c.g) && finite(c.b) && finite(c.v);
    out = n == 0.0f ? Px{0.0f, 0.0f, 0.0f, 0.0f} : c;
    return valid;
}

// One output pixel of one level.  `src` gives the level's input: src.valid(x, y) for a pixel
// inside the frame, src.px(x, y) and src.normal(x, y, n) for a valid one.  sig2 = sigma_l *
// sigma_l.  The caller handles invalid pixels (out = in).  ID_STOP (§25): a tap of another object,
// src.id(qx, qy) != src.id(x, y), is skipped as an invalid one is, in the prefilter too.
template <typename Src, bool ID_STOP = false>
__host__ __device__ inline Px level_pixel(const Src& src, int x, int y, int width, int height, int step, float sig2,
                                          int sharpness_log2) {
#pragma clang fp contract(off)
    const Px cp = src.px(x, y);
    float np[3];
    src.normal(x, y, np);
    const float lp = luma(cp);
    [[maybe_unused]] int idp = 0;
    if constexpr (ID_STOP) idp = src.id(x, y);
    // the variance the luminance stop is scaled by: a 3x3 Gaussian of the neighbours' variances
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= width || qy < 0 || qy >= height || !src.valid(qx, qy)) continue;
            if constexpr (ID_STOP)
                if (src.id(qx, qy) != idp) continue;
            const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            gs += g * src.px(qx, qy).v;
            gw += g;
        }
    const float den = sig2 * (gs / gw) + 1e-10f;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
    for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx, qy = y + step * dy;
            if (qx < 0 || qx >= width || qy < 0 || qy >= height || !src.valid(qx, qy)) continue;
            if constexpr (ID_STOP)
                if (src.id(qx, qy) != idp) continue;
            const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
            const float h = (ax == 0 ? 0.375f : ax == 1 ? 0.25f : 0.0625f) * (ay == 0 ? 0.375f : ay == 1 ? 0.25f : 0.0625f);
            const Px cq = src.px(qx, qy);
            float w = h;
            if (dx != 0 || dy != 0) {
                const float d = lp - luma(cq);
                const float wl = den / (den + d * d);
                float nq[3];
                src.normal(qx, qy, nq);
                float wn = adaptive::max_keep_nan((np[0] * nq[0] + np[1] * nq[1]) + np[2] * nq[2], 0.0f);
                for (int i = 0; i < sharpness_log2; ++i) wn = wn * wn;
                w = h * (wn * wl);
            }
            sw += w;
            sr += w * cq.r;
            sg += w * cq.g;
            sb += w * cq.b;
            sv += (w * w) * cq.v;
        }
    return Px{sr / sw, sg / sw, sb / sw, sv / (sw * sw)};
}

// The level's input as plain arrays: planes of `width` pixels per row.
struct PlaneSrc {
    const Px* in;
    const float* normal3;
    const uint8_t* ok;
    int width;
    __host__ __device__ bool valid(int x, int y) const { return ok[(size_t)y * width + x] != 0; }
    __host__ __device__ Px px(int x, int y) const { return in[(size_t)y * width + x]; }
    __host__ __device__ void normal(int x, int y, float n[3]) const {
        const float* p = normal3 + 3 * ((size_t)y * width + x);
        n[0] = p[0];
        n[1] = p[1];
        n[2] = p[2];
    }
};

// PlaneSrc with the G-buffer's object ids, for level_pixel<Src, true>.
struct PlaneIdSrc : PlaneSrc {
    const int32_t* ids;
    __host__ __device__ int id(int x, int y) const { return ids[(size_t)y * width + x]; }
};

// ---- Level 0 without moments ----
//
// Base validity b(p) and the level-0 colour of a pixel from its accumulator alone: b holds when the
// count is positive and finite and the mean is finite; the colour is the mean, 0 where the count is 0.
constexpr int SPATIAL_RADIUS = 3;

__host__ __device__ inline bool spatial_base(float sx, float sy, float sz, float n, Px& out) {
#pragma clang fp contract(off)
    const Px c{sx / n, sy / n, sz / n, 0.0f};
    out = n == 0.0f ? Px{0.0f, 0.0f, 0.0f, 0.0f} : c;
    return n > 0.0f && finite(n) && finite(c.r) && finite(c.g) && finite(c.b);
}

// The spatial variance of the mean of a base-valid pixel: the count-weighted variance of the
// luminances l_q of the base-valid pixels q of the same object in the 7x7 window, each weighted by
// its normal's agreement with the pixel's (1 at the centre).  n_q (l_q - mu)^2 estimates the
// per-pass variance whatever n_q is, so s2 is per pass and s2 / n_p is the pixel's own.
// `src.tap(x, y)` gives a pixel inside the frame whole, as one SpatialTap: its base validity and,
// for a base-valid one, luminance, count, id and normal (the device fetches its two 16-byte LDS
// slots once per tap).  Two passes over the window; 0 with fewer than two taps of positive weight.
struct SpatialTap {
    float nx, ny, nz, l, n;
    int id;
    bool base;
};

template <typename Src>
__host__ __device__ inline float spatial_variance(const Src& src, int x, int y, int width, int height, int sharpness_log2) {
#pragma clang fp contract(off)
    const SpatialTap p = src.tap(x, y);
    float mu = 0.0f, sa = 0.0f, sb = 0.0f, sw = 0.0f, sd = 0.0f;
    int m = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int dy = -SPATIAL_RADIUS; dy <= SPATIAL_RADIUS; ++dy)
            for (int dx = -SPATIAL_RADIUS; dx <= SPATIAL_RADIUS; ++dx) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= width || qy < 0 || qy >= height) continue;
                const SpatialTap q = src.tap(qx, qy);
                if (!q.base || q.id != p.id) continue;
                float w = 1.0f;
                if (dx != 0 || dy != 0) {
                    w = adaptive::max_keep_nan((p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz, 0.0f);
                    for (int i = 0; i < sharpness_log2; ++i) w = w * w;
                }
                const float a = w * q.n, lq = q.l;
                if (pass == 0) {
                    sa += a;
                    sb += a * lq;
                    sw += w;
                    if (w > 0.0f) ++m;
                } else {
                    const float d = lq - mu;
                    sd += a * (d * d);
                }
            }
        if (pass == 0) mu = sb / sa;
    }
    float s2 = 0.0f;
    if (m >= 2) {
        const float mf = (float)m;
        s2 = (sd / sw) * (mf / (mf - 1.0f));
    }
    return s2 / p.n;
}

// Level 0 of a pixel: (c0, v0) and the final validity, b(p) and a finite v0.  v0 = 0 where !b(p).
template <typename Src>
__host__ __device__ inline bool prepare_spatial(const Src& src, int x, int y, int width, int height, float sx, float sy, float sz,
                                                float n, int sharpness_log2, Px& out) {
    const bool b = spatial_base(sx, sy, sz, n, out);
    if (!b) return false;
    out.v = spatial_variance(src, x, y, width, height, sharpness_log2);
    return finite(out.v);
}

// prepare_spatial's input as plain arrays: each pixel's luminance, count and base validity (from
// spatial_base), and the G-buffer's id and normal planes.
struct SpatialPlaneSrc {
    const float* l;
    const float* n;
    const uint8_t* b;
    const int32_t* ids;
    const float* normal3;
    int width;
    __host__ __device__ SpatialTap tap(int x, int y) const {
        const size_t i = (size_t)y * width + x;
        return SpatialTap{normal3[3 * i], normal3[3 * i + 1], normal3[3 * i + 2], l[i], n[i], ids[i], b[i] != 0};
    }
};

}  // namespace filter
}  // namespace cpt
