// cpt_antialias.hpp — antialiased presentation: the sub-sample rays of a pixel, the
// edge test on the G-buffer, the attribution of a sub-sample's first hit to a pixel of the 3x3
// block, the coverage word and the coverage-weighted resolve, shared by the device
// (cpt_antialias.hip) and the host (cpt_aa_rays_host, cpt_aa_coverage_host, cpt_present_aa_host).
//
// f32 `+ - * /`, one sqrt (RayGen's normalisation), comparisons and integer operations only, each
// expression rounded as written (no contraction; `/` and sqrt are the correctly rounded operations
// of the build), so the device, the host hooks and the numpy restatement in
// tests/antialias_model.py agree bit for bit.  The tone curve and the byte transfer are
// cpt_present.hpp's.  The reference has no counterpart: RayGen shoots every pass of a pixel through
// (x / W, y / H) (motional_camera.cu:202-213).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cpt.h"
#include "cpt_internal.hpp"
#include "cpt_present.hpp"

namespace cpt {
namespace antialias {

constexpr uint32_t FLAG_EDGE = 1u;        // the pixel traced its sub-samples
constexpr uint32_t FLAG_UNMATCHED = 2u;   // a sub-sample saw a surface no centre of the 3x3 block holds
constexpr int SELF = 4;                   // the pixel itself among the nine of its block, row-major

__host__ __device__ inline bool samples_ok(int s) { return s == 2 || s == 4; }
// NaN is refused
__host__ __device__ inline bool normal_cos_ok(float c) { return c >= -1.0f && c <= 1.0f; }

__host__ __device__ inline float dot3(const float* a, const float* b) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// Sub-sample s = j * S + i (i across, j down) of pixel (x, y): ray_gen_centre's ray (cpt_path.hpp),
// operation for operation, through ((x + ox) / W, (y + oy) / H) with ox = (2i + 1 - S) / 2S, an
// exact float; the quotients are IEEE f32's, negative at x = 0 or y = 0 for the first sub-samples.
__host__ __device__ inline void sub_ray(const CamK& c, int S, int x, int y, int s, float o[3], float d[3]) {
#pragma clang fp contract(off)
    const int i = s % S, j = s / S;
    const float ox = float(2 * i + 1 - S) / float(2 * S), oy = float(2 * j + 1 - S) / float(2 * S);
    const float dx = (float(x) + ox) / float(c.width), dy = (float(y) + oy) / float(c.height);
    float v[3];
    for (int k = 0; k < 3; ++k) {
        const float offset = c.u[k] * 0.0f + c.v[k] * 0.0f;   // the lens sample taken as zero
        o[k] = c.origin[k] + offset;
        v[k] = (((c.top_left[k] + dx * c.horizontal[k]) + dy * c.vertical[k]) - c.origin[k]) - offset;
    }
    const float inv = 1.0f / __builtin_sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    for (int k = 0; k < 3; ++k) d[k] = v[k] * inv;
}

// Pixel (x, y) is an edge pixel: an in-frame 8-neighbour holds another object, or the pixel hit
// something and a neighbour's normal turns away from its own by more than normal_cos allows.
__host__ __device__ inline bool is_edge(int W, int H, int x, int y, const int32_t* id, const float* normal3, float normal_cos) {
    const size_t p = (size_t)y * W + x;
    const int32_t idp = id[p];
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx, qy = y + dy;
            if ((dx == 0 && dy == 0) || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const size_t q = (size_t)qy * W + qx;
            if (id[q] != idp) return true;
            if (idp >= 0 && dot3(normal3 + 3 * p, normal3 + 3 * q) < normal_cos) return true;
        }
    return false;
}

// The pixel k (0..8) of (x, y)'s block that a sub-sample's hit (id_s, n_s) goes to: the nearest
// in-frame pixel whose centre saw the same surface, distances in units of 1/2S between the
// sub-sample at (2i + 1 - S, 2j + 1 - S) and the pixel at (2S dx, 2S dy); ties to the pixel itself,
// then to the lowest k.  -1: no pixel of the block matches (the caller counts it on SELF and flags
// the pixel unmatched).
__host__ __device__ inline int attribute(int W, int H, int x, int y, int S, int s, int32_t id_s, const float* n_s, const int32_t* id,
                                         const float* normal3, float normal_cos) {
    const int sx = 2 * (s % S) + 1 - S, sy = 2 * (s / S) + 1 - S;
    int best = -1, best_d = 0;
    for (int pass = 0; pass < 2; ++pass)   // the pixel itself first: it keeps a tie
        for (int k = pass == 0 ? SELF : 0; k < (pass == 0 ? SELF + 1 : 9); ++k) {
            if (pass == 1 && k == SELF) continue;
            const int dx = k % 3 - 1, dy = k / 3 - 1;
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const size_t q = (size_t)qy * W + qx;
            if (id[q] != id_s) continue;
            if (id_s != -1 && !(dot3(n_s, normal3 + 3 * q) >= normal_cos)) continue;
            const int ex = sx - 2 * S * dx, ey = sy - 2 * S * dy;
            const int dist = ex * ex + ey * ey;
            if (best < 0 || dist < best_d) {
                best = k;
                best_d = dist;
            }
        }
    return best;
}

// The coverage of a pixel as one 16-byte word: nine counts (bytes 0..8, summing to S x S), the flag
// bits (byte 9), six bytes of padding.
struct Coverage {
    uint32_t c[9];
    uint32_t flags;
};

__host__ __device__ inline uint4 pack(const Coverage& v) {
    return make_uint4(v.c[0] | (v.c[1] << 8) | (v.c[2] << 16) | (v.c[3] << 24), v.c[4] | (v.c[5] << 8) | (v.c[6] << 16) | (v.c[7] << 24),
                      v.c[8] | (v.flags << 8), 0u);
}
__host__ __device__ inline Coverage unpack(const uint4& w) {
    Coverage v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v.c[k] = (w.x >> (8 * k)) & 0xFFu;
        v.c[4 + k] = (w.y >> (8 * k)) & 0xFFu;
    }
    v.c[8] = w.z & 0xFFu;
    v.flags = (w.z >> 8) & 0xFFu;
    return v;
}
// A pixel that traced nothing: all S x S on itself.
__host__ __device__ inline uint4 pack_self(uint32_t s2) { return make_uint4(0u, s2, 0u, 0u); }
__host__ __device__ inline bool all_on_self(const uint4& w, uint32_t s2) { return (w.y & 0xFFu) == s2; }

// The four output bytes of pixel (x, y) under coverage `v`: per channel the tone-mapped values of
// the covered pixels of its block (cpt_present.hpp: source, exposure, curve), summed in ascending k
// from zero with their counts as weights, scaled by 1 / S^2 (exact), then cpt_present's transfer.
// fetch(q, S4): the source's four floats of pixel q.  A count on a pixel outside the frame is
// skipped (the coverage kernels never produce one).
template <typename Fetch>
__host__ __device__ inline uint32_t pixel_word(const Fetch& fetch, int W, int H, int x, int y, const Coverage& v, int S, int source, float e,
                                               int curve, float white, int transfer, const float* T) {
#pragma clang fp contract(off)
    float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        if (v.c[k] == 0) continue;
        const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        float s4[4];
        fetch((size_t)qy * W + qx, s4);
        present::Rgb c;
        present::source_colour(source, s4[0], s4[1], s4[2], s4[3], c);
        const float w = float(v.c[k]);
        acc[0] = acc[0] + w * present::tone(c.r, e, curve, white);
        acc[1] = acc[1] + w * present::tone(c.g, e, curve, white);
        acc[2] = acc[2] + w * present::tone(c.b, e, curve, white);
    }
    const float inv = 1.0f / float(S * S);
    const uint32_t r = present::transfer_byte(acc[0] * inv, transfer, T);
    const uint32_t g = present::transfer_byte(acc[1] * inv, transfer, T);
    const uint32_t b = present::transfer_byte(acc[2] * inv, transfer, T);
    return b | (g << 8) | (r << 16) | 0xFF000000u;
}

}  // namespace antialias

// The kernels' launchers (cpt_antialias.hip).  `cov`: a 16-byte coverage word per pixel; `list`: the
// edge pixels, in no particular order; `count`: their number, a device word.
// launch_aa_edges zeroes the count on the stream, classifies every pixel of the W x H G-buffer
// planes, writes the word of each non-edge pixel and appends the others to the list.
hipError_t launch_aa_edges(const int32_t* id, const float* normal3, int width, int height, int samples, float normal_cos, uint4* cov,
                           uint32_t* list, uint32_t* count, hipStream_t stream);
// launch_aa_coverage traces samples^2 first-hit rays per listed pixel through the walk of `p` (its
// scene part and camera are read; the LDS kernel under use_lds_tree) and writes their words; the
// list's length is read on the device.  A persistent grid, sized by `grid`.
hipError_t launch_aa_coverage(const KParams& p, const int32_t* rank_obj, const int32_t* id, const float* normal3, int samples,
                              float normal_cos, const uint32_t* list, const uint32_t* count, uint4* cov, LaunchGrid& grid,
                              hipStream_t stream);
// launch_present_aa: launch_present (cpt_present.hip) resolved through the coverage words.
hipError_t launch_present_aa(const float4* src, const uint4* cov, int width, int height, int samples, int source, int tone, float white,
                             int transfer, const uint32_t* words, uint8_t* bgra, hipStream_t stream);

}  // namespace cpt
