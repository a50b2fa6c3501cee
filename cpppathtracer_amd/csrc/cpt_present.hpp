// cpt_present.hpp — presenting an HDR frame: the source colour of a pixel, the
// exposure, the tone curve, the transfer to a byte and the exposure meter's histogram and resolve,
// shared by the device (cpt_present.hip) and the host (cpt_present_host, cpt_meter_host).
//
// f32 `+ - * /`, comparisons, integer operations and one committed table (cpt_present_tables.hpp)
// only, each expression rounded as written (no contraction, no transcendental; `/` is the
// correctly rounded operation of the build), so the device, the host hooks and
// the numpy restatement in tests/present_model.py agree byte for byte and word for word.  The meter
// is an integer histogram: any order of its atomic adds gives the same words.  The reference has no
// counterpart: its display loop clamps to [0, 1] and writes 255.99 * linear (path_tracer.cu:241-254).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cpt.h"
#include "cpt_filter.hpp"
#include "cpt_present_tables.hpp"

namespace cpt {
namespace present {

constexpr int HIST_BINS = 256;               // eight per octave from 2^-16 to 2^16; the ends collect the rest
constexpr int HIST_WORDS = HIST_BINS + 1;    // word 256: the pixels that are not metered
constexpr int HIST_BIAS = 888;               // bits(2^-16) >> 20
constexpr float EXPOSED_MAX = 65504.0f;

struct Rgb { float r, g, b; };

// min and max as the definition's comparisons: a NaN first operand gives the second.
__host__ __device__ inline float lesser(float a, float b) { return a < b ? a : b; }
__host__ __device__ inline float positive(float a) { return a > 0.0f ? a : 0.0f; }   // NaN, negatives and -0 become +0

__host__ __device__ inline uint32_t bits_of(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(x);
#else
    union { float f; uint32_t u; } v;
    v.f = x;
    return v.u;
#endif
}

__host__ __device__ inline float float_of(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    union { float f; uint32_t u; } v;
    v.u = u;
    return v.f;
#endif
}

// The sanitised source colour c' of a pixel from the four floats of its source plane: the
// accumulator's (rgb sums, count) or the filter plane's (rgb, variance).  False: unsourced (an
// accumulator pixel whose count is not positive and finite), c' = 0.
__host__ __device__ inline bool source_colour(int source, float sx, float sy, float sz, float sw, Rgb& c) {
#pragma clang fp contract(off)
    if (source == CPT_PRESENT_ACCUM) {
        if (!(sw > 0.0f && filter::finite(sw))) {
            c = Rgb{0.0f, 0.0f, 0.0f};
            return false;
        }
        c = Rgb{positive(sx / sw), positive(sy / sw), positive(sz / sw)};
        return true;
    }
    c = Rgb{positive(sx), positive(sy), positive(sz)};
    return true;
}

// One component from c' to the tone curve's y in [0, 1].
__host__ __device__ inline float tone(float c, float e, int curve, float white) {
#pragma clang fp contract(off)
    const float x = lesser(c * e, EXPOSED_MAX);
    if (curve == CPT_TONE_REINHARD) return lesser((x * (1.0f + x / (white * white))) / (1.0f + x), 1.0f);
    if (curve == CPT_TONE_ACES)
        return lesser(positive((x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)), 1.0f);
    return lesser(x, 1.0f);
}

// y to a byte.  `T`: the 256 sRGB thresholds (T[0] = 0, so the byte is the last index whose
// threshold is at most y), wherever the caller keeps them.
__host__ __device__ inline uint32_t transfer_byte(float y, int transfer, const float* T) {
#pragma clang fp contract(off)
    if (transfer == CPT_TRANSFER_LINEAR) return (uint32_t)(int)(255.99f * y) & 0xFFu;
    uint32_t pos = 0;
    for (uint32_t step = 128; step != 0; step >>= 1)
        if (T[pos + step] <= y) pos += step;
    return pos;
}

// A pixel's four output bytes as one little-endian word: B, G, R, 255.
__host__ __device__ inline uint32_t pixel_word(int source, float sx, float sy, float sz, float sw, float e, int curve, float white,
                                               int transfer, const float* T) {
    Rgb c;
    source_colour(source, sx, sy, sz, sw, c);
    const uint32_t r = transfer_byte(tone(c.r, e, curve, white), transfer, T);
    const uint32_t g = transfer_byte(tone(c.g, e, curve, white), transfer, T);
    const uint32_t b = transfer_byte(tone(c.b, e, curve, white), transfer, T);
    return b | (g << 8) | (r << 16) | 0xFF000000u;
}

// The histogram word a pixel adds one to: its luminance's bin, or HIST_BINS when it is not metered
// (unsourced, or a luminance that is not finite and positive).
__host__ __device__ inline int meter_word(int source, float sx, float sy, float sz, float sw) {
    Rgb c;
    if (!source_colour(source, sx, sy, sz, sw, c)) return HIST_BINS;
    const float l = filter::luma(filter::Px{c.r, c.g, c.b, 0.0f});
    if (!(l > 0.0f && filter::finite(l))) return HIST_BINS;
    const int bin = (int)(bits_of(l) >> 20) - HIST_BIAS;
    return bin < 0 ? 0 : bin > HIST_BINS - 1 ? HIST_BINS - 1 : bin;
}

// The rank the resolve looks for among N > 0 metered pixels.
__host__ __device__ inline uint64_t meter_rank(uint64_t n, int permille) {
    const uint64_t r = n * (uint64_t)permille / 1000u;
    return r < n - 1 ? r : n - 1;
}

// The exposure after a meter whose percentile fell into bin `b`.
__host__ __device__ inline float adapted(float e, int b, float key, float adapt) {
#pragma clang fp contract(off)
    const float target = key / float_of((uint32_t)(b + HIST_BIAS) << 20);
    return adapt == 1.0f ? target : e + (target - e) * adapt;
}

// The whole resolve on a histogram (the host's; the device scans in parallel): the exposure that
// follows `e`.
inline float resolve(const uint32_t* hist, float e, float key, int permille, float adapt) {
    uint64_t n = 0;
    for (int b = 0; b < HIST_BINS; ++b) n += hist[b];
    if (n == 0) return e;
    const uint64_t rank = meter_rank(n, permille);
    uint64_t cum = 0;
    for (int b = 0; b < HIST_BINS; ++b) {
        cum += hist[b];
        if (cum > rank) return adapted(e, b, key, adapt);
    }
    return e;
}

__host__ __device__ inline bool source_ok(int s) { return s == CPT_PRESENT_ACCUM || s == CPT_PRESENT_FILTERED; }
__host__ __device__ inline bool tone_ok(int t) { return t == CPT_TONE_CLAMP || t == CPT_TONE_REINHARD || t == CPT_TONE_ACES; }
__host__ __device__ inline bool transfer_ok(int t) { return t == CPT_TRANSFER_LINEAR || t == CPT_TRANSFER_SRGB; }
// cpt_present's arguments; white: > 0 (NaN is refused; +inf turns Reinhard's curve into x / (1 + x))
__host__ __device__ inline bool args_ok(int source, int tone, float white, int transfer) {
    return source_ok(source) && tone_ok(tone) && transfer_ok(transfer) && white > 0.f;
}

// The source's four floats of pixel i as the host hooks receive them: [npix][4] for the
// accumulator, [npix][3] for the filtered rgb.
inline void host_pixel(int source, const float* src, size_t i, float S[4]) {
    const int n = source == CPT_PRESENT_ACCUM ? 4 : 3;
    S[0] = src[n * i];
    S[1] = src[n * i + 1];
    S[2] = src[n * i + 2];
    S[3] = n == 4 ? src[n * i + 3] : 0.f;
}

}  // namespace present
}  // namespace cpt
