// cpt_adaptive.hpp — the adaptive render's stop criterion (DESIGN.md §Adaptive sampling), shared
// by the device (cpt_adaptive.hip k_tile_noise) and the host (cpt_adaptive_decide_host).
//
// f32 only, each expression rounded as written (no contraction; `/` and sqrtf are the correctly
// rounded operations of the build), so the device, the host hook and the
// numpy restatement in tests/adaptive_model.py agree bit for bit.  The reference has no
// counterpart: it gives every pixel the same number of passes (path_tracer.cu:124-175).
#pragma once

#include <hip/hip_runtime.h>

namespace cpt {
namespace adaptive {

constexpr float REL_FLOOR = 1e-3f;   // means below it are held to an absolute error of t * floor

// max(a, b) that returns a NaN `a` (a > b ? a : b would return b), so a NaN moment reaches the
// comparison in decide() and makes it false.
__host__ __device__ inline float max_keep_nan(float a, float b) { return a < b ? b : a; }

// The luminance of one round's batch mean: S, n the accumulator's rgb sums and count after the
// round, P, n0 before it.
__host__ __device__ inline float batch_luma(float sr, float sg, float sb, float n, float pr, float pg, float pb,
                                            float n0) {
#pragma clang fp contract(off)
    const float dn = n - n0;
    const float br = (sr - pr) / dn, bg = (sg - pg) / dn, bb = (sb - pb) / dn;
    return (0.2126f * br + 0.7152f * bg) + 0.0722f * bb;
}

// One more batch mean into a pixel's moments.
__host__ __device__ inline void add_batch(float& m1, float& m2, float& k, float y) {
#pragma clang fp contract(off)
    m1 += y;
    m2 += y * y;
    k += 1.0f;
}

// stderr(mean) <= t * max(mean, floor) on the k batch means with sum m1 and sum of squares m2,
// without a division: k m2 - m1^2 <= (k - 1) t^2 max(m1, k floor)^2.  Needs k >= 2; a NaN on
// either side is "not converged".  `rel` is the same quantity as a ratio, for the noise map
// only (+inf while k < 2).
__host__ __device__ inline bool decide(float m1, float m2, float k, float t, float& rel) {
#pragma clang fp contract(off)
    const float q = max_keep_nan(k * m2 - m1 * m1, 0.0f);
    const float mm = max_keep_nan(m1, k * REL_FLOOR);
    const float rhs = ((k - 1.0f) * (t * t)) * (mm * mm);
    const bool enough = k >= 2.0f;
    rel = enough ? __builtin_sqrtf((q / (k * (k - 1.0f))) / k) / (mm / k) : __builtin_inff();
    return enough && q <= rhs;
}

}  // namespace adaptive
}  // namespace cpt
