// cpt_reproject.hpp — reprojection of the accumulated frame and of the display's
// running mean with its per-pixel sample counts (§22) to a moved camera, shared by the device
// (cpt_reproject.hip) and the host (cpt_reproject_host, cpt_reproject_display_host).
//
// Backward reprojection: the new pixel's first hit (or, for the sky, its direction as a point at
// infinity) is projected into the camera the history was rendered with, and the four accumulator
// pixels around that position are blended bilinearly, each only if it saw the same object on the
// new hit's tangent plane.  Means and pass counts are blended apart, so the result is again
// (rgb sum, integer pass count), which every consumer of the accumulator reads.
//
// f32 `+ - * /`, comparisons and floorf only, each expression rounded as written (no contraction,
// no transcendental, no sqrt; `/` is the correctly rounded operation of the build, DESIGN.md
// §Numerics), so the device, the host entry and the numpy restatement in tests/reproject_model.py
// agree bit for bit.  The reference has no counterpart: MotionalCamera::Refresh restarts Mix at
// 1 / 1 when the camera moves (motional_camera.cu, path_tracer.cu:177-254).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cpt.h"
#include "cpt_internal.hpp"

namespace cpt {
namespace reproject {

constexpr float SNAP = 0.03125f;         // 1/32: a position this close to a pixel is that pixel
constexpr float MIN_WEIGHT = 0.015625f;  // 1/64: less valid bilinear weight than this is no history

struct V3 { float x, y, z; };
struct Px { float r, g, b, n; };   // an accumulator pixel: rgb sums and the pass count

__host__ __device__ inline bool finite(float x) {
#pragma clang fp contract(off)
    return x - x == 0.0f;   // inf - inf and NaN - NaN are NaN
}

__host__ __device__ inline float dot(const V3& a, const V3& b) {
#pragma clang fp contract(off)
    return (a.x * b.x + a.y * b.y) + a.z * b.z;
}

__host__ __device__ inline V3 sub(const V3& a, const V3& b) {
#pragma clang fp contract(off)
    return V3{a.x - b.x, a.y - b.y, a.z - b.z};
}

// o + t * d, the point of a G-buffer ray at distance t
__host__ __device__ inline V3 at(const V3& o, float t, const V3& d) {
#pragma clang fp contract(off)
    return V3{o.x + t * d.x, o.y + t * d.y, o.z + t * d.z};
}

// What the projection into the old camera reads of it, from its GetCopy outputs alone:
// T = top_left_corner - origin, Hh = horizontal, Vv = vertical, w, and the five dot products that
// do not depend on the pixel.  Formed once per call, on the host, for the device and the host entry.
struct OldView {
    V3 o, T, Hh, Vv, w;
    float Tw, TH, HH, TV, VV;
    float fw, fh;   // the frame's size
};

inline V3 v3_of(const cpt_float3& a) { return V3{a.x, a.y, a.z}; }

inline OldView old_view(const cpt_camera& c) {
#pragma clang fp contract(off)
    OldView v;
    v.o = v3_of(c.origin);
    v.T = sub(v3_of(c.top_left_corner), v.o);
    v.Hh = v3_of(c.horizontal);
    v.Vv = v3_of(c.vertical);
    v.w = v3_of(c.w);
    v.Tw = dot(v.T, v.w);
    v.TH = dot(v.T, v.Hh);
    v.HH = dot(v.Hh, v.Hh);
    v.TV = dot(v.T, v.Vv);
    v.VV = dot(v.Vv, v.Vv);
    v.fw = (float)c.width;
    v.fh = (float)c.height;
    return v;
}

// The old frame's position (fx, fy), in pixels, of q: a point relative to the old camera's origin,
// or a direction (a point at infinity).  RayGen samples pixel x at dx = x / W, with no centre
// offset, so pixel x sits at fx = x.  false: behind or beside the old camera, or not finite.
__host__ __device__ inline bool project(const OldView& v, const V3& q, float& fx, float& fy) {
#pragma clang fp contract(off)
    const float qw = dot(q, v.w);
    if (!(qw < 0.0f) || !finite(qw)) return false;
    const float s = v.Tw / qw;
    const float dx = (s * dot(q, v.Hh) - v.TH) / v.HH;
    const float dy = (s * dot(q, v.Vv) - v.TV) / v.VV;
    fx = dx * v.fw;
    fy = dy * v.fh;
    return finite(fx) && finite(fy);
}

// A position within SNAP of a pixel becomes that pixel (floorf(f + 0.5f) is rint(f) wherever the
// two can differ by at most SNAP from f).
__host__ __device__ inline float snap(float f) {
#pragma clang fp contract(off)
    const float r = floorf(f + 0.5f);
    float d = f - r;
    if (d < 0.0f) d = -d;
    return d <= SNAP ? r : f;
}

// A tap's history: the accumulator's pixel or, DISPLAY, the display state's.
template <bool DISPLAY, typename Src>
__host__ __device__ inline Px history(const Src& src, size_t k) {
    if constexpr (DISPLAY) return src.shown(k);
    else return src.accum(k);
}

// One output pixel of the accumulator, (rgb sums, integer pass count), or, DISPLAY, of the display
// state (`display_pixel` below).  The geometry is written once, here, for both: the projection
// through OldView, the snap, the frame bounds, the id test, the tangent-plane test; the two differ
// in what a tap holds and how it is blended.  `src` gives the old frame: src.id0(k), src.t0(k) and
// src.dir0(x, y, k) of a pixel k = y * width + x inside it, and its history, src.accum(k) (rgb sums,
// pass count) or, DISPLAY, src.shown(k) (the Mix mean's rgb, sample count), of which only taps
// inside w_eff x h_eff count.  id1, t1, n1 and d1 are the new pixel's G-buffer entry and centre-ray
// direction, o1 the new camera's origin.  One body and no wrapper on the accumulator's side: its
// instantiation compiles to the kernel it was before the display look-up joined it (§22).
template <bool DISPLAY = false, typename Src>
__host__ __device__ inline Px pixel(const Src& src, const OldView& v, const V3& o1, int width, int height, int32_t id1,
                                    float t1, const V3& n1, const V3& d1, float max_history, float plane_tol, int w_eff = 0,
                                    int h_eff = 0) {
#pragma clang fp contract(off)
    const Px none{0.0f, 0.0f, 0.0f, 0.0f};
    const bool hit = id1 >= 0;
    const V3 P = at(o1, t1, d1);
    const V3 q = hit ? sub(P, v.o) : d1;
    float fx, fy;
    if (!project(v, q, fx, fy)) return none;
    fx = snap(fx);
    fy = snap(fy);
    // the taps x0, x0 + 1 (y0, y0 + 1) reach the frame only from here; also keeps the int casts defined
    if (!(fx > -1.0f && fx < v.fw && fy > -1.0f && fy < v.fh)) return none;
    const float flx = floorf(fx), fly = floorf(fy);
    const int x0 = (int)flx, y0 = (int)fly;
    const float wx = fx - flx, wy = fy - fly;
    const float bound = plane_tol * t1;
    float Wt = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
    for (int b = 0; b < 2; ++b)
        for (int a = 0; a < 2; ++a) {
            const int x = x0 + a, y = y0 + b;
            if (x < 0 || x >= width || y < 0 || y >= height) continue;
            if constexpr (DISPLAY)
                if (x >= w_eff || y >= h_eff) continue;
            const size_t k = (size_t)y * width + x;
            if (src.id0(k) != id1) continue;
            const Px A = history<DISPLAY>(src, k);
            if (!(A.n >= 1.0f) || !finite(A.r) || !finite(A.g) || !finite(A.b)) continue;
            if (hit) {
                // the tap's own hit point lies on the new hit's tangent plane
                float pd = dot(sub(at(v.o, src.t0(k), src.dir0(x, y, k)), P), n1);
                if (pd < 0.0f) pd = -pd;
                if (!(pd <= bound)) continue;
            }
            const float wgt = (a ? wx : 1.0f - wx) * (b ? wy : 1.0f - wy);
            // the one tap of weight 1, within the cap: its four floats as they are
            if (wgt == 1.0f && A.n <= max_history) return A;
            Wt += wgt;
            if constexpr (DISPLAY) {   // the mean as it is
                sr += wgt * A.r;
                sg += wgt * A.g;
                sb += wgt * A.b;
            } else {                   // sums: the mean of A.n passes
                sr += wgt * (A.r / A.n);
                sg += wgt * (A.g / A.n);
                sb += wgt * (A.b / A.n);
            }
            sn += wgt * A.n;
        }
    if (!(Wt >= MIN_WEIGHT)) return none;
    const float n = sn / Wt;
    const float cap = floorf(n < max_history ? n : max_history);
    if (!(cap >= 1.0f)) return none;
    if constexpr (DISPLAY) return Px{sr / Wt, sg / Wt, sb / Wt, cap};
    else return Px{(sr / Wt) * cap, (sg / Wt) * cap, (sb / Wt) * cap, cap};
}

// One output pixel (x1, y1) of the display state (cpt_reproject_display): (the Mix
// mean's rgb, the sample count).  The display's launch region is w_eff x h_eff: a pixel outside it
// holds nothing, a tap outside it does not count; the mean is blended as it is, the count beside it.
template <typename Src>
__host__ __device__ inline Px display_pixel(const Src& src, const OldView& v, const V3& o1, int width, int height, int w_eff,
                                            int h_eff, int x1, int y1, int32_t id1, float t1, const V3& n1, const V3& d1,
                                            float max_history, float plane_tol) {
    if (x1 >= w_eff || y1 >= h_eff) return Px{0.0f, 0.0f, 0.0f, 0.0f};
    return pixel<true>(src, v, o1, width, height, id1, t1, n1, d1, max_history, plane_tol, w_eff, h_eff);
}

// The old frame as plain arrays (the host entry).
struct PlaneSrc {
    const Px* in;
    const int32_t* id;
    const float* t;
    const float* dir3;
    __host__ __device__ Px accum(size_t k) const { return in[k]; }
    __host__ __device__ int32_t id0(size_t k) const { return id[k]; }
    __host__ __device__ float t0(size_t k) const { return t[k]; }
    __host__ __device__ V3 dir0(int, int, size_t k) const { return V3{dir3[3 * k], dir3[3 * k + 1], dir3[3 * k + 2]}; }
};

// The old frame's display state as plain arrays (the host entry): mean [npix][3], count [npix].
struct DisplayPlaneSrc {
    const float* mean3;
    const float* count;
    const int32_t* id;
    const float* t;
    const float* dir3;
    __host__ __device__ Px shown(size_t k) const { return Px{mean3[3 * k], mean3[3 * k + 1], mean3[3 * k + 2], count[k]}; }
    __host__ __device__ int32_t id0(size_t k) const { return id[k]; }
    __host__ __device__ float t0(size_t k) const { return t[k]; }
    __host__ __device__ V3 dir0(int, int, size_t k) const { return V3{dir3[3 * k], dir3[3 * k + 1], dir3[3 * k + 2]}; }
};

}  // namespace reproject

// k_reproject_accum's arguments (cpt_reproject.hip): both cameras as ray_gen_centre reads them, the
// old one as the projection reads it, the G-buffer planes of a width x height full frame (id0, t0
// at the old camera; id1, t1, normal1 at the new one), the accumulator and the plane the result
// goes to (not the same).
struct ReprojectArgs {
    CamK cam0, cam1;
    reproject::OldView view0;
    int width, height;
    const int32_t* id0;
    const float* t0;
    const int32_t* id1;
    const float* t1;
    const float* normal1;
    const float4* in;
    float4* out;
    float max_history, plane_tol;
};
hipError_t launch_reproject(const ReprojectArgs& a, hipStream_t stream);

// k_reproject_display's arguments: the same cameras and G-buffer planes; the display state of the
// width x height frame (the Mix mean [npix][3] and the count plane [npix], of which the launch
// region w_eff x h_eff is used) and the planes the result goes to (not the same).
struct ReprojectDisplayArgs {
    CamK cam0, cam1;
    reproject::OldView view0;
    int width, height, w_eff, h_eff;
    const int32_t* id0;
    const float* t0;
    const int32_t* id1;
    const float* t1;
    const float* normal1;
    const float* mean_in;
    const float* count_in;
    float* mean_out;
    float* count_out;
    float max_history, plane_tol;
};
hipError_t launch_reproject_display(const ReprojectDisplayArgs& a, hipStream_t stream);

}  // namespace cpt
