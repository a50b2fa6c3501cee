// cpt_reproject.hpp — reprojection of the accumulated frame and of the display's
// running mean with its per-pixel sample counts (§22) to a moved camera, shared by the device
// (cpt_reproject.hip) and the host (cpt_reproject_host, cpt_reproject_display_host); and the tracked
// variants of both (§23), which follow edited objects back to where the history saw them.
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

#include <cstring>

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

// Tracked reprojection: where an object stood when the history was captured.  One
// record per object index, derived on the host from the object as captured (0) and as it is now (1)
// and read by the look-up as a plain table.  Every kind is an axis-aligned scaling plus a
// translation, so the hit's normal is the same on both sides.
//   SAME      geometry and material fields bytewise equal: the point is not touched
//   SPHERE    c0 + (P - c1) * (r0 / r1)
//   CYLINDER  x, z: c0 + (P - c1) * (r0 / r1); y: c0.y + (P.y - c1.y) * (h0 / h1)
//   PLATFORM  (P.x, y_pos0, P.z)
//   DROP      no history: another primitive type, a changed material (its radiance is stale), a
//             divisor that is not finite or <= 0, a scale that is not finite
// Field by field, bytewise (-0 is not 0, a NaN equals itself); the structs' padding is not data.
inline bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

inline bool same_material(const cpt_material& a, const cpt_material& b) {
    if (a.type != b.type || (a.have_tex != 0) != (b.have_tex != 0)) return false;
    if (a.have_tex ? a.u.tex != b.u.tex
                   : !(same_bits(a.u.kd.x, b.u.kd.x) && same_bits(a.u.kd.y, b.u.kd.y) && same_bits(a.u.kd.z, b.u.kd.z)))
        return false;
    return same_bits(a.refractive_index, b.refractive_index) && same_bits(a.emit_intensity, b.emit_intensity) &&
           same_bits(a.smoothness, b.smoothness) && same_bits(a.reflectivity, b.reflectivity);
}

inline bool same_geometry(const cpt_object& a, const cpt_object& b) {
    return a.type == b.type && same_bits(a.center.x, b.center.x) && same_bits(a.center.y, b.center.y) &&
           same_bits(a.center.z, b.center.z) && same_bits(a.radius, b.radius) && same_bits(a.y_pos, b.y_pos) &&
           same_bits(a.height, b.height);
}

inline cpt_object_motion motion_of(const cpt_object& o0, const cpt_object& o1) {
#pragma clang fp contract(off)
    cpt_object_motion m;
    std::memset(&m, 0, sizeof(m));
    m.c0 = o0.center;
    m.c1 = o1.center;
    m.s_xz = m.s_y = 1.0f;
    const bool same_mat = same_material(o0.material, o1.material), same_geo = same_geometry(o0, o1);
    m.kind = CPT_MOTION_DROP;
    if (same_mat && same_geo) {
        m.kind = CPT_MOTION_SAME;
    } else if (same_mat && o0.type == o1.type) {
        const bool r_ok = finite(o1.radius) && o1.radius > 0.0f, h_ok = finite(o1.height) && o1.height > 0.0f;
        if (o1.type == CPT_PRIM_SPHERE && r_ok) {
            m.s_xz = m.s_y = o0.radius / o1.radius;
            if (finite(m.s_xz)) m.kind = CPT_MOTION_SPHERE;
        } else if (o1.type == CPT_PRIM_CYLINDER && r_ok && h_ok) {
            m.s_xz = o0.radius / o1.radius;
            m.s_y = o0.height / o1.height;
            if (finite(m.s_xz) && finite(m.s_y)) m.kind = CPT_MOTION_CYLINDER;
        } else if (o1.type == CPT_PRIM_PLATFORM) {
            m.c0.y = o0.y_pos;
            m.c1.y = o1.y_pos;
            m.kind = CPT_MOTION_PLATFORM;
        }
    }
    return m;
}

// pixel's `motion` of the untracked look-ups: none, and no code.
struct NoMotion {
    static constexpr bool TRACKED = false;
};

// pixel's `motion` of the tracked look-ups: the table (nullptr: nothing was edited since the capture).
struct TableMotion {
    static constexpr bool TRACKED = true;
    const cpt_object_motion* table;
    // P, a point of object `id` now, becomes the point it was at the capture; false: no history
    __host__ __device__ bool to_old(int32_t id, V3& P) const {
#pragma clang fp contract(off)
        if (!table) return true;
        const cpt_object_motion m = table[id];
        if (m.kind == CPT_MOTION_SAME) return true;
        if (m.kind == CPT_MOTION_PLATFORM) {
            P.y = m.c0.y;
            return true;
        }
        if (m.kind != CPT_MOTION_SPHERE && m.kind != CPT_MOTION_CYLINDER) return false;
        P = V3{m.c0.x + (P.x - m.c1.x) * m.s_xz, m.c0.y + (P.y - m.c1.y) * m.s_y, m.c0.z + (P.z - m.c1.z) * m.s_xz};
        return true;
    }
};

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
// `motion` (§23): TableMotion maps the new hit point to the point its object held when the history
// was captured, and that point stands for P in the projection and the plane test; NoMotion, the
// default, adds no code: both untracked kernels compile to the instructions they were.
template <bool DISPLAY = false, typename Src, typename Motion = NoMotion>
__host__ __device__ inline Px pixel(const Src& src, const OldView& v, const V3& o1, int width, int height, int32_t id1,
                                    float t1, const V3& n1, const V3& d1, float max_history, float plane_tol, int w_eff = 0,
                                    int h_eff = 0, const Motion& motion = Motion{}) {
#pragma clang fp contract(off)
    const Px none{0.0f, 0.0f, 0.0f, 0.0f};
    const bool hit = id1 >= 0;
    V3 P = at(o1, t1, d1);
    if constexpr (Motion::TRACKED)   // the hit point as its object held it at the capture (§23)
        if (hit && !motion.to_old(id1, P)) return none;
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
template <typename Src, typename Motion = NoMotion>
__host__ __device__ inline Px display_pixel(const Src& src, const OldView& v, const V3& o1, int width, int height, int w_eff,
                                            int h_eff, int x1, int y1, int32_t id1, float t1, const V3& n1, const V3& d1,
                                            float max_history, float plane_tol, const Motion& motion = Motion{}) {
    if (x1 >= w_eff || y1 >= h_eff) return Px{0.0f, 0.0f, 0.0f, 0.0f};
    return pixel<true, Src, Motion>(src, v, o1, width, height, id1, t1, n1, d1, max_history, plane_tol, w_eff, h_eff, motion);
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

// The arguments of k_reproject (cpt_reproject.hip), one struct per look-up.  The accumulator's: both
// cameras as ray_gen_centre reads them, the old one as the projection reads it, the G-buffer planes
// of a width x height full frame (id0, t0 at the old camera; id1, t1, normal1 at the new one), the
// accumulator and the plane the result goes to (not the same).
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

// The display's: the same cameras and G-buffer planes; the display state of the width x height
// frame (the Mix mean [npix][3] and the count plane [npix], of which the launch region
// w_eff x h_eff is used) and the planes the result goes to (not the same).
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

// A tracked look-up's: the untracked one's, with id0 / t0 the captured history's
// planes and cam0 / view0 its camera; the motion table (one record per object index; nullptr: no
// object was edited since the capture) and the planes that take the new frame's id and distance,
// the next call's history (not id0 / t0).
template <typename Look>
struct ReprojectTracked {
    Look look;
    const cpt_object_motion* motion;
    int32_t* id_next;
    float* t_next;
};

template <typename Args> constexpr bool is_tracked = false;
template <typename Look> constexpr bool is_tracked<ReprojectTracked<Look>> = true;

// The untracked struct inside either kind of argument.
template <typename Look> __host__ __device__ inline Look& look_of(ReprojectTracked<Look>& a) { return a.look; }
template <typename Look> __host__ __device__ inline const Look& look_of(const ReprojectTracked<Look>& a) { return a.look; }
template <typename Look> __host__ __device__ inline Look& look_of(Look& a) { return a; }

// Defined in cpt_reproject.hip for the four argument types.
template <typename Args> hipError_t launch_reproject(const Args& args, hipStream_t stream);

}  // namespace cpt
