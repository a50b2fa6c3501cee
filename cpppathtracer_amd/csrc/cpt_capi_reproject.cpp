// cpt_capi_reproject.cpp — the C-ABI's reprojection of the accumulated frame (include/cpt.h,
// cpt_reproject_accum) and of the display state (§22: cpt_reproject_display) to a
// moved camera, their timing, and the host-only entries on the same arithmetic.  The G-buffers
// are cpt_query.hip's kernel, the look-ups cpt_reproject.hip's; the arithmetic is
// cpt_reproject.hpp's on both sides.
#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>

#include "cpt_context.hpp"
#include "cpt_query.hpp"
#include "cpt_reproject.hpp"

using namespace cpt::ctx;
namespace rp = cpt::reproject;

namespace {

constexpr uint32_t WALK_FLAGS = CPT_TRAVERSAL_ORDERED | CPT_TRAVERSAL_PLAIN_LEAVES;

bool args_ok(int max_history, float plane_tol) { return max_history >= 1 && rp::finite(plane_tol) && plane_tol >= 0.f; }

// What cpt_reproject_accum and cpt_reproject_display (`who`) ask before they write anything.
int checked(cpt_ctx* c, const char* who, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
            uint32_t flags) {
    if (!from || !to) return fail(c, CPT_ERR_INVALID_ARG, "%s: a camera is NULL", who);
    if (flags & ~WALK_FLAGS) return fail(c, CPT_ERR_INVALID_ARG, "%s: flags 0x%x (only CPT_TRAVERSAL_* bits)", who, flags);
    if (!args_ok(max_history, plane_tol))
        return fail(c, CPT_ERR_INVALID_ARG, "%s: max_history %d (>= 1), plane_tol %g (finite, >= 0)", who, max_history,
                    (double)plane_tol);
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "%s: cpt_set_scene first", who);
    if (!c->frame.set || c->n_rows != c->height) return fail(c, CPT_ERR_STATE, "%s: needs a full frame", who);
    for (int y = 0; y < c->height; ++y)
        if (c->rows_h[y] != y) return fail(c, CPT_ERR_STATE, "%s: needs rows 0..height-1 in order", who);
    CPT_REFUSE_PENDING(c, who);
    for (const cpt_camera* cam : {from, to})
        if (cam->width != c->width || cam->height != c->height)
            return fail(c, CPT_ERR_INVALID_ARG, "%s: camera %dx%d vs frame %dx%d", who, cam->width, cam->height, c->width, c->height);
    if (n_tiles(c) > (size_t)(UINT32_MAX / 64))
        return fail(c, CPT_ERR_UNSUPPORTED, "%s: frame of %zu 8x8 tiles (max %u)", who, n_tiles(c), UINT32_MAX / 64);
    return CPT_OK;
}

// The planes both calls trace into: the frame's G-buffer and the history's id and distance.
int ensure_planes(cpt_ctx* c) {
    GBufferState& g = c->frame.gbuffer;
    ReprojectState& r = c->frame.reproject;
    const size_t npix = c->npix();
    int rc;
    if ((rc = g.d_id.ensure(c, npix)) != CPT_OK || (rc = g.d_t.ensure(c, npix)) != CPT_OK ||
        (rc = g.d_normal.ensure(c, 3 * npix)) != CPT_OK || (rc = g.d_albedo.ensure(c, 3 * npix)) != CPT_OK ||
        (rc = r.d_id.ensure(c, npix)) != CPT_OK || (rc = r.d_t.ensure(c, npix)) != CPT_OK)
        return rc;
    return CPT_OK;
}

// The two traces, with the call's first three timing events: the G-buffer at `from` into the
// history planes (its normals pass through the frame's normal plane, which the second trace
// overwrites), then the G-buffer at `to` into the frame's own.
int trace_pair(cpt_ctx* c, const cpt::KParams& p0, const cpt::KParams& p1, hipStream_t s) {
    GBufferState& g = c->frame.gbuffer;
    ReprojectState& r = c->frame.reproject;
    HIP_TRY(c, hipEventRecord(c->t_reproject.t0, s));
    HIP_TRY(c, cpt::launch_ray_query(p0, c->d_rank_obj, nullptr, cpt::QueryPixels{-1, -1},
                                     cpt::QueryOut{r.d_id, r.d_t, g.d_normal, nullptr}, s));
    HIP_TRY(c, hipEventRecord(c->ev_reproject[0], s));
    HIP_TRY(c, cpt::launch_ray_query(p1, c->d_rank_obj, nullptr, cpt::QueryPixels{-1, -1},
                                     cpt::QueryOut{g.d_id, g.d_t, g.d_normal, g.d_albedo}, s));
    g.valid = true;
    HIP_TRY(c, hipEventRecord(c->ev_reproject[1], s));
    return CPT_OK;
}

}  // namespace

extern "C" {

int cpt_reproject_accum(cpt_ctx* c, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
                        uint32_t flags) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (int rc = checked(c, "cpt_reproject_accum", from, to, max_history, plane_tol, flags)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    Frame& f = c->frame;
    GBufferState& g = f.gbuffer;
    ReprojectState& r = f.reproject;
    int rc;
    if ((rc = ensure_planes(c)) != CPT_OK || (rc = r.d_accum.ensure(c, c->npix())) != CPT_OK) return rc;
    cpt::KParams p0, p1;
    fill_params(c, from, 0, 0, flags, p0);
    fill_params(c, to, 0, 0, flags, p1);
    cpt::ReprojectArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam0 = p0.cam;
    a.cam1 = p1.cam;
    a.view0 = rp::old_view(*from);
    a.width = c->width;
    a.height = c->height;
    a.id0 = r.d_id;
    a.t0 = r.d_t;
    a.id1 = g.d_id;
    a.t1 = g.d_t;
    a.normal1 = g.d_normal;
    a.in = f.d_accum;
    a.out = r.d_accum;
    a.max_history = (float)max_history;
    a.plane_tol = plane_tol;
    hipStream_t s = c->stream();
    if ((rc = trace_pair(c, p0, p1, s)) != CPT_OK) return rc;
    HIP_TRY(c, cpt::launch_reproject(a, s));
    HIP_TRY(c, hipEventRecord(c->t_reproject.t1, s));
    c->t_reproject.recorded = true;
    // the second plane is the accumulator from here on: work already queued holds the old pointer
    // by value and runs before the kernel; every later call reads the member
    std::swap(f.d_accum, r.d_accum);
    // the moments no longer describe the accumulator
    f.adaptive.done = false;
    return CPT_OK;
}

int cpt_reproject_display(cpt_ctx* c, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
                          uint32_t flags) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (int rc = checked(c, "cpt_reproject_display", from, to, max_history, plane_tol, flags)) return rc;
    Frame& f = c->frame;
    DisplayBand& d = f.display;
    const int w_eff = 16 * (c->width / 16), h_eff = 16 * (c->height / 16);
    if (!d.d_mix) return fail(c, CPT_ERR_STATE, "cpt_reproject_display: no display pass yet");
    if (d.y0 != 0 || d.y1 != h_eff)
        return fail(c, CPT_ERR_STATE, "cpt_reproject_display: the display holds the band [%d, %d), not the full frame", d.y0, d.y1);
    HIP_TRY(c, hipSetDevice(c->device));
    GBufferState& g = f.gbuffer;
    ReprojectState& r = f.reproject;
    const size_t npix = c->npix();
    int rc;
    if ((rc = ensure_planes(c)) != CPT_OK || (rc = d.d_mix_next.ensure(c, 3 * npix)) != CPT_OK ||
        (rc = d.d_count_next.ensure(c, npix)) != CPT_OK)
        return rc;
    cpt::KParams p0, p1;
    fill_params(c, from, 0, 0, flags, p0);
    fill_params(c, to, 0, 0, flags, p1);
    cpt::ReprojectDisplayArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cam0 = p0.cam;
    a.cam1 = p1.cam;
    a.view0 = rp::old_view(*from);
    a.width = c->width;
    a.height = c->height;
    a.w_eff = w_eff;
    a.h_eff = h_eff;
    a.id0 = r.d_id;
    a.t0 = r.d_t;
    a.id1 = g.d_id;
    a.t1 = g.d_t;
    a.normal1 = g.d_normal;
    a.mean_in = d.d_mix;
    a.count_in = d.d_count;
    a.mean_out = d.d_mix_next;
    a.count_out = d.d_count_next;
    a.max_history = (float)max_history;
    a.plane_tol = plane_tol;
    hipStream_t s = c->stream();
    if ((rc = d.fill_count(c)) != CPT_OK || (rc = trace_pair(c, p0, p1, s)) != CPT_OK) return rc;
    HIP_TRY(c, cpt::launch_reproject_display(a, s));
    HIP_TRY(c, hipEventRecord(c->t_reproject.t1, s));
    c->t_reproject.recorded = true;
    // the second planes are the display state from here on (as the accumulator's above); the
    // kernel wrote every pixel of the frame, so they need no clearing
    std::swap(d.d_mix, d.d_mix_next);
    std::swap(d.d_count, d.d_count_next);
    return CPT_OK;
}

int cpt_last_reproject_ms(cpt_ctx* c, float* ms) {
    if (!c || !ms) return CPT_ERR_INVALID_ARG;
    if (!c->t_reproject.recorded) return fail(c, CPT_ERR_STATE, "cpt_last_reproject_ms: no cpt_reproject_accum or cpt_reproject_display yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->t_reproject.t1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->t_reproject.t0, c->t_reproject.t1));
    return CPT_OK;
}

int cpt_last_reproject_launch_ms(cpt_ctx* c, float* ms3) {
    if (!c || !ms3) return CPT_ERR_INVALID_ARG;
    if (!c->t_reproject.recorded) return fail(c, CPT_ERR_STATE, "cpt_last_reproject_launch_ms: no cpt_reproject_accum or cpt_reproject_display yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->t_reproject.t1));
    const hipEvent_t ev[4] = {c->t_reproject.t0, c->ev_reproject[0], c->ev_reproject[1], c->t_reproject.t1};
    for (int k = 0; k < 3; ++k) HIP_TRY(c, hipEventElapsedTime(ms3 + k, ev[k], ev[k + 1]));
    return CPT_OK;
}

int cpt_reproject_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                       const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                       const float* normal1, const float* accum_in, int max_history, float plane_tol, float* accum_out) {
    if (!cam0 || !cam1 || width <= 0 || height <= 0 || !dir0 || !dir1 || !id0 || !t0 || !id1 || !t1 || !normal1 || !accum_in ||
        !accum_out || accum_in == accum_out || !args_ok(max_history, plane_tol))
        return CPT_ERR_INVALID_ARG;
    for (const cpt_camera* cam : {cam0, cam1})
        if (cam->width != width || cam->height != height) return CPT_ERR_INVALID_ARG;
    const rp::OldView v = rp::old_view(*cam0);
    const rp::V3 o1 = rp::v3_of(cam1->origin);
    const rp::PlaneSrc src{reinterpret_cast<const rp::Px*>(accum_in), id0, t0, dir0};
    rp::Px* out = reinterpret_cast<rp::Px*>(accum_out);
    const size_t npix = (size_t)width * height;
    for (size_t i = 0; i < npix; ++i)
        out[i] = rp::pixel(src, v, o1, width, height, id1[i], t1[i], rp::V3{normal1[3 * i], normal1[3 * i + 1], normal1[3 * i + 2]},
                           rp::V3{dir1[3 * i], dir1[3 * i + 1], dir1[3 * i + 2]}, (float)max_history, plane_tol);
    return CPT_OK;
}

int cpt_reproject_display_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                               const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                               const float* normal1, const float* mean_in, const float* count_in, int max_history,
                               float plane_tol, float* mean_out, float* count_out) {
    if (!cam0 || !cam1 || width <= 0 || height <= 0 || !dir0 || !dir1 || !id0 || !t0 || !id1 || !t1 || !normal1 || !mean_in ||
        !count_in || !mean_out || !count_out || mean_in == mean_out || count_in == count_out || !args_ok(max_history, plane_tol))
        return CPT_ERR_INVALID_ARG;
    for (const cpt_camera* cam : {cam0, cam1})
        if (cam->width != width || cam->height != height) return CPT_ERR_INVALID_ARG;
    const rp::OldView v = rp::old_view(*cam0);
    const rp::V3 o1 = rp::v3_of(cam1->origin);
    const rp::DisplayPlaneSrc src{mean_in, count_in, id0, t0, dir0};
    const int w_eff = 16 * (width / 16), h_eff = 16 * (height / 16);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const rp::Px r = rp::display_pixel(src, v, o1, width, height, w_eff, h_eff, x, y, id1[i], t1[i],
                                               rp::V3{normal1[3 * i], normal1[3 * i + 1], normal1[3 * i + 2]},
                                               rp::V3{dir1[3 * i], dir1[3 * i + 1], dir1[3 * i + 2]}, (float)max_history, plane_tol);
            mean_out[3 * i] = r.r;
            mean_out[3 * i + 1] = r.g;
            mean_out[3 * i + 2] = r.b;
            count_out[i] = r.n;
        }
    return CPT_OK;
}

}  // extern "C"
