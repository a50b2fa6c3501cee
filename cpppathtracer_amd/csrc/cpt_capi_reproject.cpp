// cpt_capi_reproject.cpp — the C-ABI's reprojection of the accumulated frame to a moved camera
// (include/cpt.h): cpt_reproject_accum, its timing, and the host-only entry on the
// same arithmetic.  The G-buffers are cpt_query.hip's kernel, the look-up cpt_reproject.hip's; the
// arithmetic is cpt_reproject.hpp's on both sides.
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

}  // namespace

extern "C" {

int cpt_reproject_accum(cpt_ctx* c, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
                        uint32_t flags) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!from || !to) return fail(c, CPT_ERR_INVALID_ARG, "cpt_reproject_accum: a camera is NULL");
    if (flags & ~WALK_FLAGS) return fail(c, CPT_ERR_INVALID_ARG, "cpt_reproject_accum: flags 0x%x (only CPT_TRAVERSAL_* bits)", flags);
    if (!args_ok(max_history, plane_tol))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_reproject_accum: max_history %d (>= 1), plane_tol %g (finite, >= 0)", max_history,
                    (double)plane_tol);
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "cpt_reproject_accum: cpt_set_scene first");
    Frame& f = c->frame;
    if (!f.set || c->n_rows != c->height) return fail(c, CPT_ERR_STATE, "cpt_reproject_accum: needs a full frame");
    for (int y = 0; y < c->height; ++y)
        if (c->rows_h[y] != y) return fail(c, CPT_ERR_STATE, "cpt_reproject_accum: needs rows 0..height-1 in order");
    CPT_REFUSE_PENDING(c, "cpt_reproject_accum");
    for (const cpt_camera* cam : {from, to})
        if (cam->width != c->width || cam->height != c->height)
            return fail(c, CPT_ERR_INVALID_ARG, "cpt_reproject_accum: camera %dx%d vs frame %dx%d", cam->width, cam->height, c->width,
                        c->height);
    if (n_tiles(c) > (size_t)(UINT32_MAX / 64))
        return fail(c, CPT_ERR_UNSUPPORTED, "cpt_reproject_accum: frame of %zu 8x8 tiles (max %u)", n_tiles(c), UINT32_MAX / 64);
    HIP_TRY(c, hipSetDevice(c->device));
    GBufferState& g = f.gbuffer;
    ReprojectState& r = f.reproject;
    const size_t npix = c->npix();
    int rc;
    if ((rc = g.d_id.ensure(c, npix)) != CPT_OK || (rc = g.d_t.ensure(c, npix)) != CPT_OK ||
        (rc = g.d_normal.ensure(c, 3 * npix)) != CPT_OK || (rc = g.d_albedo.ensure(c, 3 * npix)) != CPT_OK ||
        (rc = r.d_id.ensure(c, npix)) != CPT_OK || (rc = r.d_t.ensure(c, npix)) != CPT_OK ||
        (rc = r.d_accum.ensure(c, npix)) != CPT_OK)
        return rc;
    // the G-buffer at `from` into the history planes (its normals pass through the frame's normal
    // plane, which the second trace overwrites), then the G-buffer at `to` into the frame's own
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
    HIP_TRY(c, hipEventRecord(c->t_reproject.t0, s));
    HIP_TRY(c, cpt::launch_ray_query(p0, c->d_rank_obj, nullptr, cpt::QueryPixels{-1, -1},
                                     cpt::QueryOut{r.d_id, r.d_t, g.d_normal, nullptr}, s));
    HIP_TRY(c, hipEventRecord(c->ev_reproject[0], s));
    HIP_TRY(c, cpt::launch_ray_query(p1, c->d_rank_obj, nullptr, cpt::QueryPixels{-1, -1},
                                     cpt::QueryOut{g.d_id, g.d_t, g.d_normal, g.d_albedo}, s));
    g.valid = true;
    HIP_TRY(c, hipEventRecord(c->ev_reproject[1], s));
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

int cpt_last_reproject_ms(cpt_ctx* c, float* ms) {
    if (!c || !ms) return CPT_ERR_INVALID_ARG;
    if (!c->t_reproject.recorded) return fail(c, CPT_ERR_STATE, "cpt_last_reproject_ms: no cpt_reproject_accum yet");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(c->t_reproject.t1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->t_reproject.t0, c->t_reproject.t1));
    return CPT_OK;
}

int cpt_last_reproject_launch_ms(cpt_ctx* c, float* ms3) {
    if (!c || !ms3) return CPT_ERR_INVALID_ARG;
    if (!c->t_reproject.recorded) return fail(c, CPT_ERR_STATE, "cpt_last_reproject_launch_ms: no cpt_reproject_accum yet");
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

}  // extern "C"
