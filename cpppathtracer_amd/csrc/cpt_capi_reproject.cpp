// cpt_capi_reproject.cpp — the C-ABI's reprojection of the accumulated frame (include/cpt.h,
// cpt_reproject_accum) and of the display state (§22: cpt_reproject_display) to a
// moved camera, the tracked variants that keep the history's G-buffer and follow object edits
// (§23: cpt_history_capture, cpt_reproject_accum_tracked, cpt_reproject_display_tracked), their
// timing, and the host-only entries on the same arithmetic.  The four device calls are one function,
// `reproject`, the four host entries one, `reproject_host`.  The G-buffers are cpt_query.hip's
// kernel, the look-up cpt_reproject.hip's; the arithmetic is cpt_reproject.hpp's on both sides.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <type_traits>
#include <utility>

#include "cpt_context.hpp"
#include "cpt_query.hpp"
#include "cpt_reproject.hpp"

using namespace cpt::ctx;
namespace rp = cpt::reproject;

namespace {

bool args_ok(int max_history, float plane_tol) { return max_history >= 1 && rp::finite(plane_tol) && plane_tol >= 0.f; }

// What every device call here (`who`) asks before it writes anything.
int checked(cpt_ctx* c, const char* who, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
            uint32_t flags) {
    if (!from || !to) return fail(c, CPT_ERR_INVALID_ARG, "%s: a camera is NULL", who);
    if (int rc = walk_flags_only(c, who, flags)) return rc;
    if (!args_ok(max_history, plane_tol))
        return fail(c, CPT_ERR_INVALID_ARG, "%s: max_history %d (>= 1), plane_tol %g (finite, >= 0)", who, max_history,
                    (double)plane_tol);
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "%s: cpt_set_scene first", who);
    if (int rc = require_full_frame(c, who)) return rc;
    CPT_REFUSE_PENDING(c, who);
    for (const cpt_camera* cam : {from, to})
        if (cam->width != c->width || cam->height != c->height)
            return fail(c, CPT_ERR_INVALID_ARG, "%s: camera %dx%d vs frame %dx%d", who, cam->width, cam->height, c->width, c->height);
    if (n_tiles(c) > (size_t)(UINT32_MAX / 64))
        return fail(c, CPT_ERR_UNSUPPORTED, "%s: frame of %zu 8x8 tiles (max %u)", who, n_tiles(c), UINT32_MAX / 64);
    return CPT_OK;
}

// The planes every call traces into: the frame's G-buffer and the history's id and distance.
int ensure_planes(cpt_ctx* c) {
    ReprojectState& r = c->frame.reproject;
    const size_t npix = c->npix();
    if (int rc = c->frame.gbuffer.ensure(c, npix)) return rc;
    return ensure_all(c, r.d_id, npix, r.d_t, npix);
}

// The whole G-buffer at p's camera into the frame's own planes (the kernel writes all four).
int trace_gbuffer(cpt_ctx* c, const cpt::KParams& p, hipStream_t s) {
    GBufferState& g = c->frame.gbuffer;
    HIP_TRY(c, cpt::launch_ray_query(p, c->d_rank_obj, nullptr, cpt::QueryPixels{-1, -1},
                                     cpt::QueryOut{g.d_id, g.d_t, g.d_normal, g.d_albedo}, s));
    g.valid = true;
    return CPT_OK;
}

// The traces, with the call's first three timing events: the G-buffer at `from` (p0) into the
// history planes (its normals pass through the frame's normal plane, which the second trace
// overwrites), then the G-buffer at `to` (p1) into the frame's own.  p0 == nullptr, the tracked
// calls: no trace at the captured camera (ms3[0] reads 0).
int trace(cpt_ctx* c, const cpt::KParams* p0, const cpt::KParams& p1, hipStream_t s) {
    GBufferState& g = c->frame.gbuffer;
    ReprojectState& r = c->frame.reproject;
    // the trace at `from` overwrites the planes a captured history lives in: it is gone
    if (p0) r.captured = false;
    if (int rc = c->t_reproject.begin(c, s)) return rc;
    if (p0)
        HIP_TRY(c, cpt::launch_ray_query(*p0, c->d_rank_obj, nullptr, cpt::QueryPixels{-1, -1},
                                         cpt::QueryOut{r.d_id, r.d_t, g.d_normal, nullptr}, s));
    HIP_TRY(c, hipEventRecord(c->ev_reproject[0], s));
    if (int rc = trace_gbuffer(c, p1, s)) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_reproject[1], s));
    return CPT_OK;
}

// What the tracked calls ask beyond `checked`, and the planes they need beyond ensure_planes.
int tracked_ready(cpt_ctx* c, const char* who) {
    ReprojectState& r = c->frame.reproject;
    if (!r.captured) return fail(c, CPT_ERR_STATE, "%s: no captured history (cpt_history_capture first)", who);
    if (int rc = ensure_planes(c)) return rc;
    return ensure_all(c, r.d_id_next, c->npix(), r.d_t_next, c->npix());
}

// The motion table of the objects since the capture, uploaded on the stream; *table stays nullptr
// when no object was edited (nothing is derived or uploaded then).
int motion_table(cpt_ctx* c, hipStream_t s, const cpt_object_motion** table) {
    ReprojectState& r = c->frame.reproject;
    *table = nullptr;
    const size_t n = c->objs.size();
    if (r.objs.size() != n) return fail(c, CPT_ERR_STATE, "the captured history holds %zu objects, the scene %zu", r.objs.size(), n);
    bool edited = false;
    for (size_t k = 0; k < n && !edited; ++k)
        edited = !rp::same_geometry(r.objs[k], c->objs[k]) || !rp::same_material(r.objs[k].material, c->objs[k].material);
    if (!edited) return CPT_OK;
    // two host tables by turns: an upload reads its table until its event, so this call waits only
    // for the upload of the call before the last, which has long retired unless three edited calls
    // are queued behind one unfinished render
    const int b = r.motion_turn ^= 1;
    if (!r.ev_motion[b]) HIP_TRY(c, r.ev_motion[b].create(hipEventDisableTiming));
    else HIP_TRY(c, hipEventSynchronize(r.ev_motion[b]));
    std::vector<cpt_object_motion>& h = r.motion_h[b];
    try {
        h.resize(n);
    } catch (const std::bad_alloc&) {
        return fail(c, CPT_ERR_OUT_OF_MEMORY, "motion table: host allocation failed");
    }
    for (size_t k = 0; k < n; ++k) h[k] = rp::motion_of(r.objs[k], c->objs[k]);
    if (int rc = r.d_motion.ensure(c, n)) return rc;
    HIP_TRY(c, hipMemcpyAsync(r.d_motion, h.data(), n * sizeof(cpt_object_motion), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipEventRecord(r.ev_motion[b], s));
    *table = r.d_motion;
    return CPT_OK;
}

// Behind a tracked look-up: `to`, its id and distance planes (the kernel wrote them to the second
// planes) and the current objects are the captured history.
void renew_history(cpt_ctx* c, const cpt_camera* to, bool edited) {
    ReprojectState& r = c->frame.reproject;
    std::swap(r.d_id, r.d_id_next);
    std::swap(r.d_t, r.d_t_next);
    r.cam = *to;
    if (edited) r.objs = c->objs;   // same size: assigns in place
}

// The four device calls.  Look: the accumulator's argument struct or the display's; TRACKED: `from`
// is the captured history's camera (the caller gives none) and no trace runs there.
template <typename Look, bool TRACKED>
int reproject(cpt_ctx* c, const char* who, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
              uint32_t flags) {
    constexpr bool DISPLAY = std::is_same_v<Look, cpt::ReprojectDisplayArgs>;
    if (!c) return CPT_ERR_INVALID_ARG;
    if (int rc = checked(c, who, TRACKED ? to : from, to, max_history, plane_tol, flags)) return rc;
    Frame& f = c->frame;
    DisplayBand& d = f.display;
    GBufferState& g = f.gbuffer;
    ReprojectState& r = f.reproject;
    const int w_eff = 16 * (c->width / 16), h_eff = 16 * (c->height / 16);
    if (DISPLAY) {
        if (!d.d_mix) return fail(c, CPT_ERR_STATE, "%s: no display pass yet", who);
        if (d.y0 != 0 || d.y1 != h_eff)
            return fail(c, CPT_ERR_STATE, "%s: the display holds the band [%d, %d), not the full frame", who, d.y0, d.y1);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t npix = c->npix();
    int rc;
    if ((rc = TRACKED ? tracked_ready(c, who) : ensure_planes(c)) != CPT_OK) return rc;
    if ((rc = DISPLAY ? ensure_all(c, d.d_mix_next, 3 * npix, d.d_count_next, npix) : r.d_accum.ensure(c, npix)) != CPT_OK) return rc;
    if (TRACKED) from = &r.cam;
    cpt::KParams p0, p1;
    fill_params(c, from, 0, 0, flags, p0);
    fill_params(c, to, 0, 0, flags, p1);
    std::conditional_t<TRACKED, cpt::ReprojectTracked<Look>, Look> args;
    std::memset(&args, 0, sizeof(args));
    Look& a = cpt::look_of(args);
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
    a.max_history = (float)max_history;
    a.plane_tol = plane_tol;
    if constexpr (DISPLAY) {
        a.w_eff = w_eff;
        a.h_eff = h_eff;
        a.mean_in = d.d_mix;
        a.count_in = d.d_count;
        a.mean_out = d.d_mix_next;
        a.count_out = d.d_count_next;
    } else {
        a.in = f.d_accum;
        a.out = r.d_accum;
    }
    hipStream_t s = c->stream();
    if (DISPLAY && (rc = d.fill_count(c)) != CPT_OK) return rc;
    bool edited = false;
    if constexpr (TRACKED) {
        args.id_next = r.d_id_next;
        args.t_next = r.d_t_next;
        if ((rc = motion_table(c, s, &args.motion)) != CPT_OK) return rc;
        edited = args.motion != nullptr;
    }
    if ((rc = trace(c, TRACKED ? nullptr : &p0, p1, s)) != CPT_OK) return rc;
    HIP_TRY(c, cpt::launch_reproject(args, s));
    if ((rc = c->t_reproject.end(c, s)) != CPT_OK) return rc;
    c->reproject_tracked = TRACKED;
    // the second planes are the accumulator, or the display state, from here on: work already queued
    // holds the old pointers by value and runs before the kernel; every later call reads the members.
    // The display's need no clearing: the kernel wrote every pixel of the frame.
    if (DISPLAY) {
        std::swap(d.d_mix, d.d_mix_next);
        std::swap(d.d_count, d.d_count_next);
    } else {
        std::swap(f.d_accum, r.d_accum);
        f.adaptive.done = false;   // the moments no longer describe the accumulator
    }
    if (TRACKED) renew_history(c, to, edited);
    return CPT_OK;
}

// the tracked host entries' table: NULL with 0 records, or every hit's id inside it
bool table_ok(const cpt_object_motion* table, int n_objs, const int32_t* id1, size_t npix) {
    if (!table) return n_objs == 0;
    if (n_objs <= 0) return false;
    for (size_t i = 0; i < npix; ++i)
        if (id1[i] >= n_objs) return false;
    return true;
}

// The four host entries.  The accumulator's (`in`, `out`: [npix][4]; no count planes) or, DISPLAY,
// the display state's (`in`, `out`: the mean [npix][3]); Motion: rp::NoMotion, or rp::TableMotion
// with the `n_objs` records of its table.
template <bool DISPLAY, typename Motion>
int reproject_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0, const float* dir1,
                   const int32_t* id0, const float* t0, const int32_t* id1, const float* t1, const float* normal1,
                   const float* in, const float* count_in, const Motion& motion, int n_objs, int max_history, float plane_tol,
                   float* out, float* count_out) {
    if (!cam0 || !cam1 || width <= 0 || height <= 0 || !dir0 || !dir1 || !id0 || !t0 || !id1 || !t1 || !normal1 || !in || !out ||
        in == out || (DISPLAY && (!count_in || !count_out || count_in == count_out)) || !args_ok(max_history, plane_tol))
        return CPT_ERR_INVALID_ARG;
    for (const cpt_camera* cam : {cam0, cam1})
        if (cam->width != width || cam->height != height) return CPT_ERR_INVALID_ARG;
    if constexpr (Motion::TRACKED)
        if (!table_ok(motion.table, n_objs, id1, (size_t)width * height)) return CPT_ERR_INVALID_ARG;
    const rp::OldView v = rp::old_view(*cam0);
    const rp::V3 o1 = rp::v3_of(cam1->origin);
    const auto src = [&] {
        if constexpr (DISPLAY) return rp::DisplayPlaneSrc{in, count_in, id0, t0, dir0};
        else return rp::PlaneSrc{reinterpret_cast<const rp::Px*>(in), id0, t0, dir0};
    }();
    const int w_eff = 16 * (width / 16), h_eff = 16 * (height / 16);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const rp::V3 n1{normal1[3 * i], normal1[3 * i + 1], normal1[3 * i + 2]}, d1{dir1[3 * i], dir1[3 * i + 1], dir1[3 * i + 2]};
            if constexpr (DISPLAY) {
                const rp::Px r = rp::display_pixel(src, v, o1, width, height, w_eff, h_eff, x, y, id1[i], t1[i], n1, d1,
                                                   (float)max_history, plane_tol, motion);
                out[3 * i] = r.r;
                out[3 * i + 1] = r.g;
                out[3 * i + 2] = r.b;
                count_out[i] = r.n;
            } else {
                reinterpret_cast<rp::Px*>(out)[i] =
                    rp::pixel<false>(src, v, o1, width, height, id1[i], t1[i], n1, d1, (float)max_history, plane_tol, 0, 0, motion);
            }
        }
    return CPT_OK;
}

}  // namespace

extern "C" {

int cpt_reproject_accum(cpt_ctx* c, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
                        uint32_t flags) {
    return reproject<cpt::ReprojectArgs, false>(c, "cpt_reproject_accum", from, to, max_history, plane_tol, flags);
}

int cpt_reproject_display(cpt_ctx* c, const cpt_camera* from, const cpt_camera* to, int max_history, float plane_tol,
                          uint32_t flags) {
    return reproject<cpt::ReprojectDisplayArgs, false>(c, "cpt_reproject_display", from, to, max_history, plane_tol, flags);
}

int cpt_reproject_accum_tracked(cpt_ctx* c, const cpt_camera* to, int max_history, float plane_tol, uint32_t flags) {
    return reproject<cpt::ReprojectArgs, true>(c, "cpt_reproject_accum_tracked", nullptr, to, max_history, plane_tol, flags);
}

int cpt_reproject_display_tracked(cpt_ctx* c, const cpt_camera* to, int max_history, float plane_tol, uint32_t flags) {
    return reproject<cpt::ReprojectDisplayArgs, true>(c, "cpt_reproject_display_tracked", nullptr, to, max_history, plane_tol,
                                                      flags);
}

int cpt_history_capture(cpt_ctx* c, const cpt_camera* cam, uint32_t flags) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (int rc = checked(c, "cpt_history_capture", cam, cam, 1, 0.f, flags)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    GBufferState& g = c->frame.gbuffer;
    ReprojectState& r = c->frame.reproject;
    if (int rc = ensure_planes(c)) return rc;
    // (from here on an earlier capture is gone, also if a launch below fails: a failed capture
    // leaves no history, not the previous one)
    try {
        r.objs = c->objs;
    } catch (const std::bad_alloc&) {
        return fail(c, CPT_ERR_OUT_OF_MEMORY, "cpt_history_capture: host allocation failed");
    }
    r.captured = false;   // until the planes are queued
    cpt::KParams p;
    fill_params(c, cam, 0, 0, flags, p);
    hipStream_t s = c->stream();
    // the G-buffer at cam, then its id and distance into the history's planes
    if (int rc = trace_gbuffer(c, p, s)) return rc;
    HIP_TRY(c, hipMemcpyAsync(r.d_id, g.d_id, c->npix() * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(r.d_t, g.d_t, c->npix() * sizeof(float), hipMemcpyDeviceToDevice, s));
    r.cam = *cam;
    r.captured = true;
    return CPT_OK;
}

int cpt_history_info(cpt_ctx* c, int* valid, cpt_camera* cam) {
    if (!c || !valid) return CPT_ERR_INVALID_ARG;
    const ReprojectState& r = c->frame.reproject;
    *valid = r.captured ? 1 : 0;
    if (cam && r.captured) *cam = r.cam;
    return CPT_OK;
}

int cpt_last_reproject_ms(cpt_ctx* c, float* ms) {
    return last_span_ms(c, &cpt_ctx::t_reproject, ms,
                        "cpt_last_reproject_ms: no reprojection call (cpt_reproject_accum, _display or their tracked variants) yet");
}

int cpt_last_reproject_launch_ms(cpt_ctx* c, float* ms3) {
    if (!ms3) return CPT_ERR_INVALID_ARG;
    float all;   // read for its checks and its wait for t1
    if (int rc = last_span_ms(c, &cpt_ctx::t_reproject, &all,
                              "cpt_last_reproject_launch_ms: no reprojection call (cpt_reproject_accum, _display or their tracked variants) yet"))
        return rc;
    const hipEvent_t ev[4] = {c->t_reproject.t0, c->ev_reproject[0], c->ev_reproject[1], c->t_reproject.t1};
    for (int k = 0; k < 3; ++k) HIP_TRY(c, hipEventElapsedTime(ms3 + k, ev[k], ev[k + 1]));
    if (c->reproject_tracked) ms3[0] = 0.f;   // no trace ran between the first two events
    return CPT_OK;
}

int cpt_reproject_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                       const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                       const float* normal1, const float* accum_in, int max_history, float plane_tol, float* accum_out) {
    return reproject_host<false>(cam0, cam1, width, height, dir0, dir1, id0, t0, id1, t1, normal1, accum_in, nullptr, rp::NoMotion{},
                                 0, max_history, plane_tol, accum_out, nullptr);
}

int cpt_reproject_display_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                               const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                               const float* normal1, const float* mean_in, const float* count_in, int max_history,
                               float plane_tol, float* mean_out, float* count_out) {
    return reproject_host<true>(cam0, cam1, width, height, dir0, dir1, id0, t0, id1, t1, normal1, mean_in, count_in, rp::NoMotion{},
                                0, max_history, plane_tol, mean_out, count_out);
}

int cpt_object_motion_host(const cpt_object* old_objs, const cpt_object* new_objs, int n, cpt_object_motion* out_table) {
    if (n < 0 || (n > 0 && (!old_objs || !new_objs || !out_table))) return CPT_ERR_INVALID_ARG;
    for (int k = 0; k < n; ++k) out_table[k] = rp::motion_of(old_objs[k], new_objs[k]);
    return CPT_OK;
}

int cpt_reproject_tracked_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height, const float* dir0,
                               const float* dir1, const int32_t* id0, const float* t0, const int32_t* id1, const float* t1,
                               const float* normal1, const float* accum_in, const cpt_object_motion* table, int n_objs,
                               int max_history, float plane_tol, float* accum_out) {
    return reproject_host<false>(cam0, cam1, width, height, dir0, dir1, id0, t0, id1, t1, normal1, accum_in, nullptr,
                                 rp::TableMotion{table}, n_objs, max_history, plane_tol, accum_out, nullptr);
}

int cpt_reproject_display_tracked_host(const cpt_camera* cam0, const cpt_camera* cam1, int width, int height,
                                       const float* dir0, const float* dir1, const int32_t* id0, const float* t0,
                                       const int32_t* id1, const float* t1, const float* normal1, const float* mean_in,
                                       const float* count_in, const cpt_object_motion* table, int n_objs, int max_history,
                                       float plane_tol, float* mean_out, float* count_out) {
    return reproject_host<true>(cam0, cam1, width, height, dir0, dir1, id0, t0, id1, t1, normal1, mean_in, count_in,
                                rp::TableMotion{table}, n_objs, max_history, plane_tol, mean_out, count_out);
}

}  // extern "C"
