// cpt_capi_query.cpp — the C-ABI's first-hit queries (include/cpt.h): cpt_gbuffer,
// its read-out and its checkpoint writer (cpt_write_gbuffer), cpt_trace_rays, cpt_pick and their
// timing.  The kernel is cpt_query.hip's; it reads the scene and the camera and writes only the
// buffers named here.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "cpt_context.hpp"
#include "cpt_query.hpp"

using namespace cpt::ctx;

namespace {

constexpr size_t MAX_RAYS = (size_t)1 << 30;   // the kernel's 32-bit lane index, with room

// The kernel parameters of a query: the scene, the walk of `flags`, the frame's rows, and `cam`
// (nullptr: none, for explicit rays).
void query_params(cpt_ctx* c, const cpt_camera* cam, uint32_t flags, cpt::KParams& p) {
    cpt_camera none;
    std::memset(&none, 0, sizeof(none));
    none.width = none.height = 1;
    fill_params(c, cam ? cam : &none, 0, 0, flags, p);
}

// What cpt_gbuffer and cpt_pick ask before they launch: walk flags only, a scene, a frame, a
// camera of the frame's size.
int pixel_query_ok(cpt_ctx* c, const cpt_camera* cam, uint32_t flags, const char* who) {
    if (int rc = walk_flags_only(c, who, flags)) return rc;
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "%s: cpt_set_scene first", who);
    if (!c->frame.set) return fail(c, CPT_ERR_STATE, "%s: cpt_set_frame first", who);
    if (cam->width != c->width || cam->height != c->height)
        return fail(c, CPT_ERR_INVALID_ARG, "%s: camera %dx%d vs frame %dx%d", who, cam->width, cam->height, c->width, c->height);
    return CPT_OK;
}

// One launch of the query kernel between the timing events.
int timed_query(cpt_ctx* c, const cpt::KParams& p, const cpt::QueryRays* rays, cpt::QueryPixels px, const cpt::QueryOut& out) {
    hipStream_t s = c->stream();
    if (int rc = c->t_query.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_ray_query(p, c->d_rank_obj, rays, px, out, s));
    return c->t_query.end(c, s);
}

}  // namespace

extern "C" {

int cpt_gbuffer(cpt_ctx* c, const cpt_camera* cam, uint32_t flags) {
    if (!c || !cam) return c ? fail(c, CPT_ERR_INVALID_ARG, "cpt_gbuffer: camera is NULL") : CPT_ERR_INVALID_ARG;
    if (int rc = pixel_query_ok(c, cam, flags, "cpt_gbuffer")) return rc;
    CPT_REFUSE_PENDING(c, "cpt_gbuffer");
    if (cpt::ctx::n_tiles(c) > (size_t)(UINT32_MAX / 64))
        return fail(c, CPT_ERR_UNSUPPORTED, "cpt_gbuffer: frame of %zu 8x8 tiles (max %u)", cpt::ctx::n_tiles(c), UINT32_MAX / 64);
    HIP_TRY(c, hipSetDevice(c->device));
    GBufferState& g = c->frame.gbuffer;
    if (int rc = g.ensure(c, c->npix())) return rc;
    cpt::KParams p;
    query_params(c, cam, flags, p);
    const cpt::QueryOut out{g.d_id, g.d_t, g.d_normal, g.d_albedo};
    if (int rc = timed_query(c, p, nullptr, cpt::QueryPixels{-1, -1}, out)) return rc;
    g.valid = true;
    return CPT_OK;
}

int cpt_read_gbuffer(cpt_ctx* c, int32_t* id, float* t, float* normal3, float* albedo3, size_t capacity_pixels) {
    if (!c) return CPT_ERR_INVALID_ARG;
    const GBufferState& g = c->frame.gbuffer;
    if (!c->frame.set || !g.valid) return fail(c, CPT_ERR_STATE, "cpt_read_gbuffer: cpt_gbuffer first");
    const size_t n = c->npix();
    if (capacity_pixels < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_gbuffer: %zu < %zu pixels", capacity_pixels, n);
    if (int rc = sync_checked(c)) return rc;
    int rc = CPT_OK;
    if (id) rc = read_back(c, id, g.d_id, n);
    if (t && rc == CPT_OK) rc = read_back(c, t, g.d_t, n);
    if (normal3 && rc == CPT_OK) rc = read_back(c, normal3, g.d_normal, 3 * n);
    if (albedo3 && rc == CPT_OK) rc = read_back(c, albedo3, g.d_albedo, 3 * n);
    return rc;
}

int cpt_write_gbuffer(cpt_ctx* c, const int32_t* id, const float* t, const float* normal3, const float* albedo3,
                      size_t count_pixels) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set) return fail(c, CPT_ERR_STATE, "cpt_write_gbuffer: no frame");
    const size_t n = c->npix();
    if (count_pixels < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_write_gbuffer: %zu < %zu pixels", count_pixels, n);
    if (int rc = drain(c)) return rc;
    GBufferState& g = c->frame.gbuffer;
    const size_t had[4] = {g.d_id.capacity(), g.d_t.capacity(), g.d_normal.capacity(), g.d_albedo.capacity()};
    if (int rc = g.ensure(c, n)) return rc;
    // one row per plane: the caller's array, the device plane, its 4-byte elements per pixel
    const struct { const void* host; void* dev; size_t per_pixel; } planes[4] = {
        {id, g.d_id.get(), 1}, {t, g.d_t.get(), 1}, {normal3, g.d_normal.get(), 3}, {albedo3, g.d_albedo.get(), 3}};
    if (n) {
        for (int k = 0; k < 4; ++k) {
            const size_t count = planes[k].per_pixel * n;
            // a plane that was never written starts as zeros: one that is new here (by its capacity
            // before the ensure), or all four when no G-buffer is valid yet
            const bool fresh = !g.valid || had[k] < count;
            if (planes[k].host) HIP_TRY(c, hipMemcpy(planes[k].dev, planes[k].host, count * 4, hipMemcpyHostToDevice));
            else if (fresh) HIP_TRY(c, hipMemsetAsync(planes[k].dev, 0, count * 4, c->stream()));
        }
        HIP_TRY(c, hipStreamSynchronize(c->stream()));   // the fills: a later copy into the plane must not race them
    }
    g.valid = true;
    return CPT_OK;
}

int cpt_trace_rays(cpt_ctx* c, size_t n, const float* origin3, const float* dir3, const float* tmin, uint32_t flags,
                   int32_t* id, float* t, float* normal3) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (int rc = walk_flags_only(c, "cpt_trace_rays", flags)) return rc;
    if (n > MAX_RAYS) return fail(c, CPT_ERR_INVALID_ARG, "cpt_trace_rays: %zu rays (max %zu)", n, MAX_RAYS);
    if (n > 0 && (!origin3 || !dir3 || !id || !t || !normal3))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_trace_rays: origin3, dir3, id, t and normal3 must not be NULL");
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "cpt_trace_rays: cpt_set_scene first");
    if (n == 0) return CPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    // all device memory before the first copy: nothing is allocated between the launch and the read-back
    if (int rc = ensure_all(c, c->d_query_rays, 7 * n, c->d_query_out, 4 * n, c->d_query_id, n)) return rc;
    hipStream_t s = c->stream();
    float* const d_o = c->d_query_rays;
    float* const d_d = d_o + 3 * n;
    float* const d_tmin = d_d + 3 * n;
    float* const d_t = c->d_query_out;
    float* const d_n = d_t + n;
    HIP_TRY(c, hipMemcpyAsync(d_o, origin3, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(d_d, dir3, 3 * n * sizeof(float), hipMemcpyHostToDevice, s));
    if (tmin) HIP_TRY(c, hipMemcpyAsync(d_tmin, tmin, n * sizeof(float), hipMemcpyHostToDevice, s));
    cpt::KParams p;
    query_params(c, nullptr, flags, p);
    const cpt::QueryRays rays{d_o, d_d, tmin ? d_tmin : nullptr, (uint32_t)n};
    const cpt::QueryOut out{c->d_query_id, d_t, d_n, nullptr};
    if (int rc = timed_query(c, p, &rays, cpt::QueryPixels{-1, -1}, out)) return rc;
    HIP_TRY(c, hipMemcpyAsync(id, c->d_query_id, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(t, d_t, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(normal3, d_n, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s));
    return sync_checked(c);
}

int cpt_pick(cpt_ctx* c, const cpt_camera* cam, int x, int y, uint32_t flags, int32_t* object, float* t) {
    if (!c || !cam || !object)
        return c ? fail(c, CPT_ERR_INVALID_ARG, "cpt_pick: camera and object must not be NULL") : CPT_ERR_INVALID_ARG;
    if (int rc = pixel_query_ok(c, cam, flags, "cpt_pick")) return rc;
    if (x < 0 || x >= c->width || y < 0 || y >= c->height)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_pick: pixel (%d, %d) outside the %dx%d frame", x, y, c->width, c->height);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure_all(c, c->d_query_out, 4, c->d_query_id, 1)) return rc;
    cpt::KParams p;
    query_params(c, cam, flags, p);
    float* const d_t = c->d_query_out;
    const cpt::QueryOut out{c->d_query_id, d_t, d_t + 1, nullptr};
    if (int rc = timed_query(c, p, nullptr, cpt::QueryPixels{x, y}, out)) return rc;
    hipStream_t s = c->stream();
    int32_t h_id = -1;
    float h_t = 0.f;
    HIP_TRY(c, hipMemcpyAsync(&h_id, c->d_query_id, sizeof(h_id), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(&h_t, d_t, sizeof(h_t), hipMemcpyDeviceToHost, s));
    if (int rc = sync_checked(c)) return rc;
    *object = h_id;
    if (t) *t = h_t;
    return CPT_OK;
}

int cpt_last_query_ms(cpt_ctx* c, float* ms) {
    return last_span_ms(c, &cpt_ctx::t_query, ms, "cpt_last_query_ms: no query yet");
}

}  // extern "C"
