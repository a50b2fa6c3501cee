// cpt_capi.cpp — implementation of the C-ABI in include/cpt.h: contexts, frames, the RNG init,
// the accumulator / aux / RNG transfers and the counters.  The render launches, their tile
// schedules and timing are cpt_capi_render.cpp, the adaptive render cpt_capi_adaptive.cpp, the
// a-trous filter cpt_capi_filter.cpp, the row-tile gather cpt_capi_gather.cpp, the display path
// cpt_capi_display.cpp, the first-hit queries cpt_capi_query.cpp, the reprojection
// cpt_capi_reproject.cpp, the top-up render cpt_capi_topup.cpp, presenting cpt_capi_present.cpp,
// the diagnostic probes and self-tests cpt_capi_probes.cpp.  The scene half (upload, material
// slots, walk trees, device refit) is cpt_scene.cpp; the host BVH builds and the XORWOW tables are
// cpt_host_bvh.cpp / cpt_host_rng.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "cpt_context.hpp"

static_assert(sizeof(cpt_material) == 40, "cpt_material must match Material (40 B)");
static_assert(sizeof(cpt_object) == 72, "cpt_object must match Object (72 B)");
static_assert(sizeof(cpt_camera) == 136, "cpt_camera must match MotionalCamera (136 B)");
static_assert(offsetof(cpt_object, center) == 48, "Object::center_ offset");
static_assert(offsetof(cpt_material, refractive_index) == 24, "Material::refractive_index_ offset");

using namespace cpt::host;
using namespace cpt::ctx;

namespace {
std::string g_create_error;
}  // namespace

namespace cpt {
namespace ctx {

int fail(cpt_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

int require_full_frame(cpt_ctx* c, const char* who) {
    if (!c->frame.set || c->n_rows != c->height) return fail(c, CPT_ERR_STATE, "%s: needs a full frame", who);
    for (int y = 0; y < c->height; ++y)
        if (c->rows_h[y] != y) return fail(c, CPT_ERR_STATE, "%s: needs rows 0..height-1 in order", who);
    return CPT_OK;
}

int last_span_ms(cpt_ctx* c, TimedSpan cpt_ctx::*span, float* ms, const char* nothing_yet) {
    if (!c || !ms) return CPT_ERR_INVALID_ARG;
    const TimedSpan& t = c->*span;
    if (!t.recorded) return fail(c, CPT_ERR_STATE, "%s", nothing_yet);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventSynchronize(t.t1));
    HIP_TRY(c, hipEventElapsedTime(ms, t.t0, t.t1));
    return CPT_OK;
}

// The kernels' sticky error word (KParams::error, CPT_DEVERR_*): read after the context's
// stream has drained; a set word is cleared and reported once, like a sticky HIP error.
// Both the read and the clear run on the context's own stream (a blocking hipMemcpy would
// synchronise with the legacy default stream and so with other streams' work, e.g. collectives).
int check_device_error(cpt_ctx* c) {
    uint32_t v = 0;
    hipStream_t s = c->stream();
    HIP_TRY(c, hipMemcpyAsync(&v, c->d_work + 4, sizeof(v), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (v == 0) return CPT_OK;
    HIP_TRY(c, hipMemsetAsync(c->d_work + 4, 0, sizeof(v), s));
    return fail(c, CPT_ERR_DEVICE, "device error 0x%x:%s%s%s", v,
                (v & cpt::CPT_DEVERR_KEEPER_TIMEOUT) ? " a keeper wave gave up with chains still live (pixels left unfinished);" : "",
                (v & cpt::CPT_DEVERR_PUBLISH_TIMEOUT) ? " a handed-over chain was never published (its pixel was not written);" : "",
                (v & cpt::CPT_DEVERR_RESUME_CAP) ? " the consolidation slab is too small for the grid;" : "");
}

// Drain the context's stream, then report a device-side error of the work it ran.
int sync_checked(cpt_ctx* c) {
    if (int rc = drain(c)) return rc;
    return check_device_error(c);
}

// A device-to-device copy from one of the context's buffers, ordered against the caller's stream
// without a host wait: the context's stream waits for the work queued on `caller` so far (a fill
// of dst, a collective still reading it), copies, and `caller` waits for the copy (the collective
// queued next reads the copied bytes).  Nothing to order when caller is the context's stream.
int copy_ordered(cpt_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t caller) {
    HIP_TRY(c, hipSetDevice(c->device));
    const bool other = caller != c->stream();
    if (other) {
        HIP_TRY(c, hipEventRecord(c->ev_caller, caller));
        HIP_TRY(c, hipStreamWaitEvent(c->stream(), c->ev_caller, 0));
    }
    if (bytes) HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream()));
    if (other) {
        HIP_TRY(c, hipEventRecord(c->ev_copied, c->stream()));
        HIP_TRY(c, hipStreamWaitEvent(caller, c->ev_copied, 0));
    }
    return CPT_OK;
}

}  // namespace ctx
}  // namespace cpt

extern "C" {

int cpt_abi_version(void) { return CPT_ABI_VERSION; }

const char* cpt_status_string(int status) {
    switch (status) {
        case CPT_OK: return "ok";
        case CPT_ERR_INVALID_ARG: return "invalid argument";
        case CPT_ERR_NO_DEVICE: return "no HIP device";
        case CPT_ERR_HIP: return "HIP runtime error";
        case CPT_ERR_OUT_OF_MEMORY: return "out of device memory";
        case CPT_ERR_STATE: return "invalid state";
        case CPT_ERR_UNSUPPORTED: return "unsupported";
        case CPT_ERR_DEVICE: return "device-side error";
        default: return "unknown status";
    }
}

int cpt_get_device_count(int* count) {
    if (!count) return CPT_ERR_INVALID_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    *count = (e == hipSuccess) ? n : 0;
    return CPT_OK;
}

int cpt_create(int device, cpt_ctx** out) {
    if (!out) return fail(nullptr, CPT_ERR_INVALID_ARG, "cpt_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return fail(nullptr, CPT_ERR_NO_DEVICE, "cpt_create: no HIP device visible");
    if (device < 0 || device >= n) return fail(nullptr, CPT_ERR_INVALID_ARG, "cpt_create: device %d of %d", device, n);
    cpt_ctx* c = new (std::nothrow) cpt_ctx;
    if (!c) return fail(nullptr, CPT_ERR_OUT_OF_MEMORY, "cpt_create: host allocation failed");
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&c->grid.cus, hipDeviceAttributeMultiprocessorCount, device);
    c->grid.cus = std::max(c->grid.cus, 1);
    if (e == hipSuccess) e = c->own_stream.create(hipStreamNonBlocking);
    for (TimedSpan* t : {&c->t_render, &c->t_display, &c->t_filter, &c->t_query, &c->t_reproject, &c->t_present, &c->t_aa, &c->t_bloom})
        if (e == hipSuccess) e = t->create();
    for (DevEvent* ev : {&c->ev_main, &c->ev_reproject[0], &c->ev_reproject[1]})   // the points inside two of the spans
        if (e == hipSuccess) e = ev->create();
    for (DevEvent* ev : {&c->ev_ready, &c->ev_gathered, &c->ev_caller, &c->ev_copied, &c->ev_round, &c->ev_switch})
        if (e == hipSuccess) e = ev->create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->h_ad_words.alloc(4);
    if (e == hipSuccess) e = c->d_stats.alloc(128);   // [64..128) execdiag
    if (e == hipSuccess) e = c->d_work.alloc(16);     // 64 B: [0] dequeue counter, [4] error word
    if (e == hipSuccess) e = hipMemset(c->d_work, 0, 64);
    if (e == hipSuccess) e = hipMemset(c->d_stats, 0, 128 * sizeof(unsigned long long));
    if (e == hipSuccess) {
        const std::vector<uint32_t>& J = jump_tables();
        e = c->d_jumps.alloc(J.size());
        if (e == hipSuccess) e = hipMemcpy(c->d_jumps, J.data(), J.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        int rc = fail(nullptr, CPT_ERR_HIP, "cpt_create: %s", hipGetErrorString(e));
        cpt_destroy(c);
        return rc;
    }
    *out = c;
    return CPT_OK;
}

// What the context owns is released by its members' destructors (the stream last); only the
// order of the waits is spelled out.
int cpt_destroy(cpt_ctx* c) {
    if (!c) return CPT_OK;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    if (c->user_stream) (void)hipStreamSynchronize(c->user_stream);
    delete c;
    return CPT_OK;
}

const char* cpt_last_error(const cpt_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int cpt_set_stream(cpt_ctx* c, void* s) {
    if (!c) return CPT_ERR_INVALID_ARG;
    const hipStream_t before = c->stream();
    c->user_stream = (hipStream_t)s;
    const hipStream_t after = c->stream();
    if (after == before) return CPT_OK;
    // The context's buffers (accumulator, RNG planes, the dequeue and error words of d_work) have one
    // writer at a time only while its work runs in the order of the calls: what is queued on the
    // stream being left runs before anything queued on the new one from here on, by an event, with
    // no host wait (as copy_ordered).  sync_checked drains the new stream alone, and that now
    // includes the wait for this event.
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventRecord(c->ev_switch, before));
    HIP_TRY(c, hipStreamWaitEvent(after, c->ev_switch, 0));
    return CPT_OK;
}

// MotionalCamera::GetCopy (motional_camera.cu:177-200)
int cpt_camera_get_copy(cpt_camera* cam) {
    if (!cam || cam->width <= 0 || cam->height <= 0) return CPT_ERR_INVALID_ARG;
    auto sub = [](cpt_float3 a, cpt_float3 b) { return cpt_float3{a.x - b.x, a.y - b.y, a.z - b.z}; };
    auto add = [](cpt_float3 a, cpt_float3 b) { return cpt_float3{a.x + b.x, a.y + b.y, a.z + b.z}; };
    auto scale = [](float s, cpt_float3 a) { return cpt_float3{s * a.x, s * a.y, s * a.z}; };
    auto dot = [](cpt_float3 a, cpt_float3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; };
    auto normalize = [&](cpt_float3 v) {
        float inv = 1.0f / sqrtf(dot(v, v));
        return cpt_float3{v.x * inv, v.y * inv, v.z * inv};
    };
    auto cross = [](cpt_float3 a, cpt_float3 b) {
        return cpt_float3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
    };
    float theta = (float)((double)cam->view_fov * 3.14159265358979323846 / 180);
    float aspect = float(cam->width) / float(cam->height);
    float half_height = tanf(theta / 2);
    float half_width = aspect * half_height;
    cam->w = normalize(sub(cam->origin, cam->look_at));
    cam->u = normalize(cross(cam->vup, cam->w));
    cam->v = cross(cam->w, cam->u);
    cpt_float3 ol = sub(cam->origin, cam->look_at);
    cam->dist_to_focus = sqrtf(dot(ol, ol));
    float d = cam->dist_to_focus;
    cam->top_left_corner = sub(add(sub(cam->origin, scale(half_width * d, cam->u)), scale(half_height * d, cam->v)),
                               scale(d, cam->w));
    cam->horizontal = scale(2 * half_width * d, cam->u);
    cam->vertical = scale(-2 * half_height * d, cam->v);
    cam->cur_sample_idx++;
    return CPT_OK;
}

int cpt_set_frame(cpt_ctx* c, int width, int height, const int32_t* rows, int n_rows) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (width <= 0 || height <= 0) return fail(c, CPT_ERR_INVALID_ARG, "cpt_set_frame: %dx%d", width, height);
    // the megakernel keeps a lane's pixel as 16-bit x / y and a 32-bit index
    if (width > 65535 || height > 65535)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_set_frame: %dx%d exceeds 65535 pixels per axis", width, height);
    CPT_REFUSE_PENDING(c, "cpt_set_frame");
    std::vector<int32_t> r;
    if (rows) {
        if (n_rows < 0) return fail(c, CPT_ERR_INVALID_ARG, "cpt_set_frame: n_rows %d", n_rows);
        r.assign(rows, rows + n_rows);
        for (int32_t y : r)
            if (y < 0 || y >= height) return fail(c, CPT_ERR_INVALID_ARG, "cpt_set_frame: row %d outside [0,%d)", y, height);
    } else {
        r.resize(height);
        for (int y = 0; y < height; ++y) r[y] = y;
    }
    if (int rc = drain(c)) return rc;
    // releases everything the previous frame held; with it goes the captured history of the tracked
    // reprojection (ReprojectState: planes of the old size, the motion table and its events)
    c->frame = Frame{};
    Frame& f = c->frame;
    static std::atomic<uint64_t> frame_gens{0};
    c->frame_gen = ++frame_gens;
    c->width = width;
    c->height = height;
    c->n_rows = (int)r.size();
    c->rows_h = r;
    const size_t npix = c->npix();
    if (c->n_rows > 0) {
        if (int rc = f.d_rows.ensure(c, r.size())) return rc;
        if (int rc = write_in(c, f.d_rows, r.data(), r.size())) return rc;
        if (int rc = ensure_all(c, f.d_rng, 6 * npix, f.d_accum, npix)) return rc;
        // on the context's stream, and waited for: a device hipMemset returns before the fill has
        // run and is ordered on the null stream only, which the context's non-blocking stream does
        // not wait for; on a busy GPU the fill could land after cpt_init_rng's kernel or a render
        HIP_TRY(c, hipMemsetAsync(f.d_accum, 0, npix * sizeof(float4), c->stream()));
        HIP_TRY(c, hipMemsetAsync(f.d_rng, 0, 6 * npix * sizeof(uint32_t), c->stream()));
        HIP_TRY(c, hipStreamSynchronize(c->stream()));
    }
    f.set = true;
    return CPT_OK;
}

int cpt_init_rng(cpt_ctx* c, uint64_t seed) {
    if (!c) return CPT_ERR_INVALID_ARG;
    Frame& f = c->frame;
    if (!f.set) return fail(c, CPT_ERR_STATE, "cpt_init_rng: cpt_set_frame first");
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->n_rows == 0) { f.rng_set = true; return CPT_OK; }
    if (int rc = ensure_all(c, f.d_scratch_w, 5 * (size_t)c->width, f.d_scratch_m, (size_t)c->n_rows * 800)) return rc;
    f.schedule.rng_replaced();
    uint32_t st[6];
    curand_seed_state(seed, st);
    HIP_TRY(c, cpt::launch_init_rng(c->d_jumps, st, c->width, f.d_rows, c->n_rows, f.d_scratch_w, f.d_scratch_m,
                                   f.d_rng, c->stream()));
    HIP_TRY(c, hipStreamSynchronize(c->stream()));
    // the scratch matrices are n_rows * 3.2 KB; release them (one-time init)
    f.d_scratch_m.reset();
    f.d_scratch_w.reset();
    f.rng_set = true;
    return CPT_OK;
}

int cpt_read_rng(cpt_ctx* c, uint32_t* planar6) {
    if (!c || !planar6) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set) return fail(c, CPT_ERR_STATE, "cpt_read_rng: no frame");
    if (int rc = sync_checked(c)) return rc;
    return read_back(c, planar6, c->frame.d_rng, 6 * c->npix());
}

int cpt_write_rng(cpt_ctx* c, const uint32_t* planar6) {
    if (!c || !planar6) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set) return fail(c, CPT_ERR_STATE, "cpt_write_rng: no frame");
    if (int rc = drain(c)) return rc;
    if (int rc = write_in(c, c->frame.d_rng, planar6, 6 * c->npix())) return rc;
    c->frame.rng_set = true;
    c->frame.schedule.draws_moved();
    return CPT_OK;
}

int cpt_synchronize(cpt_ctx* c) {
    if (!c) return CPT_ERR_INVALID_ARG;
    return sync_checked(c);
}

int cpt_read_accum(cpt_ctx* c, float* rgba) {
    if (!c || !rgba) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set) return fail(c, CPT_ERR_STATE, "cpt_read_accum: no frame");
    if (int rc = sync_checked(c)) return rc;
    return read_back(c, rgba, c->frame.d_accum, c->npix());
}

int cpt_clear_accum(cpt_ctx* c) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set) return fail(c, CPT_ERR_STATE, "cpt_clear_accum: no frame");
    HIP_TRY(c, hipSetDevice(c->device));
    size_t n = c->npix();
    if (n) HIP_TRY(c, hipMemsetAsync(c->frame.d_accum, 0, n * sizeof(float4), c->stream()));
    return CPT_OK;
}

int cpt_read_aux(cpt_ctx* c, float* normal3, float* depth) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!c->frame.d_normal || !c->frame.d_depth) return fail(c, CPT_ERR_STATE, "cpt_read_aux: render with CPT_RENDER_AUX first");
    if (int rc = drain(c)) return rc;
    const size_t n = c->npix();
    if (normal3)
        if (int rc = read_back(c, normal3, c->frame.d_normal, 3 * n)) return rc;
    return depth ? read_back(c, depth, c->frame.d_depth, n) : CPT_OK;
}

// Checkpoint / resume: the accumulator and the first-hit aux buffers restored
// from host copies (with cpt_write_rng, a render resumes bit for bit where it stopped).
int cpt_write_accum(cpt_ctx* c, const float* rgba) {
    if (!c || !rgba) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set) return fail(c, CPT_ERR_STATE, "cpt_write_accum: no frame");
    if (int rc = drain(c)) return rc;
    return write_in(c, c->frame.d_accum, rgba, c->npix());
}

int cpt_write_aux(cpt_ctx* c, const float* normal3, const float* depth) {
    if (!c || !normal3 || !depth) return CPT_ERR_INVALID_ARG;
    Frame& f = c->frame;
    if (!f.set) return fail(c, CPT_ERR_STATE, "cpt_write_aux: no frame");
    if (int rc = drain(c)) return rc;
    const size_t n = c->npix();
    if (int rc = f.ensure_aux(c, n)) return rc;
    if (int rc = write_in(c, f.d_normal, normal3, 3 * n)) return rc;
    return write_in(c, f.d_depth, depth, n);
}

int cpt_copy_accum_device(cpt_ctx* c, void* dst, size_t bytes, void* caller_stream) {
    if (!c || (!dst && bytes)) return CPT_ERR_INVALID_ARG;
    size_t have = c->npix() * sizeof(float4);
    if (bytes > have) return fail(c, CPT_ERR_INVALID_ARG, "cpt_copy_accum_device: %zu > %zu bytes", bytes, have);
    return copy_ordered(c, dst, c->frame.d_accum, bytes, (hipStream_t)caller_stream);
}

// `count` of the context's 64-bit counters from `first` on, once its stream has drained.
static int read_counters(cpt_ctx* c, void* out, int first, int count) {
    if (!c || !out) return CPT_ERR_INVALID_ARG;
    if (int rc = drain(c)) return rc;
    return read_back(c, out, c->d_stats, (size_t)count, (size_t)first);
}

int cpt_get_stats(cpt_ctx* c, cpt_stats* out) {
    unsigned long long h[8];
    if (int rc = read_counters(c, out ? h : nullptr, 0, 8)) return rc;
    out->segments = h[0];
    out->node_visits = h[1];
    out->prim_tests = h[2];
    out->hits = h[3];
    out->misses = h[4];
    return CPT_OK;
}

int cpt_get_raw_counters(cpt_ctx* c, uint64_t* out8) { return read_counters(c, out8, 0, 8); }
int cpt_get_diag_counters(cpt_ctx* c, uint64_t* out16) { return read_counters(c, out16, 16, 16); }
int cpt_get_execdiag_counters(cpt_ctx* c, uint64_t* out64) { return read_counters(c, out64, 64, 64); }

int cpt_get_walk_info(cpt_ctx* c, int32_t* out4) {
    if (!c || !out4) return CPT_ERR_INVALID_ARG;
    out4[0] = c->n_bvh;
    out4[1] = c->n_walk;
    out4[2] = c->n_wide;
    out4[3] = c->n_unb;
    return CPT_OK;
}

int cpt_reset_stats(cpt_ctx* c) {
    if (!c) return CPT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->d_stats, 0, 128 * sizeof(unsigned long long), c->stream()));
    return CPT_OK;
}

}  // extern "C"
