// cpt_capi_probes.cpp — the C-ABI's diagnostic entry points: the math batch, the read-bandwidth
// probes, the device self-tests, the timeline and node-memory readouts and the host-only cap-disk
// bound.  Their temporaries are local owners, so every early return releases them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cpt_context.hpp"

using namespace cpt::ctx;

// `iters` launches of a read probe between two events on the context's stream, after an untimed
// warm-up launch if asked for; the rate of `bytes_per_iter` each, in GB/s.
template <typename Launch>
static int timed_reads(cpt_ctx* c, bool warm_up, int iters, double bytes_per_iter, float* gbps, Launch launch) {
    hipStream_t s = c->stream();
    DevEvent e0, e1;
    HIP_TRY(c, e0.create());
    HIP_TRY(c, e1.create());
    if (warm_up) HIP_TRY(c, launch());
    HIP_TRY(c, hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i) HIP_TRY(c, launch());
    HIP_TRY(c, hipEventRecord(e1, s));
    HIP_TRY(c, hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, e0, e1));
    *gbps = (float)(bytes_per_iter * iters / (ms * 1e-3) / 1e9);
    return CPT_OK;
}

extern "C" {

int cpt_debug_timeline(cpt_ctx* c, uint64_t* out, int n) {
    if (!c || !out || n <= 0) return CPT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const hipError_t e = cpt::timeline_read(reinterpret_cast<unsigned long long*>(out), n, c->stream());
    if (e == hipErrorNotSupported) return fail(c, CPT_ERR_STATE, "cpt_debug_timeline: not a CPT_TIMELINE build");
    if (e != hipSuccess) return fail(c, CPT_ERR_HIP, "cpt_debug_timeline: %s", hipGetErrorString(e));
    return CPT_OK;
}

int cpt_debug_read_nodes(cpt_ctx* c, void* out, size_t capacity_bytes, size_t* n_bytes) {
    if (!c || !n_bytes) return CPT_ERR_INVALID_ARG;
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "cpt_debug_read_nodes: cpt_set_scene first");
    const size_t bytes = c->lin.size() * sizeof(cpt::Node);   // what upload_scene copied: every order in use
    *n_bytes = bytes;
    if (!out || bytes == 0) return CPT_OK;
    if (capacity_bytes < bytes)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_debug_read_nodes: %zu < %zu bytes", capacity_bytes, bytes);
    if (int rc = sync_checked(c)) return rc;
    return read_back(c, out, c->d_nodes, c->lin.size());
}

int cpt_debug_read_tile_order(cpt_ctx* c, int which, uint32_t* out, size_t capacity, size_t* n) {
    if (!c || !out || !n) return CPT_ERR_INVALID_ARG;
    if (which != CPT_TILE_ORDER_TOPUP && (which < 0 || which > 2))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_debug_read_tile_order: which %d (0..2, %d)", which, CPT_TILE_ORDER_TOPUP);
    const Frame& f = c->frame;
    const uint32_t* src = nullptr;   // stays null for the pending round's list without an order: 0, 1, 2, ...
    size_t len = n_tiles(c);
    if (which == 0) {
        if (!f.set || !f.schedule.d_cost_order) return fail(c, CPT_ERR_STATE, "cpt_debug_read_tile_order: no cost pilot on this frame");
        src = f.schedule.d_cost_order;
    } else if (which == 1) {
        src = f.schedule.previous_order();
        if (!f.set || !src)
            return fail(c, CPT_ERR_STATE, "cpt_debug_read_tile_order: no CPT_SCHEDULE_PREVIOUS order on this frame");
    } else if (which == CPT_TILE_ORDER_TOPUP) {
        if (!f.set || !f.topup.planned) return fail(c, CPT_ERR_STATE, "cpt_debug_read_tile_order: no cpt_render_to_count on this frame");
        // the active prefix: its length is the plan's device word, read behind the queued call
        src = f.topup.d_order;
        uint32_t active = 0;
        if (int rc = sync_checked(c)) return rc;
        if (int rc = read_back(c, &active, f.topup.d_words, 1)) return rc;
        if (active > len) return fail(c, CPT_ERR_DEVICE, "cpt_debug_read_tile_order: %u of %zu tiles active", active, len);
        len = active;
    } else {
        if (!f.adaptive.pending.on) return fail(c, CPT_ERR_STATE, "cpt_debug_read_tile_order: no adaptive render is pending");
        src = f.adaptive.pending.p.tile_order;
        len = f.adaptive.pending.active;
    }
    *n = len;
    if (capacity < len) return fail(c, CPT_ERR_INVALID_ARG, "cpt_debug_read_tile_order: %zu < %zu tiles", capacity, len);
    HIP_TRY(c, hipSetDevice(c->device));
    if (src && len) HIP_TRY(c, hipMemcpyAsync(out, src, len * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream()));
    HIP_TRY(c, hipStreamSynchronize(c->stream()));
    if (!src)
        for (size_t i = 0; i < len; ++i) out[i] = (uint32_t)i;
    return CPT_OK;
}

int cpt_math_batch(cpt_ctx* c, int op,const float* a, const float* b, float* out, size_t n) {
    if (!c || !a || !b || !out) return CPT_ERR_INVALID_ARG;
    if (n == 0) return CPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> da, db, dout;
    int rc;
    if ((rc = ensure_all(c, da, n, db, n, dout, n)) != CPT_OK) return rc;
    if ((rc = write_in(c, da, a, n)) != CPT_OK || (rc = write_in(c, db, b, n)) != CPT_OK) return rc;
    HIP_TRY(c, cpt::launch_math_batch(op, da, db, dout, n, c->stream()));
    HIP_TRY(c, hipStreamSynchronize(c->stream()));
    return read_back(c, out, dout, n);
}

int cpt_cap_disk_bound(float radius, float* out) {
    if (!out) return CPT_ERR_INVALID_ARG;
    *out = cpt::host::cap_disk_bound(radius);
    return CPT_OK;
}

int cpt_measure_read_bandwidth(cpt_ctx* c, size_t bytes, int iters, float* gbps) {
    if (!c || !gbps || bytes < 16 || iters < 1) return CPT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n = bytes / 16;
    DevBuf<float4> d;
    DevBuf<float> o;
    if (int rc = ensure_all(c, d, n, o, 1)) return rc;
    HIP_TRY(c, hipMemsetAsync(d, 0, n * 16, c->stream()));
    const int grid = 8 * c->grid.cus;   // 8 blocks of 256 lanes per CU, grid-stride
    return timed_reads(c, true, iters, (double)n * 16.0, gbps,
                       [&] { return cpt::launch_stream_read(d, n, o, grid, c->stream()); });
}

int cpt_measure_read_pattern(cpt_ctx* c, int bytes_per_lane, size_t bytes, int iters, float* gbps) {
    if (!c || !gbps || bytes < 64 || iters < 1 || (bytes_per_lane != 4 && bytes_per_lane != 12 && bytes_per_lane != 16))
        return CPT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_lanes = bytes / (size_t)bytes_per_lane;
    DevBuf<uint8_t> d;
    DevBuf<float> o;
    if (int rc = ensure_all(c, d, n_lanes * bytes_per_lane, o, 1)) return rc;
    HIP_TRY(c, hipMemsetAsync(d, 0, n_lanes * bytes_per_lane, c->stream()));
    const float* lanes = reinterpret_cast<const float*>(d.get());
    const int grid = 8 * c->grid.cus;
    return timed_reads(c, false, iters, (double)n_lanes * bytes_per_lane, gbps,
                       [&] { return cpt::launch_read_pattern(bytes_per_lane, lanes, n_lanes, o, grid, c->stream()); });
}

int cpt_selftest_qdiv(cpt_ctx* c, int which, uint64_t n, uint64_t seed, uint64_t* out, int out_len) {
    if (!c || !out || out_len < 1 || which < 0 || which > 18) return CPT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<unsigned long long> d;
    if (int rc = d.ensure(c, (size_t)out_len)) return rc;
    HIP_TRY(c, hipMemsetAsync(d, 0, out_len * sizeof(unsigned long long), c->stream()));
    HIP_TRY(c, cpt::launch_selftest_qdiv(which, n, seed, d, out_len, c->stream()));
    HIP_TRY(c, hipStreamSynchronize(c->stream()));
    return read_back(c, out, d, (size_t)out_len);
}

}  // extern "C"
