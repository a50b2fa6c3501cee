// cpt_capi_adaptive.cpp — the C-ABI's adaptive render (include/cpt.h, DESIGN.md §Adaptive
// sampling): rounds of `batch` passes over the 8x8 tiles that are still noisy, the noise map and
// the round record, and the host-only hook on the criterion.  Each round is the launch cpt_render
// makes (cpt_capi_render.cpp's helpers), over a shorter tile order; the kernels around it are
// cpt_adaptive.hip's.  The render is cpt_adaptive_begin (checks, buffers, the pilot, round 1
// queued) and cpt_adaptive_step (one round's read-back, the next round queued), so that one thread
// can keep a round queued on each of several contexts; cpt_render_adaptive is the two in a loop.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cpt_adaptive.hpp"
#include "cpt_context.hpp"

using namespace cpt::ctx;

namespace {

// One round on the context's stream: cpt_render's launch of `batch` passes over the listed tiles,
// the moments and keep flags, the compaction into the other order buffer, and the read-back of
// {tiles kept, pixels rendered, device error word} into the context's pinned words with an event
// behind it.  No host wait.
int enqueue_round(cpt_ctx* c) {
    Frame& f = c->frame;
    AdaptiveState::Pending& a = f.adaptive.pending;
    hipStream_t s = c->stream();
    ++a.round;
    // round 1 is cpt_render's own launch (every tile, the caller's accumulate flag); later
    // rounds add to what the earlier ones left, over the tiles still listed
    if (a.round > 1) {
        a.p.accumulate = 1;
        a.p.n_active = a.active;
    }
    HIP_TRY(c, cpt::launch_megakernel(a.p, a.stats, a.aux, c->grid, s));
    cpt::AdaptiveRound r{};
    r.order = a.p.tile_order;
    r.n_active = a.active;
    r.width = c->width;
    r.n_rows = c->n_rows;
    r.accum = f.d_accum;
    r.snap = f.adaptive.d_snap;
    r.stat = f.adaptive.d_stat;
    r.keep = f.adaptive.d_keep;
    r.rel_error = a.rel_error;
    r.eligible = (long long)a.round * a.batch >= a.min_spp;
    r.last = a.round >= a.max_rounds;
    HIP_TRY(c, cpt::launch_tile_noise(r, s));
    HIP_TRY(c, cpt::launch_compact_order(a.p.tile_order, f.adaptive.d_keep, a.active, c->width, c->n_rows, f.adaptive.d_order[a.into],
                                         f.adaptive.d_count, s));
    uint32_t* h = c->h_ad_words.raw();
    HIP_TRY(c, hipMemcpyAsync(h, f.adaptive.d_count, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(h + 2, c->d_work + 4, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipEventRecord(c->ev_round, s));
    a.queued = true;
    return CPT_OK;
}

// cpt_adaptive_begin under the name of the call that makes it (the messages of cpt_render_adaptive
// are its own).
int adaptive_begin(cpt_ctx* c, const cpt_camera* cam, int min_spp, int max_spp, int batch, float rel_error, int max_depth,
                   uint32_t flags, const char* who) {
    if (!c || !cam) return CPT_ERR_INVALID_ARG;
    if (!max_depth_ok(max_depth))
        return fail(c, CPT_ERR_INVALID_ARG, "%s: max_depth %d (must be 0..32)", who, max_depth);
    if (batch < 1 || min_spp < batch || max_spp < min_spp || min_spp % batch || max_spp % batch ||
        (min_spp < 2 * batch && min_spp != max_spp))
        return fail(c, CPT_ERR_INVALID_ARG,
                    "%s: min_spp %d, max_spp %d, batch %d (multiples of batch >= 1, batch <= min_spp <= "
                    "max_spp, min_spp >= 2 batch unless min_spp == max_spp)",
                    who, min_spp, max_spp, batch);
    if (!(rel_error >= 0.f)) return fail(c, CPT_ERR_INVALID_ARG, "%s: rel_error %g", who, (double)rel_error);
    if (flags & CPT_PATH_WAVEFRONT) return fail(c, CPT_ERR_UNSUPPORTED, "%s: the wavefront path has no adaptive render", who);
    if (flags & CPT_SCHEDULE_PREVIOUS)
        return fail(c, CPT_ERR_UNSUPPORTED, "%s: CPT_SCHEDULE_PREVIOUS (use CPT_SCHEDULE_COST)", who);
    Frame& f = c->frame;
    if (f.adaptive.pending.on) return fail(c, CPT_ERR_STATE, "%s: an adaptive render is pending (cpt_adaptive_step until 0)", who);
    if (int rc = renderable(c, cam, who)) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream();
    const size_t npix = c->npix(), tiles = n_tiles(c);
    f.adaptive.done = false;
    f.adaptive.rounds.clear();
    f.adaptive.passes = 0;
    AdaptiveState::Pending a{};
    a.batch = batch;
    a.min_spp = min_spp;
    a.max_rounds = max_spp / batch;
    a.rel_error = rel_error;
    a.active = (uint32_t)tiles;
    if (tiles == 0) {   // a context without rows: nothing to queue; the first step ends it
        a.on = true;
        f.adaptive.pending = a;
        return CPT_OK;
    }
    int rc;
    a.aux = (flags & CPT_RENDER_AUX) != 0;
    a.stats = (flags & CPT_RENDER_STATS) != 0;
    if (a.aux && (rc = f.ensure_aux(c, npix)) != CPT_OK) return rc;
    AdaptiveState& ad = f.adaptive;
    if ((rc = ensure_all(c, ad.d_snap, npix, ad.d_stat, 4 * npix, ad.d_keep, tiles, ad.d_order[0], tiles, ad.d_order[1], tiles,
                         ad.d_count, 2)) != CPT_OK)
        return rc;
    // a new estimate: no batch seen; the snapshot is the accumulator the first round adds to
    HIP_TRY(c, hipMemsetAsync(f.adaptive.d_stat, 0, 4 * npix * sizeof(float), s));
    if (flags & CPT_RENDER_ACCUMULATE)
        HIP_TRY(c, hipMemcpyAsync(f.adaptive.d_snap, f.d_accum, npix * sizeof(float4), hipMemcpyDeviceToDevice, s));
    else
        HIP_TRY(c, hipMemsetAsync(f.adaptive.d_snap, 0, npix * sizeof(float4), s));

    fill_params(c, cam, batch, max_depth, flags, a.p);
    c->t_render.recorded = false;   // ev_start .. ev_stop span the rounds: no timing until the last step
    if ((rc = c->t_render.begin(c, s)) != CPT_OK) return rc;
    if (flags & CPT_SCHEDULE_COST) {
        // one pilot, sized for the whole render; the rounds filter its order
        if ((rc = cost_pilot(c, a.p, cost_pilot_passes(max_spp), s)) != CPT_OK) return rc;
        a.p.tile_order = f.schedule.d_cost_order;
    }
    if ((rc = consolidation_slab(c, a.p, batch, flags)) != CPT_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_main, s));
    f.adaptive.pending = a;
    if ((rc = enqueue_round(c)) != CPT_OK) {
        f.adaptive.pending = AdaptiveState::Pending{};
        return rc;
    }
    f.adaptive.pending.on = true;
    return CPT_OK;
}

// The pending round's result, then the next round or the end of the render.
int adaptive_step(cpt_ctx* c, int* active_tiles, const char* who) {
    Frame& f = c->frame;
    AdaptiveState::Pending& a = f.adaptive.pending;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream();
    if (a.queued) {
        // the read-back only: what the stream holds behind it (nothing, today) is not waited for
        HIP_TRY(c, hipEventSynchronize(c->ev_round));
        a.queued = false;
        const volatile uint32_t* h = c->h_ad_words.get();
        const uint32_t kept = h[0], pixels = h[1], dev_err = h[2];
        if (dev_err) {
            const int rc = check_device_error(c);   // reports and clears the word
            return rc != CPT_OK ? rc : fail(c, CPT_ERR_DEVICE, "%s: device error 0x%x", who, dev_err);
        }
        if (kept > a.active) return fail(c, CPT_ERR_DEVICE, "%s: %u of %u tiles kept", who, kept, a.active);
        f.adaptive.rounds.push_back(a.active);
        f.adaptive.passes += (uint64_t)pixels * (uint64_t)a.batch;
        a.active = kept;
        a.p.tile_order = f.adaptive.d_order[a.into];
        a.into ^= 1;
    }
    if (a.active > 0) {
        if (int rc = enqueue_round(c)) return rc;
        *active_tiles = (int)a.active;
        return CPT_OK;
    }
    if (a.round > 0) {   // rounds ran (a context without rows has none, and no timing)
        if (int rc = c->t_render.end(c, s)) return rc;
        HIP_TRY(c, hipStreamSynchronize(s));
        c->last_launches = (int)f.adaptive.rounds.size();
        f.schedule.draws_moved();
    }
    f.adaptive.pending = AdaptiveState::Pending{};
    f.adaptive.done = true;
    *active_tiles = 0;
    return CPT_OK;
}

// A failed step ends the render: nothing pending, no adaptive result; the stream is drained so
// that what it still holds cannot run into the caller's next call.
int adaptive_step_checked(cpt_ctx* c, int* active_tiles, const char* who) {
    if (!c->frame.adaptive.pending.on) return fail(c, CPT_ERR_STATE, "%s: no adaptive render is pending (cpt_adaptive_begin first)", who);
    const int rc = adaptive_step(c, active_tiles, who);
    if (rc != CPT_OK) {
        c->frame.adaptive.pending = AdaptiveState::Pending{};
        c->frame.adaptive.done = false;
        (void)hipStreamSynchronize(c->stream());
    }
    return rc;
}

}  // namespace

extern "C" {

int cpt_adaptive_begin(cpt_ctx* c, const cpt_camera* cam, int min_spp, int max_spp, int batch, float rel_error,
                       int max_depth, uint32_t flags) {
    return adaptive_begin(c, cam, min_spp, max_spp, batch, rel_error, max_depth, flags, "cpt_adaptive_begin");
}

int cpt_adaptive_step(cpt_ctx* c, int* active_tiles) {
    if (!c || !active_tiles) return CPT_ERR_INVALID_ARG;
    return adaptive_step_checked(c, active_tiles, "cpt_adaptive_step");
}

int cpt_render_adaptive(cpt_ctx* c, const cpt_camera* cam, int min_spp, int max_spp, int batch, float rel_error,
                        int max_depth, uint32_t flags) {
    static const char who[] = "cpt_render_adaptive";
    if (int rc = adaptive_begin(c, cam, min_spp, max_spp, batch, rel_error, max_depth, flags, who)) return rc;
    for (int active = 1; active > 0;)
        if (int rc = adaptive_step_checked(c, &active, who)) return rc;
    return CPT_OK;
}

int cpt_read_noise(cpt_ctx* c, float* rel, size_t capacity) {
    if (!c || !rel) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set || !c->frame.adaptive.done) return fail(c, CPT_ERR_STATE, "cpt_read_noise: cpt_render_adaptive first");
    const size_t n = c->npix();
    if (capacity < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_noise: %zu < %zu pixels", capacity, n);
    if (int rc = sync_checked(c)) return rc;
    return read_back(c, rel, c->frame.adaptive.d_stat, n, 3 * n);   // the fourth plane
}

int cpt_adaptive_info(cpt_ctx* c, int* rounds, uint32_t* active_tiles_per_round, int capacity, uint64_t* passes_done) {
    if (!c || capacity < 0 || (capacity > 0 && !active_tiles_per_round)) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.set || !f.adaptive.done) return fail(c, CPT_ERR_STATE, "cpt_adaptive_info: cpt_render_adaptive first");
    if (rounds) *rounds = (int)f.adaptive.rounds.size();
    if (passes_done) *passes_done = f.adaptive.passes;
    const size_t n = std::min((size_t)capacity, f.adaptive.rounds.size());
    std::copy(f.adaptive.rounds.begin(), f.adaptive.rounds.begin() + n, active_tiles_per_round);
    return CPT_OK;
}

int cpt_adaptive_decide_host(float m1, float m2, float k, float t, int* converged, float* rel) {
    if (!converged || !rel) return CPT_ERR_INVALID_ARG;
    *converged = cpt::adaptive::decide(m1, m2, k, t, *rel) ? 1 : 0;
    return CPT_OK;
}

}  // extern "C"
