// cpt_capi_adaptive.cpp — the C-ABI's adaptive render (include/cpt.h, DESIGN.md §Adaptive
// sampling): rounds of `batch` passes over the 8x8 tiles that are still noisy, the noise map and
// the round record, and the host-only hook on the criterion.  Each round is the launch cpt_render
// makes (cpt_capi.cpp's helpers), over a shorter tile order; the kernels around it are
// cpt_adaptive.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "cpt_adaptive.hpp"
#include "cpt_context.hpp"

using namespace cpt::ctx;

extern "C" {

int cpt_render_adaptive(cpt_ctx* c, const cpt_camera* cam, int min_spp, int max_spp, int batch, float rel_error,
                        int max_depth, uint32_t flags) {
    if (!c || !cam) return CPT_ERR_INVALID_ARG;
    if (max_depth < 0 || max_depth > (int)cpt::MAX_RECURSION_DEPTH_SET)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_render_adaptive: max_depth %d (must be 0..32)", max_depth);
    if (batch < 1 || min_spp < batch || max_spp < min_spp || min_spp % batch || max_spp % batch ||
        (min_spp < 2 * batch && min_spp != max_spp))
        return fail(c, CPT_ERR_INVALID_ARG,
                    "cpt_render_adaptive: min_spp %d, max_spp %d, batch %d (multiples of batch >= 1, batch <= min_spp <= "
                    "max_spp, min_spp >= 2 batch unless min_spp == max_spp)",
                    min_spp, max_spp, batch);
    if (!(rel_error >= 0.f)) return fail(c, CPT_ERR_INVALID_ARG, "cpt_render_adaptive: rel_error %g", (double)rel_error);
    if (flags & CPT_PATH_WAVEFRONT)
        return fail(c, CPT_ERR_UNSUPPORTED, "cpt_render_adaptive: the wavefront path has no adaptive render");
    if (flags & CPT_SCHEDULE_PREVIOUS)
        return fail(c, CPT_ERR_UNSUPPORTED, "cpt_render_adaptive: CPT_SCHEDULE_PREVIOUS (use CPT_SCHEDULE_COST)");
    Frame& f = c->frame;
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "cpt_render_adaptive: cpt_set_scene first");
    if (!f.set || !f.rng_set) return fail(c, CPT_ERR_STATE, "cpt_render_adaptive: cpt_set_frame + cpt_init_rng first");
    if (cam->width != c->width || cam->height != c->height)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_render_adaptive: camera %dx%d vs frame %dx%d", cam->width, cam->height,
                    c->width, c->height);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream();
    const size_t npix = c->npix(), tiles = n_tiles(c);
    const int max_rounds = max_spp / batch;
    f.ad_done = false;
    f.ad_active.clear();
    f.ad_passes = 0;
    if (tiles == 0) {   // a context without rows: nothing to render, an empty record
        f.ad_done = true;
        return CPT_OK;
    }
    int rc;
    const bool aux = (flags & CPT_RENDER_AUX) != 0, stats = (flags & CPT_RENDER_STATS) != 0;
    if (aux) {
        if ((rc = f.d_normal.ensure(c, npix * 3)) != CPT_OK) return rc;
        if ((rc = f.d_depth.ensure(c, npix)) != CPT_OK) return rc;
    }
    if ((rc = f.d_ad_snap.ensure(c, npix)) != CPT_OK || (rc = f.d_ad_stat.ensure(c, 4 * npix)) != CPT_OK ||
        (rc = f.d_ad_keep.ensure(c, tiles)) != CPT_OK || (rc = f.d_ad_order[0].ensure(c, tiles)) != CPT_OK ||
        (rc = f.d_ad_order[1].ensure(c, tiles)) != CPT_OK || (rc = f.d_ad_count.ensure(c, 2)) != CPT_OK)
        return rc;
    // a new estimate: no batch seen; the snapshot is the accumulator the first round adds to
    HIP_TRY(c, hipMemsetAsync(f.d_ad_stat, 0, 4 * npix * sizeof(float), s));
    if (flags & CPT_RENDER_ACCUMULATE)
        HIP_TRY(c, hipMemcpyAsync(f.d_ad_snap, f.d_accum, npix * sizeof(float4), hipMemcpyDeviceToDevice, s));
    else
        HIP_TRY(c, hipMemsetAsync(f.d_ad_snap, 0, npix * sizeof(float4), s));

    cpt::KParams p;
    fill_params(c, cam, batch, max_depth, flags, p);
    HIP_TRY(c, hipEventRecord(c->ev_start, s));
    if (flags & CPT_SCHEDULE_COST) {
        // one pilot, sized for the whole render; the rounds filter its order
        if ((rc = cost_pilot(c, p, cost_pilot_passes(max_spp), s)) != CPT_OK) return rc;
        p.tile_order = f.d_tile_order;
    }
    if ((rc = consolidation_slab(c, p, batch, flags)) != CPT_OK) return rc;
    HIP_TRY(c, hipEventRecord(c->ev_main, s));
    uint32_t active = (uint32_t)tiles;
    int into = 0;   // the order buffer the next compaction writes
    for (int round = 1; active > 0; ++round) {
        // round 1 is cpt_render's own launch (every tile, the caller's accumulate flag); later
        // rounds add to what the earlier ones left, over the tiles still listed
        if (round > 1) {
            p.accumulate = 1;
            p.n_active = active;
        }
        HIP_TRY(c, cpt::launch_megakernel(p, stats, aux, c->dbg_max_workgroups, s));
        cpt::AdaptiveRound a{};
        a.order = p.tile_order;
        a.n_active = active;
        a.width = c->width;
        a.n_rows = c->n_rows;
        a.accum = f.d_accum;
        a.snap = f.d_ad_snap;
        a.stat = f.d_ad_stat;
        a.keep = f.d_ad_keep;
        a.rel_error = rel_error;
        a.eligible = (long long)round * batch >= min_spp;
        a.last = round >= max_rounds;
        HIP_TRY(c, cpt::launch_tile_noise(a, s));
        HIP_TRY(c, cpt::launch_compact_order(p.tile_order, f.d_ad_keep, active, c->width, c->n_rows, f.d_ad_order[into],
                                             f.d_ad_count, s));
        uint32_t got[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(got, f.d_ad_count, sizeof(got), hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
        if ((rc = check_device_error(c)) != CPT_OK) return rc;
        if (got[0] > active) return fail(c, CPT_ERR_DEVICE, "cpt_render_adaptive: %u of %u tiles kept", got[0], active);
        f.ad_active.push_back(active);
        f.ad_passes += (uint64_t)got[1] * (uint64_t)batch;
        active = got[0];
        p.tile_order = f.d_ad_order[into];
        into ^= 1;
    }
    HIP_TRY(c, hipEventRecord(c->ev_stop, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    c->last_launches = (int)f.ad_active.size();
    c->have_timing = true;
    f.prev_d_valid = false;   // CPT_SCHEDULE_PREVIOUS counts draws from the next render on
    f.ad_done = true;
    return CPT_OK;
}

int cpt_read_noise(cpt_ctx* c, float* rel, size_t capacity) {
    if (!c || !rel) return CPT_ERR_INVALID_ARG;
    if (!c->frame.set || !c->frame.ad_done) return fail(c, CPT_ERR_STATE, "cpt_read_noise: cpt_render_adaptive first");
    const size_t n = c->npix();
    if (capacity < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_noise: %zu < %zu pixels", capacity, n);
    if (int rc = sync_checked(c)) return rc;
    if (n) HIP_TRY(c, hipMemcpy(rel, c->frame.d_ad_stat + 3 * n, n * sizeof(float), hipMemcpyDeviceToHost));
    return CPT_OK;
}

int cpt_adaptive_info(cpt_ctx* c, int* rounds, uint32_t* active_tiles_per_round, int capacity, uint64_t* passes_done) {
    if (!c || capacity < 0 || (capacity > 0 && !active_tiles_per_round)) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.set || !f.ad_done) return fail(c, CPT_ERR_STATE, "cpt_adaptive_info: cpt_render_adaptive first");
    if (rounds) *rounds = (int)f.ad_active.size();
    if (passes_done) *passes_done = f.ad_passes;
    const size_t n = std::min((size_t)capacity, f.ad_active.size());
    std::copy(f.ad_active.begin(), f.ad_active.begin() + n, active_tiles_per_round);
    return CPT_OK;
}

int cpt_adaptive_decide_host(float m1, float m2, float k, float t, int* converged, float* rel) {
    if (!converged || !rel) return CPT_ERR_INVALID_ARG;
    *converged = cpt::adaptive::decide(m1, m2, k, t, *rel) ? 1 : 0;
    return CPT_OK;
}

}  // extern "C"
