// cpt_capi_render.cpp — the C-ABI's render launches (include/cpt.h): what a megakernel launch of
// the context's frame is made of (parameters, the shared preconditions, the cost pilot, the
// CPT_SCHEDULE_PREVIOUS order, the consolidation slab; cpt_capi_adaptive.cpp launches with the
// same pieces), the wavefront path's storage, cpt_render, cpt_tile_costs, the scheduling test
// hooks and the render's timing.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "cpt_context.hpp"

using namespace cpt::ctx;

// CPT_SCHEDULE_PREVIOUS: renders between rebuilds of the heaviest-first tile order.  Round 5,
// C4 DispatchRay loop, three interleaved rounds (profiles/r05/ab_dispatch_order_every.log): every
// render 1.71-1.72 ms per pass, every 4th 1.66-1.68, every 8th 1.65-1.66; the 1-spp render itself
// is unchanged (1.42-1.43), so the staler order costs nothing measurable.
constexpr int PREV_ORDER_EVERY = 8;

// The megakernel's parameters for a render of the context's frame (cpt_render, cpt_tile_costs,
// cpt_render_adaptive).
void cpt::ctx::fill_params(cpt_ctx* c, const cpt_camera* cam, int spp, int max_depth, uint32_t flags, cpt::KParams& p) {
    std::memset(&p, 0, sizeof(p));
    p.nodes = c->d_nodes;
    p.mats = c->d_mats;
    p.n_nodes = c->n_bvh;
    p.n_walk = c->n_walk;
    p.n_wide = c->n_wide;
    p.n_unb = c->n_unb;
    p.n_leaves = c->n_wide > 0 ? c->n_leaves : 0;
    p.ordered = (flags & CPT_TRAVERSAL_ORDERED) ? ((flags & CPT_TRAVERSAL_PLAIN_LEAVES) ? 2 : 1) : 0;
    p.env = c->d_env;
    p.env_w = c->env_w;
    p.env_h = c->env_h;
    p.env_cols = c->d_env ? c->env_cols : 0;
    for (int k = 0; k < 3; ++k) {
        p.cam.origin[k] = (&cam->origin.x)[k];
        p.cam.u[k] = (&cam->u.x)[k];
        p.cam.v[k] = (&cam->v.x)[k];
        p.cam.top_left[k] = (&cam->top_left_corner.x)[k];
        p.cam.horizontal[k] = (&cam->horizontal.x)[k];
        p.cam.vertical[k] = (&cam->vertical.x)[k];
    }
    p.cam.lens_radius = cam->lens_radius;
    p.cam.width = cam->width;
    p.cam.height = cam->height;
    p.cam.inv_w = 1.0 / (double)(float)cam->width;
    p.cam.inv_h = 1.0 / (double)(float)cam->height;
    p.rows = c->frame.d_rows;
    p.n_rows = c->n_rows;
    p.width = c->width;
    p.rng = c->frame.d_rng;
    p.accum = c->frame.d_accum;
    p.normal = c->frame.d_normal;
    p.depth = c->frame.d_depth;
    p.stats = c->d_stats;
    p.work = c->d_work;
    p.spp = spp;
    p.max_depth = max_depth;
    p.accumulate = (flags & CPT_RENDER_ACCUMULATE) ? 1 : 0;
    p.lanes = 64;
#ifdef CPT_DIAGNOSTIC_LANES
    // lane-latency experiments (tools/lane_latency.py builds with -DCPT_DIAGNOSTIC_LANES)
    if (const char* e = getenv("CPT_LANES_PER_WAVE")) p.lanes = std::max(1, std::min(64, atoi(e)));
    if (const char* e = getenv("CPT_REPLICATE")) p.replicate = std::max(1, std::min(64, atoi(e)));
#endif
    if (p.replicate < 1) p.replicate = 1;
    if (c->dbg_lanes_per_wave > 0) p.lanes = c->dbg_lanes_per_wave;   // TEST HOOK cpt_set_debug_grid
    p.error = c->d_work + 4;
    p.dbg = c->dbg;
    p.keeper_spin_log2 = c->keeper_spin_log2;
    p.publish_wait_log2 = c->publish_wait_log2;
}

int cpt::ctx::renderable(cpt_ctx* c, const cpt_camera* cam, const char* who) {
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "%s: cpt_set_scene first", who);
    if (!c->frame.set || !c->frame.rng_set) return fail(c, CPT_ERR_STATE, "%s: cpt_set_frame + cpt_init_rng first", who);
    if (cam->width != c->width || cam->height != c->height)
        return fail(c, CPT_ERR_INVALID_ARG, "%s: camera %dx%d vs frame %dx%d", who, cam->width, cam->height, c->width, c->height);
    return CPT_OK;
}

// The 8x8 tiles of the context's frame rows.
size_t cpt::ctx::n_tiles(const cpt_ctx* c) { return (size_t)cpt::TileGrid{c->width, c->n_rows}.count(); }

// The one list of the wavefront path's arrays: each is allocated for its view pointer's element
// type and the view filled from the same call.
int WfStorage::alloc(cpt_ctx* c, size_t npix, cpt::WfState& view) {
    WfStorage fresh;
    cpt::WfState v{};
    int rc = CPT_OK;
    auto take = [&](auto*& slot, size_t count) {
        using T = std::remove_reference_t<decltype(*slot)>;
        if (rc != CPT_OK) return;
        fresh.mem.emplace_back();
        rc = fresh.mem.back().ensure(c, count * sizeof(T));
        slot = reinterpret_cast<T*>(fresh.mem.back().get());
    };
    for (int b = 0; b < 2; ++b)
        for (float4** a : {&v.ray_o[b], &v.ray_d[b], &v.att[b], &v.rad[b], &v.aux[b]}) take(*a, npix);
    take(v.hit_p, npix);
    take(v.hit_n, npix);
    for (int b = 0; b < 2; ++b) {
        take(v.rng_a[b], npix);
        take(v.rng_b[b], npix);
    }
    for (int32_t** q : {&v.queue[0], &v.queue[1], &v.ident}) take(*q, npix);
    take(v.counts, 8);
    if (rc != CPT_OK) return rc;   // `fresh` releases what it got
    *this = std::move(fresh);
    view = v;
    return CPT_OK;
}

// The wavefront path's state, allocated on the frame's first wavefront render.
static int ensure_wavefront(cpt_ctx* c, const cpt::KParams& p, hipStream_t s) {
    Frame& f = c->frame;
    if (f.wavefront.ready || c->n_rows == 0) return CPT_OK;
    if (int rc = f.wavefront.mem.alloc(c, c->npix(), f.wavefront.view)) return rc;
    HIP_TRY(c, cpt::wavefront_build_ident(p, f.wavefront.view, s));
    f.wavefront.ready = true;
    return CPT_OK;
}

// CPT_SCHEDULE_PREVIOUS, before the render: the order the previous render's draws gave; the
// draws of this one are counted from here.
int TileSchedule::previous_begin(cpt_ctx* c, cpt::KParams& p, hipStream_t s) {
    const size_t npix = c->npix();
    if (prev_order_valid) p.tile_order = d_prev_order;
    if (int rc = d_prev_d.ensure(c, npix)) return rc;
    if (!prev_d_valid) {
        HIP_TRY(c, hipMemcpyAsync(d_prev_d, c->frame.d_rng + 5 * npix, npix * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
        prev_d_valid = true;   // the draws are counted from here
    }
    return CPT_OK;
}

// CPT_SCHEDULE_PREVIOUS, after the render: the next render's order from this one's draws (after
// the timed events: the render's own time is the kernel's; the stream runs this before the
// caller's next work).  Refreshed every PREV_ORDER_EVERY renders: the draws then span those
// renders (the RNG's d word counts them all), and the order, a heuristic, costs ~65 us to rebuild.
int TileSchedule::previous_refresh(cpt_ctx* c, const cpt::KParams& p, hipStream_t s) {
    if (prev_order_valid && ++prev_since_order < PREV_ORDER_EVERY) return CPT_OK;
    if (int rc = ensure_all(c, d_scratch, cpt::tile_schedule_scratch_bytes(c->width, c->n_rows), d_prev_order, n_tiles(c))) return rc;
    HIP_TRY(c, cpt::launch_tile_order_from_draws(p, d_prev_d, d_scratch, d_scratch.capacity(), d_prev_order, s));
    prev_d_valid = true;
    prev_order_valid = true;
    prev_since_order = 0;
    return CPT_OK;
}

// The cost schedule's pilot: `passes` passes, then the tiles sorted by their heaviest pixel,
// first, into the frame's tile order.  cpt_render runs min(PILOT_MAX, max(1, spp / PILOT_DIV))
// passes.  Round 6 (interleaved, profiles/r06/keymax/): with the max key, up to 16 passes at one
// per 128 spp against round 5's 4 at one per 512: C4 2182-2198 vs 2065-2072 Mpaths/s (8 passes
// at one per 256: 2159-2175), C5 N = 8 slowest rank 2101 vs 2388 ms; C2 / C3 unchanged.
constexpr int PILOT_MAX = 16, PILOT_DIV = 128;
int cpt::ctx::cost_pilot_passes(int spp) { return std::min(PILOT_MAX, std::max(1, spp / PILOT_DIV)); }
int cpt::ctx::cost_pilot(cpt_ctx* c, const cpt::KParams& p, int passes, hipStream_t s) {
    Frame& f = c->frame;
    if (int rc = ensure_all(c, f.schedule.d_scratch, cpt::tile_schedule_scratch_bytes(c->width, c->n_rows),
                            f.schedule.d_cost_order, n_tiles(c)))
        return rc;
    HIP_TRY(c, cpt::launch_tile_schedule(p, passes, f.schedule.d_scratch, f.schedule.d_scratch.capacity(), f.schedule.d_cost_order,
                                         c->grid, s));
    return CPT_OK;
}

// Tail consolidation (cpt_megakernel.hip): one slab of ho_slots chains per resident workgroup of
// the consolidating kernel, by the figure its launch gets from the context's grid (one LDS
// workgroup per CU): the slab and the grid cannot disagree (CPT_DEVERR_RESUME_CAP).  By
// default for frames of more than 1 and at most 4 pixels per lane and chains of at least
// 512 passes: with more pixels the tail is a small part of the render, with short chains
// the hand-overs do not pay, and the plain kernel's tighter code wins (DESIGN.md
// §Multi-GPU; C2 at 0.9 pixels per lane and 256 spp: 23.2 vs 21.9 Gpaths/s without).  At
// one pixel per lane no lane takes a second chain and the plain kernel wins too (C4 at
// N = 8, slowest rank: 309 vs 322 ms in r06, 314-318 vs 322 in r05, 304 vs 325 with
// this rule; profiles/r06/reh_cons_r06z.log, r06/cert/reh_c4_cons_rule.log,
// profiles/r05/reh_cons_off_vs_auto.log).
int cpt::ctx::consolidation_slab(cpt_ctx* c, cpt::KParams& p, int spp, uint32_t flags) {
    const bool forced = (flags & CPT_SCHEDULE_CONSOLIDATE) != 0;
    if (spp <= 1 || (!forced && ((flags & CPT_SCHEDULE_NO_CONSOLIDATE) || spp < 512))) return CPT_OK;
    long long resident = 0;
    HIP_TRY(c, cpt::consolidating_workgroups(p, (flags & CPT_RENDER_STATS) != 0, (flags & CPT_RENDER_AUX) != 0, c->grid,
                                             &resident));
    const size_t frame_px = c->npix(), grid_lanes = (size_t)cpt::LDS_BLOCK * (size_t)resident;
    if (!forced && !(frame_px > grid_lanes && frame_px <= 4u * grid_lanes)) return CPT_OK;
    const size_t cap = cpt::consolidation_chains(resident);
    if (int rc = c->d_resume.ensure(c, cpt::HO_SLOT_QUADS * cap)) return rc;
    p.resume = c->d_resume;
    p.resume_cap = cap;
    return CPT_OK;
}

extern "C" {

int cpt_render(cpt_ctx* c, const cpt_camera* cam, int spp, int max_depth, uint32_t flags) {
    if (!c || !cam) return CPT_ERR_INVALID_ARG;
    if (spp < 0 || !max_depth_ok(max_depth))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_render: spp %d, max_depth %d (must be 0..32)", spp, max_depth);
    CPT_REFUSE_PENDING(c, "cpt_render");
    if (int rc = renderable(c, cam, "cpt_render")) return rc;
    Frame& f = c->frame;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream();
    int rc;
    const bool aux = (flags & CPT_RENDER_AUX) != 0;
    if (aux && (rc = f.ensure_aux(c, c->npix())) != CPT_OK) return rc;
    cpt::KParams p;
    fill_params(c, cam, spp, max_depth, flags, p);
    const bool wavefront = (flags & CPT_PATH_WAVEFRONT) != 0;
    const bool work = spp > 0 && c->n_rows > 0;
    if (wavefront && (rc = ensure_wavefront(c, p, s)) != CPT_OK) return rc;
    if ((rc = c->t_render.begin(c, s)) != CPT_OK) return rc;
    if (wavefront) {
        if (!p.accumulate && c->n_rows > 0) HIP_TRY(c, hipMemsetAsync(f.d_accum, 0, c->npix() * sizeof(float4), s));
        int launches = 0;
        HIP_TRY(c, hipEventRecord(c->ev_main, s));
        HIP_TRY(c, cpt::launch_wavefront(p, f.wavefront.view, (flags & CPT_RENDER_STATS) != 0, aux, c->grid, s, &launches));
        c->last_launches = launches;
        if ((rc = c->t_render.end(c, s)) != CPT_OK) return rc;
    } else {
        c->last_launches = 1;
        const bool cost = (flags & CPT_SCHEDULE_COST) && work;
        const bool previous = !(flags & CPT_SCHEDULE_COST) && (flags & CPT_SCHEDULE_PREVIOUS) && work;
        if (previous && (rc = f.schedule.previous_begin(c, p, s)) != CPT_OK) return rc;
        if (cost) {
            if ((rc = cost_pilot(c, p, cost_pilot_passes(spp), s)) != CPT_OK) return rc;
            p.tile_order = f.schedule.d_cost_order;
        }
        if ((rc = consolidation_slab(c, p, spp, flags)) != CPT_OK) return rc;
        HIP_TRY(c, hipEventRecord(c->ev_main, s));
        HIP_TRY(c, cpt::launch_megakernel(p, (flags & CPT_RENDER_STATS) != 0, aux, c->grid, s));
        if ((rc = c->t_render.end(c, s)) != CPT_OK) return rc;
        if (previous && (rc = f.schedule.previous_refresh(c, p, s)) != CPT_OK) return rc;
    }
    if (flags & CPT_RENDER_SYNC) return sync_checked(c);
    return CPT_OK;
}

// The cost schedule's pilot on its own (cost-balanced row partitions, tiling.py): `passes` passes
// from the context's current RNG states, nothing written back, into `out` the work (segments +
// node visits + primitive tests) of each 8x8 tile's heaviest pixel: the pilot keeps a tile's
// maximum over its pixels, not their sum (cpt_megakernel.hip, the tile_cost update).
int cpt_tile_costs(cpt_ctx* c, const cpt_camera* cam, int passes, int max_depth, uint32_t flags, uint32_t* out,
                   size_t n_out) {
    if (!c || !cam || !out || passes < 1 || !max_depth_ok(max_depth)) return CPT_ERR_INVALID_ARG;
    if (int rc = renderable(c, cam, "cpt_tile_costs")) return rc;
    if (n_out < n_tiles(c)) return fail(c, CPT_ERR_INVALID_ARG, "cpt_tile_costs: %zu < %zu tiles", n_out, n_tiles(c));
    if (n_tiles(c) == 0) return CPT_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream();
    cpt::KParams p;
    fill_params(c, cam, passes, max_depth, flags & WALK_FLAGS, p);
    if (int rc = cost_pilot(c, p, passes, s)) return rc;
    // the unsorted costs are the scratch's first n_tiles words (the sort writes elsewhere)
    HIP_TRY(c, hipMemcpyAsync(out, c->frame.schedule.d_scratch, n_tiles(c) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    return sync_checked(c);
}

int cpt_set_debug_consolidation(cpt_ctx* c, uint32_t flags, int keeper_spin_log2, int publish_wait_log2) {
    if (!c || keeper_spin_log2 < 0 || keeper_spin_log2 > 30 || publish_wait_log2 < 0 || publish_wait_log2 > 30 ||
        (flags & ~3u))
        return c ? fail(c, CPT_ERR_INVALID_ARG, "cpt_set_debug_consolidation: bad arguments") : CPT_ERR_INVALID_ARG;
    c->dbg = flags;
    c->keeper_spin_log2 = keeper_spin_log2;
    c->publish_wait_log2 = publish_wait_log2;
    return CPT_OK;
}

int cpt_set_debug_grid(cpt_ctx* c, int max_workgroups, int lanes_per_wave) {
    if (!c || max_workgroups < 0 || lanes_per_wave < 0 || lanes_per_wave > 64)
        return c ? fail(c, CPT_ERR_INVALID_ARG, "cpt_set_debug_grid: bad arguments") : CPT_ERR_INVALID_ARG;
    c->grid.max_workgroups = max_workgroups;
    c->dbg_lanes_per_wave = lanes_per_wave;
    return CPT_OK;
}

int cpt_launch_grid_host(int cus, int blocks_per_cu, int block, int64_t tiles, int lanes, int replicate, int max_workgroups,
                         int* workgroups, uint64_t* slab_chains) {
    if (!workgroups || cus < 1 || blocks_per_cu < 1 || block < 1 || tiles < 0) return CPT_ERR_INVALID_ARG;
    const long long resident = (long long)blocks_per_cu * cus;
    *workgroups = cpt::grid_workgroups(cpt::megakernel_want(tiles, lanes, replicate, block), resident, max_workgroups);
    if (slab_chains) *slab_chains = cpt::consolidation_chains(resident);
    return CPT_OK;
}

int cpt_last_render_ms(cpt_ctx* c, float* ms) {
    if (int rc = last_span_ms(c, &cpt_ctx::t_render, ms, "cpt_last_render_ms: nothing rendered")) return rc;
    c->last_kernel_ms = *ms;
    return CPT_OK;
}

int cpt_last_kernel_stats(cpt_ctx* c, float* avg_ms, int* launches) {
    if (!c || !avg_ms || !launches) return CPT_ERR_INVALID_ARG;
    float ms = 0.f;
    int rc = cpt_last_render_ms(c, &ms);
    if (rc != CPT_OK) return rc;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_main, c->t_render.t1));   // without the pilot
    *launches = c->last_launches;
    *avg_ms = c->last_launches > 0 ? ms / (float)c->last_launches : 0.f;
    return CPT_OK;
}

}  // extern "C"
