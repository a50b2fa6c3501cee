// cpt_capi_topup.cpp — the C-ABI's top-up render (include/cpt.h):
// cpt_render_to_count gives every pixel the passes its accumulator count lacks to a target, in one
// megakernel launch over the tiles that have a deficit, heaviest first; cpt_topup_info reads the
// plan's totals back; cpt_topup_deficit_host is the deficit rule without a GPU.  The plan's kernel
// is cpt_topup.hip's, the launch cpt_render's (cpt_capi_render.cpp's helpers) with the TOPUP
// kernels; the rule is cpt_topup.hpp's on both sides.
#include <hip/hip_runtime.h>

#include "cpt_context.hpp"
#include "cpt_topup.hpp"

using namespace cpt::ctx;
namespace tu = cpt::topup;

extern "C" {

int cpt_render_to_count(cpt_ctx* c, const cpt_camera* cam, int target, int max_depth, uint32_t flags) {
    static const char who[] = "cpt_render_to_count";
    if (!c || !cam) return CPT_ERR_INVALID_ARG;
    if (target < 1 || target > tu::MAX_TARGET || !max_depth_ok(max_depth))
        return fail(c, CPT_ERR_INVALID_ARG, "%s: target %d (must be 1..%d), max_depth %d (must be 0..32)", who, target,
                    tu::MAX_TARGET, max_depth);
    if (flags & CPT_PATH_WAVEFRONT) return fail(c, CPT_ERR_UNSUPPORTED, "%s: the wavefront path has no top-up render", who);
    if (flags & (CPT_SCHEDULE_PREVIOUS | CPT_SCHEDULE_COST))
        return fail(c, CPT_ERR_UNSUPPORTED, "%s: CPT_SCHEDULE_PREVIOUS / CPT_SCHEDULE_COST (the order is the plan's)", who);
    if (flags & CPT_SCHEDULE_CONSOLIDATE) return fail(c, CPT_ERR_UNSUPPORTED, "%s: a top-up launch never consolidates", who);
    CPT_REFUSE_PENDING(c, who);
    if (int rc = renderable(c, cam, who)) return rc;
    Frame& f = c->frame;
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream();
    int rc;
    const bool aux = (flags & CPT_RENDER_AUX) != 0;
    if (aux && (rc = f.ensure_aux(c, c->npix())) != CPT_OK) return rc;
    if ((rc = f.topup.d_words.ensure(c, tu::PLAN_WORDS)) != CPT_OK) return rc;
    const size_t tiles = n_tiles(c);
    if (tiles > 0 && (rc = ensure_all(c, f.schedule.d_scratch, cpt::tile_schedule_scratch_bytes(c->width, c->n_rows),
                                      f.topup.d_order, tiles)) != CPT_OK)
        return rc;
    cpt::KParams p;
    fill_params(c, cam, target, max_depth, flags | CPT_RENDER_ACCUMULATE, p);
    p.tile_order = f.topup.d_order;
    p.topup_active = f.topup.d_words.get() + tu::PLAN_ACTIVE;
    if ((rc = c->t_render.begin(c, s)) != CPT_OK) return rc;
    const cpt::TopupPlan plan{f.d_accum, c->width, c->n_rows, target, f.topup.d_order, f.topup.d_words};
    HIP_TRY(c, cpt::launch_topup_plan(plan, f.schedule.d_scratch, f.schedule.d_scratch.capacity(), s));
    f.topup.planned = true;
    HIP_TRY(c, hipEventRecord(c->ev_main, s));
    HIP_TRY(c, cpt::launch_megakernel_topup(p, (flags & CPT_RENDER_STATS) != 0, aux, c->grid, s));
    if ((rc = c->t_render.end(c, s)) != CPT_OK) return rc;
    c->last_launches = 1;
    // draws happened outside a CPT_SCHEDULE_PREVIOUS render: its next one counts from its start
    f.schedule.draws_moved();
    if (flags & CPT_RENDER_SYNC) return sync_checked(c);
    return CPT_OK;
}

int cpt_topup_info(cpt_ctx* c, uint32_t* tiles, uint64_t* pixels, uint64_t* passes) {
    if (!c) return CPT_ERR_INVALID_ARG;
    Frame& f = c->frame;
    if (!f.set || !f.topup.planned) return fail(c, CPT_ERR_STATE, "cpt_topup_info: cpt_render_to_count first");
    if (int rc = sync_checked(c)) return rc;
    uint32_t w[tu::PLAN_WORDS];
    if (int rc = read_back(c, w, f.topup.d_words, tu::PLAN_WORDS)) return rc;
    if (tiles) *tiles = w[tu::PLAN_ACTIVE];
    if (pixels) *pixels = (uint64_t)w[tu::PLAN_PIXELS] | ((uint64_t)w[tu::PLAN_PIXELS + 1] << 32);
    if (passes) *passes = (uint64_t)w[tu::PLAN_PASSES] | ((uint64_t)w[tu::PLAN_PASSES + 1] << 32);
    return CPT_OK;
}

int cpt_topup_deficit_host(float count, int target, int* d) {
    if (!d || target < 1 || target > tu::MAX_TARGET) return CPT_ERR_INVALID_ARG;
    *d = tu::deficit(count, target);
    return CPT_OK;
}

}  // extern "C"
