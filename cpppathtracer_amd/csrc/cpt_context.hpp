// cpt_context.hpp — the C-ABI's context (struct cpt_ctx of include/cpt.h) and the helpers its
// implementation files share: cpt_capi.cpp (context, frame, RNG, accumulator, counters),
// cpt_capi_render.cpp (render launches, tile schedules, timing), cpt_capi_adaptive.cpp (adaptive
// render), cpt_capi_filter.cpp (a-trous filter), cpt_capi_gather.cpp (row-tile gather),
// cpt_capi_display.cpp (display path), cpt_capi_query.cpp (G-buffer, ray queries, picking),
// cpt_capi_reproject.cpp (reprojection to a moved camera), cpt_capi_topup.cpp (top-up render),
// cpt_capi_probes.cpp (diagnostic probes, self-tests), cpt_capi_present.cpp (presenting, DESIGN.md
// §26), cpt_antialias_capi.cpp (antialiased presentation), cpt_bloom_capi.cpp (bloom,
// DESIGN.md §28) and cpt_scene.cpp (scene upload, material slots, walk trees, device refit).  What those files
// would otherwise each spell out is here once: the timed spans (TimedSpan), the buffer lists
// (GBufferState::ensure, Frame::ensure_aux; ensure_all, read_back and write_in are cpt_devmem.hpp's),
// the two drains, and the argument checks more than one file makes.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cpt.h"
#include "cpt_devmem.hpp"
#include "cpt_host.hpp"
#include "cpt_internal.hpp"
#include "cpt_tiles.hpp"

using cpt::Mat;
using cpt::Node;
using cpt::TexDesc;
using cpt::ctx::DevBuf;
using cpt::ctx::DevEvent;
using cpt::host::HostBvh;

// The wavefront path's storage, owned beside the plain view (cpt::WfState) the launchers take.
struct WfStorage {
    std::vector<DevBuf<uint8_t>> mem;   // 12 float4 + 4 RNG + 3 queue arrays and the counts
    // All arrays for `npix` pixels and the view of them, or nothing: a failed allocation
    // part-way leaves both as they were (cpt_capi_render.cpp, the one list of the arrays).
    int alloc(cpt_ctx* c, size_t npix, cpt::WfState& view);
};

// What lives and dies with cpt_set_frame (which assigns a fresh Frame), by subsystem: each owns its
// device buffers, sized by the frame and allocated on first use, and the flags that say what they hold.

// The tile orders of CPT_SCHEDULE_COST and CPT_SCHEDULE_PREVIOUS (cpt_capi_render.cpp).
struct TileSchedule {
    DevBuf<uint8_t> d_scratch;       // pilot tile costs + sort scratch (bytes), shared by both orders
    DevBuf<uint32_t> d_cost_order;   // the cost pilot's order (cost_pilot)
    // CPT_SCHEDULE_PREVIOUS: the Weyl plane the draws are counted from, and the tile order the
    // draws up to the last rebuild gave (the next such render's dequeue order)
    DevBuf<uint32_t> d_prev_d, d_prev_order;

    // The RNG streams were replaced (cpt_init_rng): the order was measured on streams that are
    // gone, and so was the plane.  The next CPT_SCHEDULE_PREVIOUS render runs in raster order,
    // counts its draws from its start and rebuilds the order.
    void rng_replaced() {
        prev_d_valid = prev_order_valid = false;
        prev_since_order = 0;
    }
    // Draws happened, or the states changed, outside a CPT_SCHEDULE_PREVIOUS render (cpt_write_rng,
    // an adaptive render): the plane no longer matches, so the next such render counts from its
    // start.  The order stays valid, and its rebuild is not brought forward: it is a heuristic for
    // the dequeue order only, the image does not depend on it, and a caller who writes back states
    // it read (a checkpoint) keeps the order that fits them.
    void draws_moved() { prev_d_valid = false; }
    // The CPT_SCHEDULE_PREVIOUS order, or null while none is valid.
    const uint32_t* previous_order() const { return prev_order_valid ? d_prev_order.get() : nullptr; }
    // Around a CPT_SCHEDULE_PREVIOUS render: the order to dequeue in and the plane to count from;
    // then, every PREV_ORDER_EVERY renders, the order rebuilt from the draws since.
    int previous_begin(cpt_ctx* c, cpt::KParams& p, hipStream_t s);
    int previous_refresh(cpt_ctx* c, const cpt::KParams& p, hipStream_t s);

private:
    bool prev_d_valid = false, prev_order_valid = false;
    int prev_since_order = 0;   // renders since the order was rebuilt
};

// The wavefront path (allocated on the frame's first wavefront render).
struct WavefrontState {
    cpt::WfState view{};
    WfStorage mem;
    bool ready = false;   // allocated, the identity queue built
};

// The display path (cpt_capi_display.cpp): the buffers of one band of output rows.
struct DisplayBand {
    DevBuf<float> d_mix;       // running mean (Mix), rgb per pixel of the band
    DevBuf<uint8_t> d_bgra;    // the display frame (band rows)
    DevBuf<float4> d_sink;     // k_denoise_strip: where lanes without an output pixel store (DN_SINK_SLOTS)
    int y0 = -1, y1 = -1;      // the band the buffers hold
    // The per-pixel display history (cpt_denoise_mix_history, cpt_reproject_display):
    // each pixel's sample count beside d_mix, an integer held as a float.  cpt_denoise_mix[_band]
    // does not write it: it records its index and marks the plane stale, and the next reader of
    // the plane first fills the launch region with that index (fill_count).
    DevBuf<float> d_count;
    uint32_t last_idx = 0;     // the last recorded global index (0: none since the planes were zeroed)
    bool count_stale = false;
    // the planes the next cpt_reproject_display writes; swapped with d_mix / d_count behind it
    DevBuf<float> d_mix_next, d_count_next;

    // the count plane brought up to date on the context's stream (cpt_capi_display.cpp)
    int fill_count(cpt_ctx* c);
};

// The adaptive render (cpt_capi_adaptive.cpp; allocated on the frame's first cpt_render_adaptive).
struct AdaptiveState {
    // the accumulator before the current round, the per-pixel moments and noise map (planar
    // [4][npix]: m1, m2, k, rel), a keep flag per position of the active list, the list's two
    // buffers (each round compacts one into the other) and {new length, pixels rendered}
    DevBuf<float4> d_snap;
    DevBuf<float> d_stat;
    DevBuf<uint32_t> d_keep, d_order[2], d_count;
    bool done = false;               // d_stat holds a result (a completed render's, or an adopted one)
    std::vector<uint32_t> rounds;    // the render's rounds: the tiles each one rendered
    uint64_t passes = 0;             // its pixel passes, all rounds
    // a render between cpt_adaptive_begin and the cpt_adaptive_step that returns 0: what the next
    // round is launched with; `queued`: a round and its read-back are on the stream
    struct Pending {
        bool on = false, queued = false;
        cpt::KParams p{};
        bool stats = false, aux = false;
        int batch = 0, min_spp = 0, max_rounds = 0;
        float rel_error = 0.f;
        int round = 0;          // rounds queued so far
        uint32_t active = 0;    // tiles of the round queued (or to queue) next
        int into = 0;           // the order buffer the next compaction writes
    } pending;

    // moments of `npix` pixels that the filter and the gather can read
    bool has_result(size_t npix) const { return done && d_stat.capacity() >= 4 * npix; }
    // d_stat was filled from outside (cpt_write_moments, a gather): a result that no round of
    // this context produced, with an empty round record
    void adopt_result() {
        rounds.clear();
        passes = 0;
        done = true;
    }
};

// The a-trous filter (cpt_capi_filter.cpp; allocated on the frame's first cpt_filter_frame or
// cpt_filter_frame_spatial, which share the planes).
struct FilterState {
    DevBuf<float4> d_plane[2];   // the levels ping-pong between them (rgb + variance of the mean)
    DevBuf<uint8_t> d_ok;        // each pixel's validity
    int result = -1;             // the plane that holds the last call's result (-1: no call yet)
};

// The G-buffer (cpt_capi_query.cpp; allocated on the frame's first cpt_gbuffer or cpt_write_gbuffer).
struct GBufferState {
    DevBuf<int32_t> d_id;               // object index per pixel (-1: miss)
    DevBuf<float> d_t;                  // hit distance
    DevBuf<float> d_normal, d_albedo;   // [npix][3] each
    bool valid = false;                 // a cpt_gbuffer has been queued, or a cpt_write_gbuffer made, since cpt_set_frame

    // the four planes of `npix` pixels
    int ensure(cpt_ctx* c, size_t npix) { return cpt::ctx::ensure_all(c, d_id, npix, d_t, npix, d_normal, 3 * npix, d_albedo, 3 * npix); }
};

// The reprojection (cpt_capi_reproject.cpp; allocated on the frame's first cpt_reproject_accum or
// cpt_reproject_display, which uses the history's id and distance planes).
struct ReprojectState {
    DevBuf<int32_t> d_id;      // the G-buffer at the camera the history was rendered with: object
    DevBuf<float> d_t;         // index and hit distance per pixel
    DevBuf<float4> d_accum;    // the plane the next call writes; swapped with Frame::d_accum behind it
    // The captured history (cpt_history_capture and the tracked calls): d_id / d_t
    // then hold the G-buffer at `cam` of the scene as `objs` had it.  Dropped by the untracked
    // cpt_reproject_accum / cpt_reproject_display (they trace `from` into d_id / d_t), by cpt_set_scene
    // (object indices change their meaning) and, with everything else here, by cpt_set_frame, which
    // assigns a fresh Frame: the planes have the old frame's size.
    bool captured = false;
    cpt_camera cam{};
    std::vector<cpt_object> objs;
    // the planes a tracked look-up writes the new frame's id and distance to; swapped with d_id /
    // d_t behind it
    DevBuf<int32_t> d_id_next;
    DevBuf<float> d_t_next;
    // the motion table of the last tracked call after an edit: the host's copies, used by turns,
    // each read by its upload on the stream until its event, and the device's
    std::vector<cpt_object_motion> motion_h[2];
    DevBuf<cpt_object_motion> d_motion;
    DevEvent ev_motion[2];
    int motion_turn = 0;
};

// The top-up render (cpt_capi_topup.cpp; allocated on the frame's first cpt_render_to_count).
struct TopupState {
    DevBuf<uint32_t> d_order;   // the plan's order: every tile, largest deficit first
    DevBuf<uint32_t> d_words;   // the plan's record (cpt_topup.hpp PLAN_*): active tiles, pixels, passes
    bool planned = false;       // a cpt_render_to_count has been queued since cpt_set_frame
};

// Presenting (cpt_capi_present.cpp; allocated on the frame's first cpt_set_exposure,
// cpt_meter_exposure, cpt_read_exposure or cpt_present).
struct PresentState {
    DevBuf<uint8_t> d_bgra;     // the last cpt_present's BGRA8 plane ([npix][4])
    DevBuf<uint32_t> d_words;   // the meter's 257 histogram words, then the exposure's bits (1.0f at first)
    bool presented = false;     // a cpt_present has been queued since cpt_set_frame
};

// Antialiased presentation (cpt_antialias_capi.cpp; allocated on the frame's first
// cpt_aa_coverage).
struct AntialiasState {
    DevBuf<uint4> d_cov;        // a 16-byte coverage word per pixel: nine counts, the flags, padding
    DevBuf<uint32_t> d_list;    // the edge pixels of the last cpt_aa_coverage, in no particular order
    DevBuf<uint32_t> d_count;   // their number, a device word
    int samples = 0;            // S of the last cpt_aa_coverage queued since cpt_set_frame (0: none)
};

// Bloom (cpt_bloom_capi.cpp; allocated on the frame's first cpt_bloom).
struct BloomState {
    DevBuf<float4> d_pyramid;   // levels 1..CPT_BLOOM_MAX_LEVELS one behind the other (cpt_bloom.hpp Pyramid), rgb + 0 per texel
    int levels = 0;             // L of the last cpt_bloom queued since cpt_set_frame (0: none)
};

struct Frame {
    bool set = false, rng_set = false;
    DevBuf<int32_t> d_rows;
    DevBuf<uint32_t> d_rng;
    DevBuf<float4> d_accum;
    DevBuf<float> d_normal, d_depth;
    // rng init (released again once the states are written)
    DevBuf<uint32_t> d_scratch_w, d_scratch_m;
    TileSchedule schedule;
    WavefrontState wavefront;
    DisplayBand display;
    AdaptiveState adaptive;
    FilterState filter;
    GBufferState gbuffer;
    ReprojectState reproject;
    TopupState topup;
    PresentState present;
    AntialiasState antialias;
    BloomState bloom;

    // the first-hit aux pair of a CPT_RENDER_AUX render (or cpt_write_aux) of `npix` pixels
    int ensure_aux(cpt_ctx* c, size_t npix) { return cpt::ctx::ensure_all(c, d_normal, 3 * npix, d_depth, npix); }
};

// A pair of timing events around a subsystem's last launches, once they have been recorded:
// begin(c, s) before the launches on `s`, end(c, s) behind them.  A call that returns between the
// two leaves `recorded` as it was; only end, once t1 is recorded, sets it.
struct TimedSpan {
    DevEvent t0, t1;
    bool recorded = false;

    hipError_t create() {
        const hipError_t e = t0.create();
        return e != hipSuccess ? e : t1.create();
    }
    int begin(cpt_ctx* c, hipStream_t s) {
        using cpt::ctx::fail;
        HIP_TRY(c, hipEventRecord(t0, s));
        return CPT_OK;
    }
    int end(cpt_ctx* c, hipStream_t s) {
        using cpt::ctx::fail;
        HIP_TRY(c, hipEventRecord(t1, s));
        recorded = true;
        return CPT_OK;
    }
};

// ======================================================================================
// Context
// ======================================================================================
struct cpt_ctx {
    int device = 0;
    cpt::LaunchGrid grid;   // the device's CUs, each kernel's blocks per CU, the test hook's cap
    // declared before the buffers and events: destroyed after them
    cpt::ctx::DevStream own_stream;
    hipStream_t user_stream = nullptr;
    TimedSpan t_render;    // the last render, all of it
    DevEvent ev_main;      // after the cost schedule's pilot: the dominant kernel(s) only, to t_render.t1
    TimedSpan t_display;   // the last display kernel (k_denoise_rows)
    TimedSpan t_filter;    // the last cpt_filter_frame's launches
    TimedSpan t_query;     // the last query kernel (cpt_gbuffer, cpt_trace_rays, cpt_pick)
    TimedSpan t_reproject; // the last cpt_reproject_accum's or cpt_reproject_display's launches ...
    DevEvent ev_reproject[2];   // ... and the two points between them: after each G-buffer trace
    bool reproject_tracked = false;   // ... of a tracked call: the trace at `from` did not run
    TimedSpan t_present;   // the last cpt_meter_exposure's or cpt_present's launches
    TimedSpan t_aa;        // the last cpt_aa_coverage's launches behind its G-buffer trace
    TimedSpan t_bloom;     // the last cpt_bloom's launches
    std::string err;

    // scene
    std::vector<cpt_object> objs;
    HostBvh bvh;
    std::vector<Node> lin;             // 9 orders of n_bvh nodes: reference, then octants 0..7
    std::vector<int> pos_of_node;      // BNode -> position in the reference order
    int n_bvh = 0;                     // nodes of the reference order
    int n_walk = 0;                    // nodes of each octant order (walk tree + unbounded leaves)
    int n_wide = 0;                    // 4-wide walk-tree nodes per octant (0: none, binary walk)
    int n_unb = 0;                     // unbounded (platform) leaves at the head of each octant order
    int n_leaves = 0;                  // the wide tree's leaf array (after its compact image)
    std::vector<Mat> mats_h;           // deduplicated materials (host-staged, see Mat)
    std::vector<int> mat_have_tex;     // per material slot: textured?
    std::vector<uint64_t> mat_tex;     // per material slot: texture handle (textured slots)
    std::vector<int> mat_of_obj;       // object index -> material index
    DevBuf<Node> d_nodes;
    DevBuf<Mat> d_mats;
    // reference-order position -> object index (-1: an internal node): what a leaf's rank
    // (Node::miss) names, for the ray queries.  Fixed with the topology: a refit leaves it alone.
    std::vector<int32_t> rank_obj;
    DevBuf<int32_t> d_rank_obj;
    bool scene_set = false;
    // device refit (cpt_update_objects): the plan of both trees (ids: reference tree, then walk
    // tree), parents, heights, each object's walk-tree leaf, the boxes as built
    std::vector<cpt::RefitNode> refit_plan;
    std::vector<int32_t> refit_parent, refit_height, refit_walk_leaf;
    std::vector<cpt::Box6> refit_boxes;
    std::vector<uint8_t> refit_mark;   // scratch of an update batch (all zero between batches)
    int refit_n_ref = 0;
    DevBuf<cpt::RefitNode> d_refit_plan;
    DevBuf<cpt::Box6> d_refit_boxes;
    DevBuf<uint8_t> d_refit_work;   // an update batch: RefitLeaf records, then the dirty node ids
    float last_update_ms = 0.f;     // host wall time of the last cpt_update_objects[_rebuild]

    // material textures (cpt_bind_texture)
    struct Texture { uint64_t handle; DevBuf<uint32_t> d_texels; int w, h, cols, addr, filter; };
    std::vector<Texture> textures;
    DevBuf<TexDesc> d_texdescs;
    DevBuf<int32_t> d_tex_of_mat;

    // environment
    DevBuf<uint32_t> d_env;
    int env_w = 1, env_h = 1, env_cols = 0;

    // frame: the geometry the last cpt_set_frame gave, and what lives and dies with it
    int width = 0, height = 0, n_rows = 0;
    std::vector<int32_t> rows_h;
    uint64_t frame_gen = 0;           // process-unique id of the current frame layout (cpt_set_frame)
    Frame frame;

    DevBuf<uint32_t> d_jumps;    // rng init: the XORWOW jump tables
    DevBuf<unsigned long long> d_stats;
    DevBuf<uint32_t> d_work;
    DevBuf<uint4> d_resume;      // tail consolidation: handed-over chains (HO_SLOT_QUADS x uint4 each)
    float last_kernel_ms = 0.f;
    int last_launches = 0;
    // row-tile gather (cpt_gather_rows): per source context, the frame row each of its rows goes
    // to (a device buffer, rebuilt when either frame changes); a source's rows staged on this
    // device when the pair has no peer path
    struct GatherMap {
        const cpt_ctx* src = nullptr;
        uint64_t src_gen = 0, dst_gen = 0;
        int src_device = -1;
        bool peer = false;
        int mode = -1;   // last gather: CPT_GATHER_SAME_DEVICE / _PEER / _STAGED
        DevBuf<int32_t> d_map;
    };
    std::vector<GatherMap> gather_maps;
    DevBuf<float4> d_gather;
    DevBuf<float> d_gather_stat;   // a staged source's moment planes (planar [4][src npix])
    // ray queries (cpt_trace_rays, cpt_pick): the rays ([n][3] origins, [n][3] directions, [n]
    // tmin) and their results ([n] t, [n][3] normals; ids apart), sized before the launch
    DevBuf<float> d_query_rays, d_query_out;
    DevBuf<int32_t> d_query_id;
    // adaptive rounds (cpt_adaptive_begin / _step): the read-back of a round, {tiles kept, pixels
    // rendered, device error word}, and the event recorded behind it
    cpt::ctx::HostPinned<uint32_t> h_ad_words;
    DevEvent ev_round;
    DevEvent ev_ready;    // a gather's source: its queued work
    DevEvent ev_gathered; // a gather's destination: the stitch done
    DevEvent ev_caller;   // a device copy's caller stream: its queued work
    DevEvent ev_copied;   // a device copy: done on the context's stream
    DevEvent ev_switch;   // cpt_set_stream: the work queued on the stream being left
    // consolidation test hooks (cpt_set_debug_consolidation)
    uint32_t dbg = 0;
    bool force_staged_gather = false;   // gather test hook (cpt_set_debug_gather)
    int keeper_spin_log2 = 0, publish_wait_log2 = 0;
    // persistent-grid test hook (cpt_set_debug_grid; its cap is grid.max_workgroups): 0 = all 64 lanes
    int dbg_lanes_per_wave = 0;

    hipStream_t stream() const { return user_stream ? user_stream : (hipStream_t)own_stream; }
    size_t npix() const { return (size_t)n_rows * width; }
};

namespace cpt {
namespace ctx {

// CPT_ERR_STATE from `who` while an adaptive render is pending on the context (between
// cpt_adaptive_begin and the cpt_adaptive_step that returns 0): its rounds own the frame's buffers.
// CPT_OK otherwise.  The refusal is written here alone; the macro returns it from the caller.
inline int refuse_pending(cpt_ctx* c, const char* who) {
    if (!c->frame.adaptive.pending.on) return CPT_OK;
    return fail(c, CPT_ERR_STATE, "%s: an adaptive render is pending (cpt_adaptive_step until 0)", who);
}
#define CPT_REFUSE_PENDING(ctx, who)                             \
    do {                                                         \
        if (int rc_ = refuse_pending((ctx), (who))) return rc_;  \
    } while (0)

// CPT_ERR_STATE from `who` unless the frame holds every row, 0..height-1 in order (cpt_capi.cpp).
int require_full_frame(cpt_ctx* c, const char* who);
// The milliseconds between a span's two events, behind a cpt_last_*_ms entry: CPT_ERR_INVALID_ARG for
// a NULL c or ms, CPT_ERR_STATE with `nothing_yet` while nothing was recorded; waits for t1 (cpt_capi.cpp).
int last_span_ms(cpt_ctx* c, TimedSpan cpt_ctx::*span, float* ms, const char* nothing_yet);
// The two drains of the context's stream in front of a blocking host copy.  drain: the device made
// current and the stream waited for, the kernels' error word left unread.  sync_checked
// (cpt_capi.cpp): the same, then a device-side error of the work the stream ran is reported (and
// cleared).  Which entry uses which is kept as it grew, on record here:
//   drain         cpt_set_frame, cpt_write_rng, cpt_write_accum, cpt_write_aux, cpt_write_moments,
//                 cpt_write_gbuffer (every write: it replaces what the work before it made),
//                 cpt_read_aux, cpt_get_stats and the three cpt_get_*_counters
//   sync_checked  cpt_synchronize, cpt_render / cpt_render_to_count with CPT_RENDER_SYNC,
//                 cpt_tile_costs, cpt_read_rng, cpt_read_accum, cpt_read_noise, cpt_read_moments,
//                 cpt_read_filtered, cpt_read_gbuffer, cpt_trace_rays, cpt_pick, cpt_read_mix,
//                 cpt_read_display_count, cpt_read_exposure, cpt_read_present, cpt_topup_info,
//                 cpt_debug_read_nodes, cpt_debug_read_tile_order (the top-up list's length)
// The remaining waits are a stream synchronisation alone, behind work the entry itself queued
// (cpt_init_rng, the last cpt_adaptive_step, a display pass with a host frame, cpt_math_batch,
// cpt_selftest_qdiv, cpt_debug_read_tile_order, the scene uploads of cpt_scene.cpp).
inline int drain(cpt_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream()));
    return CPT_OK;
}
int check_device_error(cpt_ctx* c);
int sync_checked(cpt_ctx* c);
// The walk bits a query or a reprojection may pass, and CPT_ERR_INVALID_ARG from `who` for any other.
constexpr uint32_t WALK_FLAGS = CPT_TRAVERSAL_ORDERED | CPT_TRAVERSAL_PLAIN_LEAVES;
inline int walk_flags_only(cpt_ctx* c, const char* who, uint32_t flags) {
    if (!(flags & ~WALK_FLAGS)) return CPT_OK;
    return fail(c, CPT_ERR_INVALID_ARG, "%s: flags 0x%x (only CPT_TRAVERSAL_* bits)", who, flags);
}
// max_depth within 0..MAX_RECURSION_DEPTH_SET; each caller reports it in its own words.
inline bool max_depth_ok(int max_depth) { return max_depth >= 0 && max_depth <= (int)cpt::MAX_RECURSION_DEPTH_SET; }
// A device-to-device copy from one of the context's buffers, ordered against the caller's
// stream without a host wait (cpt_capi.cpp).
int copy_ordered(cpt_ctx* c, void* dst, const void* src, size_t bytes, hipStream_t caller);
// What cpt_render, cpt_tile_costs and cpt_adaptive_begin ask before they launch, in this order:
// a scene, a frame with RNG states, a camera of the frame's size (the messages start with `who`).
// max_depth (0..32) each of them checks with its own arguments, before this.
int renderable(cpt_ctx* c, const cpt_camera* cam, const char* who);
// What a megakernel launch of the context's frame is made of (cpt_capi_render.cpp; shared with
// cpt_capi_adaptive.cpp): the kernel parameters, the frame's 8x8 tiles, the cost schedule's pilot
// into TileSchedule::d_cost_order and its length for a render of `spp` passes, the consolidation slab.
void fill_params(cpt_ctx* c, const cpt_camera* cam, int spp, int max_depth, uint32_t flags, cpt::KParams& p);
size_t n_tiles(const cpt_ctx* c);
int cost_pilot_passes(int spp);
int cost_pilot(cpt_ctx* c, const cpt::KParams& p, int passes, hipStream_t s);
int consolidation_slab(cpt_ctx* c, cpt::KParams& p, int spp, uint32_t flags);

// cpt_capi_present.cpp, shared with cpt_antialias_capi.cpp and cpt_bloom_capi.cpp.  present_source: what every presenting
// call asks of the context before it writes anything (a frame, no adaptive render pending and, for
// the filtered source, a filter result); *src: the source plane.  present_state: the frame's
// present state, allocated and initialised on the stream at its first call (histogram 0, exposure 1).
int present_source(cpt_ctx* c, const char* who, int source, const float4** src);
int present_state(cpt_ctx* c);

// cpt_scene.cpp
int material_slot(cpt_ctx* c, const cpt_material& m);
void linearise_all(cpt_ctx* c);
int upload_scene(cpt_ctx* c);
int upload_materials(cpt_ctx* c);
int device_refit(cpt_ctx* c, int n, const int* indices, bool mats_changed);

}  // namespace ctx
}  // namespace cpt
