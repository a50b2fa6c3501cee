// cpt_internal.hpp — shared between the HIP kernels and the C-ABI implementation.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "cpt_device.hpp"
#include "cpt_tuning.hpp"

// Per-lane LDS stack entries of the wide walk; the host keeps the binary walk for a tree that
// could need more (cpt_host_bvh.cpp linearise_wide).
#define CPT_WSTACK 32

namespace cpt {

// Wide-tree nodes staged in LDS by the LDS kernels (cpt_path.hpp trace_wide); the host numbers
// a larger tree so that these are its top (cpt_host_bvh.cpp linearise_wide).
constexpr int LDS_TREE_NODES = 512;
__host__ __device__ __forceinline__ int lds_tree_nodes(int n_wide) { return n_wide < LDS_TREE_NODES ? n_wide : LDS_TREE_NODES; }

// uint4s of KParams::resume per handed-over chain (k_megakernel's hand-over payload: 17 words).
constexpr int HO_SLOT_QUADS = 5;
// Hand-over slots per workgroup of BLK lanes: each of the waves of levels 1.. retires once and
// hands over at most its 64 chains, so (levels - 1) x 256 slots always suffice.
template <int BLK> constexpr int ho_slots() { return (BLK / 256 - 1) * 256; }

// Camera snapshot as the kernel needs it (the reference passes the whole MotionalCamera by
// value in PathTracerParams, path_tracer.cu:14-27; only these fields are read by RayGen).
struct CamK {
    float origin[3];
    float u[3], v[3];
    float top_left[3], horizontal[3], vertical[3];
    float lens_radius;
    int width, height;
    double inv_w, inv_h;   // 1.0 / (double)(float)width, height: RayGen's x / width, y / height as
                           // exact quotients (cpt_path.hpp ray_gen)
};

// Kernel arguments (passed by value: they land in the kernarg segment and are read with
// scalar loads).
struct KParams {
    const Node* nodes;      // skip-link orders, leaves inline: the reference order (n_nodes), then
                            // the walk tree's eight octant orders (n_walk each)
    const Mat* mats;        // deduplicated materials, indexed by Node::code >> 2
    int n_nodes, n_walk;
    int n_wide;             // 4-wide walk-tree nodes: their compact image follows the eight octant
                            // orders (0: the ordered walk uses the binary octant orders)
    int n_unb;              // unbounded leaves at the head of every octant order
    int n_leaves;           // the wide tree's leaf array (platforms first), after its compact image
    int ordered;            // CPT_TRAVERSAL_ORDERED: walk the ray's octant order (2: plain leaves)
    const uint32_t* env;    // packed RGBA8, env_cols x env_h
    int env_w, env_h, env_cols;
    CamK cam;
    const int32_t* rows;    // global row index per context row
    int n_rows, width;
    uint32_t* rng;          // planar [6][n_rows*width]
    float4* accum;          // [n_rows*width] rgb sums + pass count
    float* normal;          // [n_rows*width][3] (AUX)
    float* depth;           // [n_rows*width]    (AUX)
    unsigned long long* stats;  // [5]           (STATS)
    uint32_t* work;         // pixel dequeue counter (zeroed before each launch)
    const uint32_t* tile_order;  // megakernel dequeue order of the 8x8 tiles (nullptr: row-major)
    // One pointer slot, two launches that never coincide (a TOPUP kernel is never a PROBE kernel):
    union {
        uint32_t* tile_cost;           // pilot launch only: per-tile work (cost schedule)
        // Top-up launch only (cpt_render_to_count, the TOPUP kernels): the device word that holds
        // how many entries of tile_order have a deficit (cpt_topup.hip's plan); they alone are
        // dequeued.  spp is then the target, a lane's passes its pixel's deficit (cpt_topup.hpp).
        // In the pilot's slot, not appended: a longer KParams moves the hidden arguments of every
        // kernel that takes one, and the explicit ones behind it, by 8 bytes.
        const uint32_t* topup_active;
    };
    int spp, max_depth, accumulate;
    int lanes;              // lanes per wave that take pixels (64; fewer: DIAGNOSTIC CPT_LANES_PER_WAVE)
    int replicate;          // lanes per taken pixel (1; more: DIAGNOSTIC CPT_REPLICATE, identical copies)
    // Tail consolidation (LDS walk only; nullptr: off): slabs of chains handed over at a pass
    // boundary by retiring waves, HO_SLOT_QUADS x uint4 per chain, ho_slots chains per workgroup.
    uint4* resume;
    size_t resume_cap;      // chains (all workgroups)
    // Sticky device error word (CPT_DEVERR_*), or-ed by a kernel that had to abandon work; the
    // host reads and clears it at its next synchronising call (cpt_capi.cpp check_device_error).
    uint32_t* error;
    // Test hooks of the consolidation's error paths (cpt_set_debug_consolidation; 0 in normal
    // use): dbg bit 0 = a phantom live chain in every workgroup (a lost count), bit 1 = hand-overs
    // never publish their slot; the keeper's idle-spin limit and the hand-over wait as log2
    // (0 = the defaults, 2^26 and 2^22).
    uint32_t dbg;
    int keeper_spin_log2, publish_wait_log2;
    // Adaptive render (cpt_render_adaptive): only the first n_active entries of tile_order are
    // dequeued (tiles still noisy); 0 = every tile of the frame, as every other launch passes.
    uint32_t n_active;
};

// The wide walk (the ordered walk on a 4-wide tree) runs in the LDS kernels: the image's first
// LDS_TREE_NODES nodes in LDS, the rest of a larger tree from global memory.  The launchers pick
// the LDST kernels by this, and trace_segment's LDST branch walks by it.
__host__ __device__ __forceinline__ bool use_lds_tree(const KParams& p) { return p.ordered == 1 && p.n_wide > 0; }

// Device error bits (KParams::error).
enum : uint32_t {
    CPT_DEVERR_KEEPER_TIMEOUT = 1u,    // a keeper wave gave up waiting while chains were live
    CPT_DEVERR_PUBLISH_TIMEOUT = 2u,   // a taken hand-over slot was never published (chain lost)
    CPT_DEVERR_RESUME_CAP = 4u,        // consolidation slab too small for the grid
};

// Who sizes a persistent launch: the context's LaunchGrid, the one source of the
// device's CU count, each kernel's blocks per CU and the test hook's cap.  Host code.
// The arithmetic, pure (cpt_launch_grid_host runs it without a GPU).  The workgroups of `block`
// lanes the megakernel wants for `tiles` 8x8 tiles: a lane per pixel id, a wave holding
// lanes / replicate pixels at once (64 in normal use; fewer: DIAGNOSTIC).
inline long long megakernel_want(long long tiles, int lanes, int replicate, int block) {
    const int per_wave = std::max(1, lanes / std::max(1, replicate));
    return (tiles * 64 * ((64 + per_wave - 1) / per_wave) + block - 1) / block;
}
// A launch that wants `want` workgroups gets every resident slot at most once, then at most
// max_workgroups (TEST HOOK cpt_set_debug_grid; 0: no cap).  0: launch nothing.
inline int grid_workgroups(long long want, long long resident, int max_workgroups) {
    const long long grid = std::min(want, resident);
    return (int)std::max(0LL, max_workgroups > 0 ? std::min<long long>(grid, max_workgroups) : grid);
}
// The chains of the hand-over slab (consolidation_slab): ho_slots for each resident workgroup.
inline size_t consolidation_chains(long long resident) { return (size_t)ho_slots<LDS_BLOCK>() * (size_t)resident; }

struct LaunchGrid {
    int cus = 1;              // the device's compute units (read once, cpt_create)
    int max_workgroups = 0;   // TEST HOOK cpt_set_debug_grid: the megakernel's cap (0: none)

    // Resident workgroups of kernel `fn` at `block` lanes: its blocks per CU x the CUs.  The
    // occupancy is asked on the kernel's first launch in this context (whose device is current:
    // every entry point sets it) and kept; a failed query is the caller's HIP error.
    hipError_t resident(const void* fn, int block, long long* out) {
        auto it = std::find_if(per_cu.begin(), per_cu.end(), [fn](const auto& k) { return k.first == fn; });
        if (it == per_cu.end()) {
            int n = 0;
            const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, block, 0);
            if (e != hipSuccess) return e;
            it = per_cu.insert(it, {fn, std::max(n, 1)});
        }
        *out = (long long)it->second * cus;
        return hipSuccess;
    }
    // Workgroups for a launch of `fn` that wants `want`; `hooked`: the cap applies (the megakernel
    // and its pilot; the wavefront path ignores the hook).
    hipError_t size(const void* fn, int block, long long want, bool hooked, int* out) {
        long long r = 0;
        const hipError_t e = resident(fn, block, &r);
        if (e == hipSuccess) *out = grid_workgroups(want, r, hooked ? max_workgroups : 0);
        return e;
    }

private:
    std::vector<std::pair<const void*, int>> per_cu;   // blocks per CU of each kernel launched so far
};

// Cost schedule (cpt_schedule.hip, DESIGN.md §Cost schedule): a `passes`-pass pilot of the
// megakernel sums each 8x8 tile's work, then `order` (one u32 per tile) gets the tiles
// heaviest first.  `scratch` holds tile_schedule_scratch_bytes() bytes.
size_t tile_schedule_scratch_bytes(int width, int n_rows);
hipError_t launch_cost_pilot(const KParams& p, LaunchGrid& grid, hipStream_t stream);   // cpt_megakernel.hip: the pilot's launch
// CPT_SCHEDULE_PREVIOUS: each 8x8 tile's RNG draws since `d_prev` (the Weyl plane d of the
// states, planar [5] of p.rng), then d_prev := d; the tiles sorted heaviest first into `order`.
hipError_t launch_tile_order_from_draws(const KParams& p, uint32_t* d_prev, void* scratch, size_t scratch_bytes,
                                        uint32_t* order, hipStream_t stream);
hipError_t launch_tile_schedule(const KParams& p, int passes, void* scratch, size_t scratch_bytes, uint32_t* order,
                                LaunchGrid& grid, hipStream_t stream);

// Adaptive render (cpt_adaptive.hip, DESIGN.md §Adaptive sampling).  After a round of `batch`
// passes over the first n_active tiles of `order` (nullptr: tiles 0..n_active-1), launch_tile_noise
// folds the round's batch mean of every pixel of those tiles into its moments (cpt_adaptive.hpp),
// copies the accumulator into the snapshot and writes keep[i] for each list position i: 0 when the
// tile leaves the list (all its pixels converged in an `eligible` round, or the `last` round).
struct AdaptiveRound {
    const uint32_t* order;
    uint32_t n_active;
    int width, n_rows;
    const float4* accum;    // [n_rows*width] after the round
    float4* snap;           // [n_rows*width] before the round; after it on return
    float* stat;            // planar [4][n_rows*width]: m1, m2, k, rel (the noise map)
    uint32_t* keep;         // [n_active]
    float rel_error;
    int eligible, last;
};
hipError_t launch_tile_noise(const AdaptiveRound& a, hipStream_t stream);
// dst := the kept entries of src (nullptr: 0..n-1) in their order (a stable compaction);
// out[0] = their number, out[1] = the frame pixels of the n tiles of the input list.
hipError_t launch_compact_order(const uint32_t* src, const uint32_t* keep, uint32_t n, int width, int n_rows,
                                uint32_t* dst, uint32_t* out, hipStream_t stream);

// The a-trous filter of cpt_filter_frame (cpt_filter.hip).  launch_filter_prepare:
// plane[i] = (mean rgb, variance of the mean) and ok[i] = validity of pixel i, from the accumulator
// and the adaptive moments `stat` (planar [4][npix]).  launch_filter_level: one level at `step`
// from plane `in` into plane `out` (sig2 = sigma_l squared); normal3 and ok are only read.
hipError_t launch_filter_prepare(const float4* accum, const float* stat, size_t npix, float4* plane, uint8_t* ok,
                                 hipStream_t stream);
hipError_t launch_filter_level(const float4* in, const float* normal3, const uint8_t* ok, float4* out, int width, int height,
                               int step, float sig2, int sharpness_log2, hipStream_t stream);
// The same filter without moments (cpt_filter_frame_spatial).
// launch_filter_prepare_spatial: plane and ok from the accumulator and the G-buffer's id and normal
// planes, the variance from the 7x7 window.  launch_filter_level_id: launch_filter_level with the
// stop at object boundaries, a tap of another `id` being skipped.
hipError_t launch_filter_prepare_spatial(const float4* accum, const int32_t* id, const float* normal3, int width, int height,
                                         int sharpness_log2, float4* plane, uint8_t* ok, hipStream_t stream);
hipError_t launch_filter_level_id(const float4* in, const float* normal3, const int32_t* id, const uint8_t* ok, float4* out,
                                  int width, int height, int step, float sig2, int sharpness_log2, hipStream_t stream);

// Wavefront path state (cpt_wavefront.hip): SoA float4 arrays indexed by QUEUE SLOT + queues.
// The carried state is double-buffered: bounce b reads buffer b & 1 at its queue slot and shade
// writes each surviving path into buffer (b + 1) & 1 at the slot the compaction gave it, so
// every state access is coalesced.  Hit records are per slot of the current bounce.
struct WfState {
    float4 *ray_o[2], *ray_d[2], *att[2], *rad[2], *aux[2];
    float4 *hit_p, *hit_n;
    uint4* rng_a[2];      // a live path's XORWOW state by slot: (v0, v1, v2, v3) ...
    uint2* rng_b[2];      // ... and (v4, d); back in the per-pixel planes when the path ends
    int32_t* queue[2];
    int32_t* ident;       // tile-ordered identity queue (first bounce)
    uint32_t* counts;     // [0], [1]: queue sizes; [3]: ident size
};

// Device refit of cpt_update_objects (SceneBVH::UpdateObject, bvh.cu:122-157, on the GPU).  The
// reference tree's nodes and the walk tree's nodes are numbered together ("refit ids": the
// reference tree's BNodes first, then the walk tree's); each records where its copies live in
// the node buffer.  The topology is fixed until the next cpt_set_scene.
struct RefitNode {
    int32_t left, right;    // children (refit ids); a leaf has left = -1
    int32_t slot;           // 4-wide image slot holding this node's box (wide id * 4 + k), or -1
    int32_t leaf;           // index in the wide tree's leaf array (walk-tree leaves), or -1
    int32_t pos[8];         // node-buffer index of each copy: the reference order (pos[0]) or the
                            // octant orders 0..7 of the walk tree (octant form); -1: none
};
struct Box6 { float lo[3], hi[3]; };
// One updated object: its inline primitive (Node::miss is not written: each copy keeps its own)
// and its box (Object::GetAABBMin/Max), for its leaf in each tree.
struct RefitLeaf {
    Node prim;
    Box6 box;
    int32_t ref_id, walk_id;
};
// The leaves, then the dirty internal nodes height by height (children before parents): one
// launch of k_refit_leaves, one of k_refit_nodes per height.  n_ref: reference-tree ids are
// [0, n_ref); `image` / `leaves` are the wide tree's compact image and leaf array (nullptr: none).
hipError_t launch_refit(const RefitLeaf* leaves_in, int n_leaves, const int32_t* dirty, const int32_t* level_end,
                        int n_levels, int n_ref, const RefitNode* nodes_plan, Box6* boxes, Node* nodes, uint32_t* image,
                        Node* leaves, hipStream_t stream);

hipError_t launch_megakernel(const KParams& p, bool stats, bool aux, LaunchGrid& grid, hipStream_t stream);
// The top-up launch (p.topup_active and p.tile_order from the plan, p.spp the target): the TOPUP
// kernels, never consolidating, on a grid sized for the whole frame.
hipError_t launch_megakernel_topup(const KParams& p, bool stats, bool aux, LaunchGrid& grid, hipStream_t stream);
// The resident workgroups of the consolidating kernel such a launch runs (consolidation_slab).
hipError_t consolidating_workgroups(const KParams& p, bool stats, bool aux, LaunchGrid& grid, long long* out);
hipError_t launch_wavefront(const KParams& p, WfState& w, bool stats, bool aux, LaunchGrid& grid, hipStream_t stream,
                            int* launches);
hipError_t wavefront_build_ident(const KParams& p, WfState& w, hipStream_t stream);
hipError_t launch_prepare_materials(Mat* mats, const int32_t* tex_of_mat, const TexDesc* texs, int n,
                                    hipStream_t stream);
hipError_t launch_init_rng(const uint32_t* jumps, const uint32_t seed_state[6], int width, const int32_t* rows,
                           int n_rows, uint32_t* scratch_w, uint32_t* scratch_mats, uint32_t* rng, hipStream_t stream);
hipError_t launch_math_batch(int op, const float* a, const float* b, float* out, size_t n, hipStream_t stream);
hipError_t launch_stream_read(const float4* p, size_t n, float* out, int grid, hipStream_t stream);
hipError_t launch_read_pattern(int bpl, const float* p, size_t n_lanes, float* out, int grid, hipStream_t stream);
hipError_t timeline_read(unsigned long long* out, int n, hipStream_t stream);
hipError_t launch_selftest_qdiv(int which, uint64_t n, uint64_t seed, unsigned long long* out, int out_len,
                                hipStream_t stream);
hipError_t launch_selftest_dn_weight(int which, uint64_t n, unsigned long long* out, int out_len, hipStream_t stream);
hipError_t launch_stitch_rows(const float4* src_acc, const float* src_nrm, const float* src_dep, const int32_t* dst_row,
                              int width, int n_rows, float4* acc, float* nrm, float* dep, hipStream_t stream);
// The gather's moments (cpt_display.hip): the four planes of `src` (planar [4][src_npix], n_rows
// rows of `width`) to rows dst_row[r] of `dst` (planar [4][dst_npix]).
hipError_t launch_stitch_moments(const float* src, size_t src_npix, const int32_t* dst_row, int width, int n_rows,
                                 float* dst, size_t dst_npix, hipStream_t stream);
// out_host (nullable): the device alias of a pinned host frame, written beside `out`; accum /
// normal / depth hold the context's ctx_rows rows from row0; sink: a
// device buffer of DN_SINK_SLOTS float4s the strip kernel's lanes without an output pixel store to
constexpr int DN_SINK_SLOTS = 1024 * 64;
// count == nullptr: Mix at 1 / cur_sample_idx; else the per-pixel Mix on that count plane (beside
// mix, one float per pixel), which does not read cur_sample_idx
hipError_t launch_denoise_mix(const float4* accum, const float* normal, const float* depth, float* mix, float* count,
                              uint8_t* out, uint8_t* out_host, float4* sink, int width, int height, int row0, int ctx_rows, int y0,
                              int y1, uint32_t cur_sample_idx, const LaunchGrid& grid, hipStream_t stream);
// `value` into the first w_eff columns of `rows` rows of a count plane of `width` columns
hipError_t launch_fill_count(float* count, int width, int w_eff, int rows, float value, hipStream_t stream);

// Presenting (cpt_present.hip).  `src`: the accumulator or a filter plane, npix
// float4; `words`: the 257 histogram words, then the exposure's bits.  launch_meter zeroes the
// histogram on the stream, fills it (at most `cus` x 4 workgroups) and resolves it into the
// exposure with a second, one-workgroup launch.  launch_present reads the exposure and writes bgra
// ([npix][4] bytes, 16-byte aligned).
hipError_t launch_meter(const float4* src, size_t npix, int source, float key, int permille, float adapt, uint32_t* words,
                        int cus, hipStream_t stream);
hipError_t launch_present(const float4* src, size_t npix, int source, int tone, float white, int transfer,
                          const uint32_t* words, uint8_t* bgra, hipStream_t stream);

}  // namespace cpt
