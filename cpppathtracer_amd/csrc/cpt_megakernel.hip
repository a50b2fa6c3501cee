// cpt_megakernel.hip — the persistent megakernel of the MI355X integrator (gfx950, wave64).
//
//   k_megakernel         SamplePixel (path_tracer.cu:124-175), all spp passes per launch,
//                        per-lane path regeneration, state in registers; with what it alone
//                        uses: Lane, decode_pixel, the coherent load/store helpers
//                        and the hand-over queue of the tail consolidation
//   launch_mk*           the STATS / AUX / PROBE / LDS / CONS / HYB / TOPUP ladder; each launch is sized
//                        by the context's LaunchGrid (cpt_internal.hpp)
//   launch_megakernel    the render's entry;  launch_cost_pilot: the cost schedule's pilot;
//                        launch_megakernel_topup: the top-up render's (the TOPUP kernels)
//   timeline_read        the CPT_TIMELINE read-out (timeline::g_tl is per translation unit)
//   k_prepare_materials  per-material constants: GetKd(0,0), emission, 1/alpha — material.cu:43-45,
//                        69-70, 103-104; here because its register assignment depends on the unit
//
// Reference semantics per function are cited inline; DESIGN.md has the data layout and the
// roofline of each kernel.  Out of the round as named pieces so far: HoPayload (the
// hand-over slot's one layout), finish_pixel, and in cpt_path.hpp stage_wide_tree, ray_is_finite,
// load_rng / store_rng and flush_walk_counters; refill, hand-over queue and sky are still inline.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "cpt_path.hpp"
#include "cpt_topup.hpp"

namespace cpt {

// ======================================================================================
// k_megakernel — SamplePixel (path_tracer.cu:124-175) for `spp` consecutive passes, as a
// persistent kernel.
//
// A lane owns one pixel at a time: the pixel's XORWOW state, path state and pass
// accumulator stay in VGPRs; HBM is touched once when the lane takes the pixel (24 B rng +
// 16 B accumulator) and once when it has run all `spp` passes.  A lane whose path ends
// starts the pixel's next pass at once; a lane whose pixel is finished takes the next pixel
// from a device-wide counter (a wave draws 64 ids per atomic, see the refill), so every lane of
// every wave does useful work until the image runs out — no per-pass kernel boundaries and
// no idle lanes behind a wave's slowest path.  Pixels are handed out in 8x8 tiles so a fresh
// wave starts coherent; with the cost schedule the tiles come heaviest first (p.tile_order).
//
// PROBE (the cost schedule's pilot, DESIGN.md §Cost schedule): the same passes from the same
// RNG states, but nothing is written back except each pixel's work (segments + node visits +
// primitive tests), whose maximum over the tile's pixels is the tile's cost.
// ======================================================================================
// TAIL CONSOLIDATION (LDS walk, p.resume != nullptr).  Once the pixel
// queue is drained, chains finish and the waves thin out, but every wave keeps its SIMD slot
// until its last lane is done: in the tail of a frame (and for all of it when a rank holds
// about one pixel per lane) a few live lanes in each of four waves per SIMD share the SIMD,
// and a chain's segment takes ~30 us instead of the ~17 us of a wave alone on its SIMD.  So
// the block's 16 waves are ranked in four levels of four (one wave per SIMD each, by wave
// index); when the chains still live fit into the waves of the levels below l, the waves of
// level l retire: each lane, at the end of its current pass, hands its chain over (RNG state,
// running sum, passes left: the pass boundary needs no path state) through a queue, and the
// waves of the lower levels take those chains into their idle lanes.  Level 0 never retires
// and takes hand-overs until no chain of its workgroup is live.  A chain's passes run in the
// same order from the same state wherever they run, so the image is unchanged.
// Everything is per workgroup (one per CU): the live count and the queue's head, tail and
// publication flags are LDS words, the payloads a per-workgroup slab in HBM, so the waves of a
// CU consolidate among themselves without device-wide traffic (a device-wide queue measured
// 20-40% slower at 1-4 pixels per lane from its polling and contended CAS).  Payloads are
// coherent (sc1) loads and stores, ordered before the flag by waiting for the stores.
__device__ __forceinline__ uint32_t ld_coherent(const uint32_t* a) {
    return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_coherent(uint32_t* a, uint32_t v) {
    __hip_atomic_store(a, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wait_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

struct Lane {
    uint32_t xy;     // x | y << 16 (frames are < 65536 pixels wide and high)
    uint32_t pix;    // context pixel index (frames are < 2^32 pixels)
    uint32_t tile;
    Xorwow s;
    v3 sum;
    float passes;
    int left;
    // the pixel's state from HBM: its XORWOW words (planar [6][npix]) and its accumulator (ACC: the
    // render, if it accumulates; p.accumulate is read after the RNG loads are issued)
    template <bool ACC>
    __device__ __forceinline__ void load(const KParams& p, size_t npix) {
        load_rng(p, npix, pix, s);
        const float4 a = (p.accumulate && ACC) ? p.accum[pix] : make_float4(0.f, 0.f, 0.f, 0.f);
        sum = mk(a.x, a.y, a.z);
        passes = a.w;
    }
};

// A lane's pending sky fetch in LDS (its column of pending_q, nine floats at a stride of BLK):
// direction, the pass's radiance and attenuation so far.
template <int BLK>
struct PendingSky {
    float* q;
    __device__ __forceinline__ void park(const v3& dir, const v3& rad, const v3& att) const {
        q[0 * BLK] = dir.x; q[1 * BLK] = dir.y; q[2 * BLK] = dir.z;
        q[3 * BLK] = rad.x; q[4 * BLK] = rad.y; q[5 * BLK] = rad.z;
        q[6 * BLK] = att.x; q[7 * BLK] = att.y; q[8 * BLK] = att.z;
    }
    __device__ __forceinline__ v3 dir() const { return mk(q[0 * BLK], q[1 * BLK], q[2 * BLK]); }
    __device__ __forceinline__ v3 rad() const { return mk(q[3 * BLK], q[4 * BLK], q[5 * BLK]); }
    __device__ __forceinline__ v3 att() const { return mk(q[6 * BLK], q[7 * BLK], q[8 * BLK]); }
};

// A hand-over slot's payload, the chain at a pass boundary (HO_SLOT_QUADS x 16 B in the slab):
// pix, xy, the six RNG words, sum, passes, the first normal and a spare word (AUX only), passes
// left; moved by coherent (sc1) stores / loads of the words in use, in word order.
struct HoPayload {
    static constexpr int WORDS = 17;
    static_assert(WORDS <= 4 * HO_SLOT_QUADS, "a slot holds the payload");
    template <bool AUX> static constexpr bool used(int k) { return AUX || k < 12 || k == 16; }
    template <bool AUX>
    __device__ __forceinline__ static void store(uint32_t* e, const Lane& L, const v3& first_normal) {
        const uint32_t w[WORDS] = {L.pix, L.xy, L.s.v0, L.s.v1, L.s.v2, L.s.v3, L.s.v4, L.s.d,
                                   __float_as_uint(L.sum.x), __float_as_uint(L.sum.y), __float_as_uint(L.sum.z),
                                   __float_as_uint(L.passes), __float_as_uint(first_normal.x),
                                   __float_as_uint(first_normal.y), __float_as_uint(first_normal.z), 0u, (uint32_t)L.left};
#pragma unroll
        for (int k = 0; k < WORDS; ++k)
            if (used<AUX>(k)) st_coherent(e + k, w[k]);
    }
    template <bool AUX>
    __device__ __forceinline__ static void load(const uint32_t* e, Lane& L, v3& first_normal) {
        uint32_t w[WORDS];
#pragma unroll
        for (int k = 0; k < WORDS; ++k) w[k] = used<AUX>(k) ? ld_coherent(e + k) : 0u;
        L.pix = w[0]; L.xy = w[1]; L.s.v0 = w[2]; L.s.v1 = w[3]; L.s.v2 = w[4]; L.s.v3 = w[5]; L.s.v4 = w[6]; L.s.d = w[7];
        L.sum = mk(__uint_as_float(w[8]), __uint_as_float(w[9]), __uint_as_float(w[10]));
        L.passes = __uint_as_float(w[11]);
        if (AUX) first_normal = mk(__uint_as_float(w[12]), __uint_as_float(w[13]), __uint_as_float(w[14]));
        L.left = (int)w[16];
    }
};
__device__ __forceinline__ uint32_t* ho_slot(uint4* slab, uint32_t slot) {
    return reinterpret_cast<uint32_t*>(slab + HO_SLOT_QUADS * (size_t)slot);
}

// A finished chain: the pilot's cost (PROBE), or the write-back (path_tracer.cu:172-174).
template <bool AUX, bool PROBE>
__device__ __forceinline__ void finish_pixel(const KParams& p, const Lane& L, const v3& first_normal, uint32_t work_at_take,
                                             const Counters& cnt, size_t npix, uint32_t max_depth) {
    if (PROBE) {
        // the tile's key is its heaviest pixel's work, not the tile's sum (round 6): one long
        // chain in an otherwise light tile must start with the first tiles, not in the tail
        // (tools/timeline.py: C5 N = 8, the rank's last quarter ran a few hundred such chains)
        atomicMax(&p.tile_cost[L.tile], cnt.segments + cnt.nodes + cnt.prims - work_at_take);
        return;
    }
    execdiag::lanes(p.stats + 64, 11);
    p.accum[L.pix] = make_float4(L.sum.x, L.sum.y, L.sum.z, L.passes);
    if (AUX && p.spp > 0) {
        p.normal[3 * (size_t)L.pix + 0] = first_normal.x;
        p.normal[3 * (size_t)L.pix + 1] = first_normal.y;
        p.normal[3 * (size_t)L.pix + 2] = first_normal.z;
        p.depth[L.pix] = max_depth > 0 ? DEFAULT_RAY_TMAX : 0.f;   // a18
    }
    store_rng(p, npix, L.pix, L.s);
}

__device__ __forceinline__ bool decode_pixel(const KParams& p, uint32_t id, int& x, int& ri, uint32_t& tile) {
    tile = id >> 6;
    if (p.tile_order) tile = p.tile_order[tile];
    return TileGrid{p.width, p.n_rows}.pixel(tile, id & 63, x, ri);
}

// Scheduling constants (SUSPEND_AT, STATIC_FIRST, DEFER_MISS_ROUND, CPT_LDS_BLOCK): cpt_tuning.hpp.

// LDST: the 4-wide walk tree's compact image (its first LDS_TREE_NODES nodes: the top of the
// tree) is staged in LDS once per workgroup, and the walk reads those nodes there (a lane's
// node loads become ds_read_b128s: LDS latency instead of L1/L2 latency on every dependent
// step of the walk); a larger tree's other nodes come from the image in global memory.
// One LDS workgroup per CU: 16 waves, 4 per SIMD (the image, the 16-bit stacks and the pending
// sky fetches take 156 KB of the CU's 160 KB), which caps the kernel at 128 VGPRs.
template <bool LDST> constexpr int mk_block() { return LDST ? LDS_BLOCK : 256; }
template <bool LDST> constexpr int mk_waves() { return LDST ? LDS_BLOCK / 256 : WAVES_PER_SIMD; }

// HYB (LDST): the wide tree has more nodes than the LDS image holds; the rest are read from
// global memory (cpt_path.hpp load_wide_node).
// TOPUP (cpt_render_to_count): a lane's passes are its pixel's deficit to the target
// p.spp (cpt_topup.hpp), read from the accumulator at the take; a pixel without one is neither
// loaded nor written.  Only the first *p.topup_active tiles of p.tile_order are dequeued.
template <bool STATS, bool AUX, bool PROBE, bool LDST, bool CONS, bool HYB, bool TOPUP = false>
__global__ void __launch_bounds__(mk_block<LDST>(), mk_waves<LDST>()) k_megakernel(const KParams p) {
    static_assert(!TOPUP || (!PROBE && !CONS), "a top-up launch writes its pixels and never consolidates");
    constexpr bool COUNT = STATS || PROBE;
    constexpr int BLK = mk_block<LDST>();
    __shared__ uint4 s_tree[LDST ? LDS_TREE_NODES * 7 : 1];
    pooldiag::init();
    if (LDST) stage_wide_tree<BLK>(s_tree, p);
    const int lane = threadIdx.x & 63;
    const size_t npix = (size_t)p.n_rows * p.width;
    // (an adaptive render's later rounds dequeue only the first n_active tiles of p.tile_order)
    // (a top-up launch: the tiles with a deficit, counted on the device by the plan before it)
    const uint32_t n_work =
        (TOPUP ? *p.topup_active : (p.n_active ? p.n_active : (uint32_t)TileGrid{p.width, p.n_rows}.count())) * 64u;
    const uint32_t max_depth = (uint32_t)p.max_depth;
    Counters cnt{};
    uint32_t work_at_take = 0;   // PROBE: the lane's counters when it took its pixel

    Lane L;
    bool busy = false;
    bool exhausted = false;      // wave-uniform: the counter ran past n_work
    Ray ray;
    v3 att = mk1(1.f), rad = mk1(0.f);
    uint32_t depth = 0;
    bool first = true;
    // AUX: the first hit's normal of the lane's latest pass (path_tracer.cu:160-163: summed into
    // zeroed accumulators on the pass's first segment only, so 0 + n); its depth is always
    // DEFAULT_RAY_TMAX (a18: TraceRay took the ray by value), written as that constant
    v3 first_normal = mk1(0.f);

    // a lane's pending sky fetch: direction, the pass's radiance and attenuation so far
    __shared__ float pending_q[DEFER_MISS_ROUND > 0 ? 9 * BLK : 1];
    const PendingSky<BLK> pq{pending_q + threadIdx.x};
    bool pend = false;
    WalkState ws;          // the lane's suspended walk, if any
    ws.active = false;
    // tail consolidation (see above): this wave's level, the lanes one level holds over the grid
    static_assert(!CONS || (LDST && !PROBE && ho_slots<BLK>() > 0), "consolidation needs the LDS walk");
    constexpr int QS = CONS ? ho_slots<BLK>() : 1;
    // hand-over queue head, tail; the workgroup's live chains (taken, not finished, counted
    // before the taking wave can be seen exhausted); its waves still taking pixels
    __shared__ uint32_t s_q[CONS ? 4 : 1];
    __shared__ uint8_t s_qflag[QS];          // slot published
    const bool cons = CONS && (size_t)(blockIdx.x + 1) * QS <= p.resume_cap;
    if (CONS && !cons && threadIdx.x == 0) atomicOr(p.error, CPT_DEVERR_RESUME_CAP);   // runs unconsolidated
    uint4* const qslab = cons ? p.resume + HO_SLOT_QUADS * (size_t)blockIdx.x * QS : nullptr;
    volatile uint32_t* const vq = s_q;
    const uint32_t level = __builtin_amdgcn_readfirstlane((uint32_t)(threadIdx.x >> 8));
    bool retiring = false;       // wave-uniform: hand every chain over at its next pass end
    uint32_t idle_spins = 0;
    const uint32_t keeper_spins = 1u << (p.keeper_spin_log2 > 0 ? p.keeper_spin_log2 : 26);
    const uint32_t publish_wait = 1u << (p.publish_wait_log2 > 0 ? p.publish_wait_log2 : 22);
    if (cons) {
        if (threadIdx.x < 4)
            s_q[threadIdx.x] = threadIdx.x == 3 ? (uint32_t)(BLK / 64) : (threadIdx.x == 2 ? (p.dbg & 1u) : 0u);
        for (int i = threadIdx.x; i < QS; i += BLK) s_qflag[i] = 0;
        __syncthreads();
    }
    // a chain's next pass (RayGen, path_tracer.cu:134)
    auto start_pass = [&]() {
        ray = ray_gen(kernarg_field<CamK>(offsetof(KParams, cam)), (int)(L.xy & 0xffffu), (int)(L.xy >> 16), L.s);
        att = mk1(1.f);
        rad = mk1(0.f);
        depth = 0;
        first = true;
    };
    // STATIC_FIRST (LDS walk): each wave's first tile is placed by level (see the refill); the
    // counter then hands out the tiles after the first gridDim.x * BLK pixels
    const bool stat = STATIC_FIRST && LDST && !PROBE && p.lanes == 64 && p.tile_order != nullptr;
    const uint32_t n_static = gridDim.x * (uint32_t)BLK;
    bool first_take = true;
    // batched takes: the wave's reserved ids [res_id, res_end), the counter position it last saw,
    // and whether the counter has run past the image (all wave-uniform)
    uint32_t res_id = 0, res_end = 0, res_seen = 0;
    bool counter_done = false;
    stamps::init();
    timeline::State tl;
    timeline::init(tl);
    for (;;) {
        stamps::lap(5);
        stamps::count(8);
        timeline::round(tl, __ballot(busy), exhausted, level);
        if (cons && !retiring && level > 0 && exhausted && vq[3] == 0u && vq[2] <= level * (uint32_t)CONS_RETIRE_PER_LEVEL) retiring = true;
        bool begin = false;   // a lane took a chain: start its next pass
        // ---- refill idle lanes with new pixels (wave-aggregated dequeue) ----------------
        if (!exhausted && !retiring) {
            // cold fields reloaded here from the kernarg segment rather than held in SGPRs
            // across the loop (cpt_path.hpp kernarg_field: +2% at C4 from fewer SGPR spills)
            const KParams& p = kernarg_params();
            const uint64_t need = __ballot(!busy && lane < p.lanes);
            if (need) {
                const int leader = __ffsll((unsigned long long)need) - 1;
                uint32_t base = 0;
                uint32_t lane_id = 0;   // the id this lane takes (if it needs one)
                const bool first_take_was = first_take;
                first_take = false;
                if (stat && first_take_was) {
                    // the wave's first tile by level: the heaviest tiles (cost order) go to the
                    // level-0 waves (one per SIMD), the lightest to level 3, so every SIMD holds
                    // one heavy wave that runs alone once its lighter neighbours finish
                    // (pairing the heaviest level-0 waves with the lightest of the other levels
                    // instead lost: C4 N = 4 / 8 slowest rank 389-409 / 316-318 vs 323-338 /
                    // 308-310 ms, profiles/r06/ab_reh_snake.log)
                    base = (level * (gridDim.x * 4u) + blockIdx.x * 4u + ((threadIdx.x >> 6) & 3u)) * 64u;
                    if (n_static >= n_work) exhausted = true;
                    lane_id = base + lane_rank(need);
                }
                else if (p.replicate == 1) {
                    // Batched take: the wave draws a tile's worth of ids (TAKE_BATCH = 64) from the
                    // counter and serves its idle lanes from that range over the next rounds, so the
                    // device atomic on the one counter every wave of the grid contends for is issued
                    // once per 64 takes instead of once per round (at 1 spp a wave takes ~11 pixels
                    // every round: 2.43 -> 1.43 ms per 1-spp C4 render, DESIGN.md §Lane refill).  Pixels
                    // are independent chains, so the order they are taken in does not change the image.
                    const uint32_t n_need = wave_count(need);
                    const uint32_t avail = res_end - res_id;
                    const uint32_t off = stat ? n_static : 0u;
                    uint32_t nb = 0, ncnt = 0;
                    if (n_need > avail && !counter_done) {
                        const uint32_t want = n_need - avail;
                        // `res_seen` is the counter as this wave saw it at its last draw; a wave on
                        // long chains (spp >= 64) draws rarely, so its leader reads the counter's
                        // current value first, until its last draw fell inside the tail (the counter
                        // only grows, so a wave once in the tail stays there)
                        uint32_t seen = res_seen;
                        if (p.spp >= 64 && res_seen + n_static < n_work) {
                            uint32_t cur = 0;
                            if (lane == leader) cur = __hip_atomic_load(p.work, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            seen = __builtin_amdgcn_readfirstlane(__shfl(cur, leader)) + off;
                        }
                        uint32_t bsz = (uint32_t)TAKE_BATCH;
                        const uint32_t left_ids = n_work > seen ? n_work - seen : 0u;
                        // long chains: the range shrinks with what is left (guided scheduling), so the
                        // ids waves hold unstarted never amount to more than 1/TAKE_TAPER of a round of
                        // the grid's lanes; short chains draw exactly what they need once less than
                        // one id per lane of the grid is left
                        if (p.spp >= 64) {
                            const uint64_t t = (uint64_t)bsz * left_ids / ((uint64_t)n_static * TAKE_TAPER);
                            bsz = t < bsz ? (uint32_t)t : bsz;
                        }
                        const bool batch_ok = p.spp >= 64 || left_ids > n_static;
                        // the consolidating kernel (frames of <= 4 pixels per lane) takes exactly what
                        // it needs: there a wave's unstarted ids hold back chains other waves' idle
                        // lanes could run (DESIGN.md §Lane refill)
                        const uint32_t grab = !CONS && batch_ok && bsz > want ? bsz : want;
                        if (lane == leader) nb = atomicAdd(p.work, grab);
                        nb = __builtin_amdgcn_readfirstlane(__shfl(nb, leader)) + off;
                        ncnt = grab;
                    }
                    if (ncnt) {
                        res_seen = nb + ncnt;
                        if (nb + ncnt >= n_work) counter_done = true;
                    }
                    const uint32_t rank = lane_rank(need);
                    lane_id = rank < avail ? res_id + rank : (rank - avail < ncnt ? nb + (rank - avail) : n_work);
                    if (ncnt) {
                        res_id = nb + min(n_need - avail, ncnt);
                        res_end = nb + ncnt;
                    } else {
                        res_id += n_need < avail ? n_need : avail;
                    }
                    if (counter_done && res_id >= res_end) exhausted = true;
                }
                else {
                    // DIAGNOSTIC p.replicate > 1: every taken pixel runs on that many lanes, as
                    // identical copies (tools/lane_latency.py); 1 in normal use
                    const uint32_t rep = (uint32_t)p.replicate;
                    const uint32_t n_take = ((uint32_t)__popcll(need) + rep - 1) / rep;
                    if (lane == leader) base = atomicAdd(p.work, n_take);
                    base = __shfl(base, leader) + (stat ? n_static : 0u);
                    if (base + n_take >= n_work) exhausted = true;
                    lane_id = base + lane_rank(need) / rep;
                }
                bool took = false;
                if ((need >> lane) & 1ull) {
                    const uint32_t id = lane_id;
                    int x, ri;
                    if (id < n_work && decode_pixel(p, id, x, ri, L.tile)) {
                        execdiag::lanes(p.stats + 64, 0);
                        L.xy = (uint32_t)x | ((uint32_t)p.rows[ri] << 16);
                        L.pix = (uint32_t)ri * (uint32_t)p.width + (uint32_t)x;
                        bool owed = true;   // TOPUP: the pixel has a deficit
                        if constexpr (TOPUP) {
                            // the accumulator first: a pixel at its target is done here, its RNG
                            // planes not read and nothing of it written
                            const float4 a = p.accum[L.pix];
                            L.left = topup::deficit(a.w, p.spp);
                            owed = L.left > 0;
                            if (owed) {
                                load_rng(p, npix, L.pix, L.s);
                                L.sum = mk(a.x, a.y, a.z);
                                L.passes = a.w;
                            }
                        } else {
                            L.load<!PROBE>(p, npix);
                            L.left = p.spp;
                        }
                        if (owed) {
                            first_normal = mk1(0.f);
                            if (PROBE) work_at_take = cnt.segments + cnt.nodes + cnt.prims;
                            if (max_depth == 0) {
                                // while (0 < 0) never runs: each pass is RayGen's draws and zero radiance
                                for (; L.left > 0; --L.left) {
                                    (void)ray_gen(p, (int)(L.xy & 0xffffu), (int)(L.xy >> 16), L.s);
                                    L.sum = L.sum + mk1(0.f);
                                    L.passes += 1.0f;
                                }
                            }
                            busy = true;
                            took = true;
                            begin = L.left > 0;
                        }
                    }
                }
                if (cons) {   // live chains (taken, not finished): the consolidation's measure
                    const uint64_t t = __ballot(took);
                    if (t && lane == leader) atomicAdd(&s_q[2], (uint32_t)__popcll(t));
                    // this wave takes no more pixels: after its takes are counted (LDS atomics of
                    // one wave complete in order), so a keeper that sees no wave still taking and
                    // no live chain has seen every chain of the workgroup finish
                    if (exhausted && lane == leader) atomicSub(&s_q[3], 1u);
                }
            }
        }
        // ---- take handed-over chains into idle lanes (consolidation) ---------------------
        if (cons && !retiring && exhausted) {
            const uint64_t need = __ballot(!busy && lane < p.lanes);
            // (After the refill: a wave whose last take this round exhausted the counter with every
            // lane idle joins the keepers at once.)
            // A keeper with no chain left waits here, in this block, until it holds a handed-over
            // chain or its workgroup is done (no wave still taking, no chain live; a chain in
            // flight is never more than a pass away from its hand-over or its end).  Waiting by
            // going round the loop instead -- a back edge with every lane idle -- made the
            // register allocator spill 26 VGPRs in this kernel.
            const bool idle_wave = !__any(busy);
            bool quit = false;
            for (;;) {
                if (idle_wave) {
                    while (vq[1] == vq[0]) {   // nothing allocated to take
                        if (vq[3] == 0u && vq[2] == 0u) { quit = true; break; }
                        if (++idle_spins > keeper_spins) {
                            // never hang the device on a lost count, but never end silently either:
                            // chains of this workgroup may be left unfinished
                            if (lane == 0) atomicOr(p.error, CPT_DEVERR_KEEPER_TIMEOUT);
                            quit = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(16);
                    }
                    if (quit) break;
                }
                if (need && vq[1] != vq[0]) {
                    const int leader = __ffsll((unsigned long long)need) - 1;
                    uint32_t h = 0, n = 0;
                    if (lane == leader) {
                        for (int tries = 0; tries < 16; ++tries) {
                            h = vq[0];
                            uint32_t t = vq[1];
                            t = t < (uint32_t)QS ? t : (uint32_t)QS;   // slots past the cap are never written
                            const uint32_t want = (uint32_t)__popcll(need);
                            n = t > h ? (t - h < want ? t - h : want) : 0u;
                            if (n == 0 || atomicCAS(&s_q[0], h, h + n) == h) break;
                            n = 0;
                        }
                    }
                    h = __shfl(h, leader);
                    n = __shfl(n, leader);
                    const uint32_t rank = lane_rank(need);
                    bool lost = false;
                    if (((need >> lane) & 1ull) && rank < n) {
                        const uint32_t slot = h + rank;
                        // the slot was allocated before it was written: wait for its publication
                        const volatile uint8_t* fl = s_qflag + slot;
                        for (uint32_t w = 0; *fl == 0 && w < publish_wait; ++w) __builtin_amdgcn_s_sleep(1);
                        lost = *fl == 0;
                    }
                    if (lost) {
                        // never published: the chain is abandoned (its pixel is not written) and
                        // the render reports CPT_DEVERR_PUBLISH_TIMEOUT instead of reading the slot
                        atomicOr(p.error, CPT_DEVERR_PUBLISH_TIMEOUT);
                        atomicSub(&s_q[2], 1u);
                    } else if (((need >> lane) & 1ull) && rank < n) {
                        HoPayload::load<AUX>(ho_slot(qslab, h + rank), L, first_normal);
                        busy = true;
                        begin = true;
                    }
                }
                // one pass for a wave with chains; an idle wave whose take lost the race (or whose
                // chains were never published) tries again
                if (!idle_wave || __any(busy)) break;
                if (++idle_spins > keeper_spins) {
                    if (lane == 0) atomicOr(p.error, CPT_DEVERR_KEEPER_TIMEOUT);
                    quit = true;
                    break;
                }
            }
            if (quit) break;
        }
        if (begin) {
            execdiag::lanes(p.stats + 64, 10);
            start_pass();
        }
        stamps::lap(0);
        if (!__any(busy)) {
            // (a wave whose takes all fell outside the frame takes again while ids remain: it may
            // still hold reserved ids, which no other wave would render)
            // (a keeper of a consolidating workgroup never gets here idle: it waits in the take
            // above until its workgroup is done; an idle wave here holds no chain)
            if (!exhausted) continue;
            break;
        }
        Hit h;
        int code = -1;
        int tr = 2;
        bool hand_over = false;
        if (busy && L.left > 0) {
            // ---- one path segment: TraceRay (path_tracer.cu:141-158); a walk suspended in an
            // earlier round resumes here (LDST: trace_wide's suspension) -------------------
            if (COUNT && !ws.active) cnt.segments++;
            execdiag::lanes(p.stats + 64, 12);
            const RayK rk = make_rayk(ray);
            const bool finite_ray = ray_is_finite(ray);
            tr = trace_segment<COUNT, BLK, LDST, HYB>(p, rk, finite_ray, h, code, cnt, s_tree, ws, LDST ? SUSPEND_AT : 0);
        }
        stamps::lap(3);
        if (busy && L.left > 0 && tr != 2) {
            // ---- ClosetHit / Miss and the path bookkeeping (path_tracer.cu:159-169) --------
            const bool hit = tr == 1;
            execdiag::lanes(p.stats + 64, 13);
            Shade sh;
            v3 attr_normal;
            if (hit) {
                if (COUNT) cnt.hits++;
                execdiag::lanes(p.stats + 64, 4);
                const Mat m = p.mats[code >> 2];
#ifdef CPT_EXECDIAG
                eval_material(m, h.normal, ray.d, L.s, sh, p.stats + 64);
#else
                eval_material(m, h.normal, ray.d, L.s, sh);
#endif
                attr_normal = h.normal;
                ray.o = h.pos;                         // payload.hit_pos = position
                stamps::lap(4);
            } else {
                if (COUNT) cnt.misses++;
                sh.attenuation = mk1(0.f);             // never read: the path ends here
                sh.bounce = ray.d;
                attr_normal = -ray.d;
            }
            // Deferred sky fetches.  A miss ends the pass, and the sky's radiance only feeds
            // the pixel's running sum, so the lane may start its next pass first and add
            // rad + att * sky later, as long as the sums are added in pass order.  Pending
            // fetches run together once enough lanes hold one, instead of in every round
            // where any lane misses; a lane that would end another pass (or its pixel) with
            // one pending forces the round.  No RNG draw depends on the sky.
            bool deferred = false;
            {
                const bool ends = !hit || !(depth + 1 < max_depth);
                const bool need_now = (pend && ends) || (!hit && L.left == 1);
                // (32-bit scalar counts: SALU compares, cpt_path.hpp wave_count)
                const bool flush = DEFER_MISS_ROUND == 0 || retiring || __ballot(need_now) != 0 ||
                                   wave_count(__ballot(pend || !hit)) * 64u >=
                                       (uint32_t)DEFER_MISS_ROUND * wave_count(__builtin_amdgcn_read_exec());
                if (flush) {
                    // One sky fetch per lane that needs one: the pending (older) direction, else
                    // this miss.  A lane holding both fetches the pending one here; its new miss
                    // becomes the pending fetch (or, on the chain's last pass, is fetched below).
                    const KParams& p = kernarg_params();   // cold fields (see the refill)
                    const bool had = pend;
                    if (had || !hit) {
                        execdiag::lanes(p.stats + 64, 6);
                        const v3 dir = had ? pq.dir() : ray.d;
                        const v3 sky = miss_radiance(p, dir);
                        if (had) {
                            const v3 pr = pq.rad();
                            const v3 pa = pq.att();
                            L.sum = L.sum + (pr + pa * sky);
                            pend = false;
                        } else {
                            sh.radiance = sky;
                        }
                    }
                    if (had && !hit) {
                        if (L.left == 1 || retiring) {   // the chain ends or is handed over: due now
                            execdiag::lanes(p.stats + 64, 7);
                            sh.radiance = miss_radiance(p, ray.d);
                        } else {
                            pq.park(ray.d, rad, att);
                            pend = true;
                            deferred = true;
                            sh.radiance = mk1(0.f);
                        }
                    }
                } else if (!hit) {
                    execdiag::lanes(p.stats + 64, 8);
                    pq.park(ray.d, rad, att);
                    pend = true;
                    deferred = true;
                    sh.radiance = mk1(0.f);            // placeholder: this pass's sum waits
                }
            }
            if (!hit) depth = MAX_RECURSION_DEPTH_SET;   // termination sentinel (path_tracer.cu:121)
            rad = rad + att * sh.radiance;
            att = att * sh.attenuation;
            // the pass's first segment: its normal (0 + n, as the reference's zeroed sum; a pass
            // ends at a pass boundary only, so first_normal is the finished pass's at every read)
            if (AUX && first) first_normal = mk1(0.f) + attr_normal;
            first = false;
            ray.d = normalize_u(sh.bounce);
            ray.tmin = BOUNCE_RAY_TMIN;
            ray.tmax = DEFAULT_RAY_TMAX;
            depth++;
            if (!(depth < max_depth)) {
                if (!deferred) L.sum = L.sum + rad;
                L.passes += 1.0f;
                if (--L.left > 0) {
                    if (retiring) hand_over = true;   // the next pass runs in a keeper wave
                    else {
                        execdiag::lanes(p.stats + 64, 9);
                        start_pass();
                    }
                }
            }
        }
        if (cons) {
            // ---- hand chains over at their pass boundary (retiring waves) ---------------
            const uint64_t ho = __ballot(hand_over);
            if (ho) {
                const int leader = __ffsll((unsigned long long)ho) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(&s_q[1], (uint32_t)__popcll(ho));
                base = __shfl(base, leader);
                if (hand_over) {
                    execdiag::lanes(p.stats + 64, 14);
                    const uint32_t slot = base + lane_rank(ho);   // < QS (ho_slots)
                    HoPayload::store<AUX>(ho_slot(qslab, slot), L, first_normal);
                    wait_stores();   // the payload is in memory before the flag
                    if (!(p.dbg & 2u)) *(volatile uint8_t*)(s_qflag + slot) = 1;
                    busy = false;
                    hand_over = false;
                }
            }
        }
        bool finished = false;
        if (busy && L.left == 0) {
            // (cold fields from the kernarg segment: see the refill)
            finish_pixel<AUX, PROBE>(kernarg_params(), L, first_normal, work_at_take, cnt, npix, max_depth);
            busy = false;
            finished = true;
        }
        if (cons) {
            const uint64_t f = __ballot(finished);
            if (f && lane == __ffsll((unsigned long long)f) - 1) atomicSub(&s_q[2], (uint32_t)__popcll(f));
        }
    }
    stamps::flush(p.stats + 16);
    pooldiag::flush(p.stats + 64);
    timeline::flush(tl);
    if (STATS && !PROBE) flush_walk_counters<true>(cnt, p.stats);
}

// ======================================================================================
// Host-side launchers (called from cpt_capi_render.cpp and cpt_capi_adaptive.cpp).
// ======================================================================================
template <bool S, bool A, bool P, bool T, bool C = false, bool H = false, bool U = false>
static hipError_t launch_mk(const KParams& p, LaunchGrid& g, hipStream_t stream) {
    constexpr int block = mk_block<T>();
    // persistent grid: every resident slot once; lanes pull pixels from p.work.  (The test hook's
    // cap makes lanes take several pixels in turn on small frames; the kernel's gridDim.x follows.)
    const long long tiles = p.n_active ? (long long)p.n_active : (long long)TileGrid{p.width, p.n_rows}.count();
    int grid = 0;
    const hipError_t e = g.size((const void*)k_megakernel<S, A, P, T, C, H, U>, block,
                                megakernel_want(tiles, p.lanes, p.replicate, block), true, &grid);
    if (e != hipSuccess || grid < 1) return e;
    hipLaunchKernelGGL((k_megakernel<S, A, P, T, C, H, U>), dim3((unsigned)grid), dim3(block), 0, stream, p);
    return hipGetLastError();
}

template <bool S, bool A, bool P, bool H>
static hipError_t launch_mk_lds(const KParams& p, LaunchGrid& g, hipStream_t stream) {
    if constexpr (!P && ho_slots<mk_block<true>()>() > 0) {
        if (p.resume) return launch_mk<S, A, P, true, true, H>(p, g, stream);   // tail consolidation
    }
    return launch_mk<S, A, P, true, false, H>(p, g, stream);
}

template <bool S, bool A, bool P>
static hipError_t launch_mk_any(const KParams& p, LaunchGrid& g, hipStream_t stream) {
    if (!use_lds_tree(p)) return launch_mk<S, A, P, false>(p, g, stream);
    if (p.n_wide > LDS_TREE_NODES) return launch_mk_lds<S, A, P, true>(p, g, stream);
    return launch_mk_lds<S, A, P, false>(p, g, stream);
}

hipError_t launch_megakernel(const KParams& p, bool stats, bool aux, LaunchGrid& g, hipStream_t stream) {
    if (p.width <= 0 || p.n_rows <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(p.work, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (stats && aux) return launch_mk_any<true, true, false>(p, g, stream);
    if (stats) return launch_mk_any<true, false, false>(p, g, stream);
    if (aux) return launch_mk_any<false, true, false>(p, g, stream);
    return launch_mk_any<false, false, false>(p, g, stream);
}

// The top-up launch (cpt_render_to_count): the TOPUP kernels over STATS x AUX x {no LDS tree, LDST,
// LDST + HYB}, never consolidating.  p.n_active is 0, so the grid is sized for the whole frame;
// the workgroups that find the plan's active tiles taken leave at their first take.
template <bool S, bool A>
static hipError_t launch_mk_topup(const KParams& p, LaunchGrid& g, hipStream_t stream) {
    if (!use_lds_tree(p)) return launch_mk<S, A, false, false, false, false, true>(p, g, stream);
    if (p.n_wide > LDS_TREE_NODES) return launch_mk<S, A, false, true, false, true, true>(p, g, stream);
    return launch_mk<S, A, false, true, false, false, true>(p, g, stream);
}

hipError_t launch_megakernel_topup(const KParams& p, bool stats, bool aux, LaunchGrid& g, hipStream_t stream) {
    if (p.width <= 0 || p.n_rows <= 0) return hipSuccess;
    if (!p.topup_active || !p.tile_order || p.n_active || p.resume) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(p.work, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (stats && aux) return launch_mk_topup<true, true>(p, g, stream);
    if (stats) return launch_mk_topup<true, false>(p, g, stream);
    if (aux) return launch_mk_topup<false, true>(p, g, stream);
    return launch_mk_topup<false, false>(p, g, stream);
}

// The resident workgroups of the consolidating kernel launch_mk_lds picks for these flags and
// this tree: consolidation_slab sizes the slab by them before the launch.
template <bool S, bool A, bool H> static const void* cons_fn() { return (const void*)k_megakernel<S, A, false, true, true, H>; }
hipError_t consolidating_workgroups(const KParams& p, bool stats, bool aux, LaunchGrid& g, long long* out) {
    const void* const fn[2][2][2] = {{{cons_fn<0, 0, 0>(), cons_fn<0, 0, 1>()}, {cons_fn<0, 1, 0>(), cons_fn<0, 1, 1>()}},
                                     {{cons_fn<1, 0, 0>(), cons_fn<1, 0, 1>()}, {cons_fn<1, 1, 0>(), cons_fn<1, 1, 1>()}}};
    return g.resident(fn[stats][aux][p.n_wide > LDS_TREE_NODES], mk_block<true>(), out);
}

// The cost schedule's pilot (cpt_schedule.hip launch_tile_schedule): the PROBE kernels.
hipError_t launch_cost_pilot(const KParams& p, LaunchGrid& g, hipStream_t stream) {
    return launch_mk_any<false, false, true>(p, g, stream);
}

// DIAGNOSTIC (CPT_TIMELINE builds): copy the lane-occupancy timeline out (n words, at most
// timeline::TL_WORDS) and clear it for the next render; other builds: hipErrorNotSupported.
hipError_t timeline_read(unsigned long long* out, int n, hipStream_t stream) {
#ifdef CPT_TIMELINE
    if (n > timeline::TL_WORDS) n = timeline::TL_WORDS;
    void* sym = nullptr;
    hipError_t e = hipGetSymbolAddress(&sym, HIP_SYMBOL(timeline::g_tl));
    if (e == hipSuccess) e = hipMemcpyAsync(out, sym, (size_t)n * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemsetAsync(sym, 0, (size_t)timeline::TL_WORDS * 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync((unsigned long long*)sym + 4 * timeline::TL_BINS, 0xff, 8, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    return e;
#else
    (void)out; (void)n; (void)stream;
    return hipErrorNotSupported;
#endif
}

// ======================================================================================
// Per-material constants: alpha = pow(1000.0f, s) (float pow), 1.0 / alpha in double
// (material.cu:43-45, 69-70, 103-104).
// ======================================================================================
// Completes the host-staged materials (cpt_device.hpp Mat): emission colour, GetKd(0, 0) of
// textured materials (tex_of_mat[i] >= 0: index into texs), 1/alpha.
// (Kept in the megakernel's unit: compiled in a unit without k_megakernel the same instructions
// come out with another register assignment, and its assembly is held identical across refactors.)
__global__ void k_prepare_materials(Mat* mats, const int32_t* tex_of_mat, const TexDesc* texs, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Mat m = mats[i];
    const v3 kd = mk(m.att_x, m.att_y, m.att_z);   // staged: kd_ (the union's bits)
    const v3 rad = m.rad_x * kd;                    // staged: rad_x = emit_intensity_
    m.rad_x = rad.x; m.rad_y = rad.y; m.rad_z = rad.z;
    const int t = tex_of_mat ? tex_of_mat[i] : -1;
    if (t >= 0) {
        const TexDesc d = texs[t];
        const v3 c = tex_fetch_dyn(TexView{d.texels, d.w, d.h, d.cols}, d.addr, d.filter, 0.0f, 0.0f);
        m.att_x = c.x; m.att_y = c.y; m.att_z = c.z;
    }
    float alpha = dm::powf_(1000.0f, m.smoothness);
    m.inv_alpha = 1.0 / (double)alpha;
    m.inv_ior = 1.f / m.ior;
    if (m.type == 3) {   // Glass (the only shader that reads r0; Mirror reads reflectivity)
        float r0 = (1 - m.ior) / (1 + m.ior);
        r0 *= r0;
        m.schlick_r0 = r0;
    }
    mats[i] = m;
}

hipError_t launch_prepare_materials(Mat* mats, const int32_t* tex_of_mat, const TexDesc* texs, int n,
                                    hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_prepare_materials, dim3((n + 63) / 64), dim3(64), 0, stream, mats, tex_of_mat, texs, n);
    return hipGetLastError();
}

}  // namespace cpt
