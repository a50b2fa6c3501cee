// cpt_kernels.hip — HIP kernels of the MI355X integrator (gfx950, wave64).
//
//   k_prepare_materials  per-material constants: GetKd(0,0), emission, 1/alpha — material.cu
//   k_rng_*              InitCuRand (path_tracer.cu:36-42) as three GF(2) kernels
//   k_megakernel         SamplePixel (path_tracer.cu:124-175), all spp passes per launch,
//                        per-lane path regeneration, state in registers
//   k_math_batch         device-math KAT surface for the parity tests
//
// Reference semantics per function are cited inline; DESIGN.md has the data layout and the
// roofline of each kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include <hipcub/hipcub.hpp>

#include "cpt_path.hpp"
#include "cpt_dn_exp.hpp"

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
// Hand-over slots per workgroup: each of the waves of levels 1.. retires once and hands over
// at most its 64 chains, so (levels - 1) x 256 slots always suffice.
template <int BLK> constexpr int ho_slots() { return (BLK / 256 - 1) * 256; }
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {   // set lanes of `mask` below this one
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

struct Lane {
    uint32_t xy;     // x | y << 16 (frames are < 65536 pixels wide and high)
    uint32_t pix;    // context pixel index (frames are < 2^32 pixels)
    uint32_t tile;
    Xorwow s;
    v3 sum;
    float passes;
    int left;
};

__device__ __forceinline__ bool decode_pixel(const KParams& p, uint32_t id, int& x, int& ri, uint32_t& tile) {
    const int tiles_x = (p.width + 7) >> 3;
    tile = id >> 6;
    if (p.tile_order) tile = p.tile_order[tile];
    const uint32_t k = id & 63;
    x = (int)(tile % tiles_x) * 8 + (int)(k & 7);
    ri = (int)(tile / tiles_x) * 8 + (int)(k >> 3);
    return x < p.width && ri < p.n_rows;
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
template <bool STATS, bool AUX, bool PROBE, bool LDST, bool CONS, bool HYB>
__global__ void __launch_bounds__(mk_block<LDST>(), mk_waves<LDST>()) k_megakernel(const KParams p) {
    constexpr bool COUNT = STATS || PROBE;
    constexpr int BLK = mk_block<LDST>();
    __shared__ uint4 s_tree[LDST ? LDS_TREE_NODES * 7 : 1];
    pooldiag::init();
    if (LDST) {
        const uint4* src = reinterpret_cast<const uint4*>(p.nodes + wide_image_base(p));
        for (int i = threadIdx.x; i < 7 * lds_tree_nodes(p.n_wide); i += BLK) s_tree[i] = src[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const size_t npix = (size_t)p.n_rows * p.width;
    const uint32_t n_work = (uint32_t)(((p.width + 7) >> 3) * ((p.n_rows + 7) >> 3)) * 64u;
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
    float* const pq = pending_q + threadIdx.x;
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
    uint4* const qslab = cons ? p.resume + 5 * (size_t)blockIdx.x * QS : nullptr;
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
                        L.s.v0 = p.rng[L.pix];
                        L.s.v1 = p.rng[npix + L.pix];
                        L.s.v2 = p.rng[2 * npix + (size_t)L.pix];
                        L.s.v3 = p.rng[3 * npix + (size_t)L.pix];
                        L.s.v4 = p.rng[4 * npix + (size_t)L.pix];
                        L.s.d = p.rng[5 * npix + (size_t)L.pix];
                        float4 acc = (p.accumulate && !PROBE) ? p.accum[L.pix] : make_float4(0.f, 0.f, 0.f, 0.f);
                        L.sum = mk(acc.x, acc.y, acc.z);
                        L.passes = acc.w;
                        L.left = p.spp;
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
                        const uint32_t slot = h + rank;
                        const uint32_t* e = reinterpret_cast<const uint32_t*>(qslab + 5 * (size_t)slot);
                        auto ld4 = [&](int q) {
                            return make_uint4(ld_coherent(e + 4 * q), ld_coherent(e + 4 * q + 1), ld_coherent(e + 4 * q + 2),
                                              ld_coherent(e + 4 * q + 3));
                        };
                        const uint4 e0 = ld4(0), e1 = ld4(1), e2 = ld4(2), e3 = AUX ? ld4(3) : make_uint4(0u, 0u, 0u, 0u);
                        const uint32_t left = ld_coherent(e + 16);
                        L.pix = e0.x; L.xy = e0.y; L.s.v0 = e0.z; L.s.v1 = e0.w;
                        L.s.v2 = e1.x; L.s.v3 = e1.y; L.s.v4 = e1.z; L.s.d = e1.w;
                        L.sum = mk(__uint_as_float(e2.x), __uint_as_float(e2.y), __uint_as_float(e2.z));
                        L.passes = __uint_as_float(e2.w);
                        if (AUX) {
                            first_normal = mk(__uint_as_float(e3.x), __uint_as_float(e3.y), __uint_as_float(e3.z));
                        }
                        L.left = (int)left;
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
            const bool finite_ray = !(ray.o.x != ray.o.x || ray.o.y != ray.o.y || ray.o.z != ray.o.z ||
                                      ray.d.x != ray.d.x || ray.d.y != ray.d.y || ray.d.z != ray.d.z);
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
                        const v3 dir = had ? mk(pq[0 * BLK], pq[1 * BLK], pq[2 * BLK]) : ray.d;
                        const v3 sky = miss_radiance(p, dir);
                        if (had) {
                            const v3 pr = mk(pq[3 * BLK], pq[4 * BLK], pq[5 * BLK]);
                            const v3 pa = mk(pq[6 * BLK], pq[7 * BLK], pq[8 * BLK]);
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
                            pq[0 * BLK] = ray.d.x; pq[1 * BLK] = ray.d.y; pq[2 * BLK] = ray.d.z;
                            pq[3 * BLK] = rad.x; pq[4 * BLK] = rad.y; pq[5 * BLK] = rad.z;
                            pq[6 * BLK] = att.x; pq[7 * BLK] = att.y; pq[8 * BLK] = att.z;
                            pend = true;
                            deferred = true;
                            sh.radiance = mk1(0.f);
                        }
                    }
                } else if (!hit) {
                    execdiag::lanes(p.stats + 64, 8);
                    pq[0 * BLK] = ray.d.x; pq[1 * BLK] = ray.d.y; pq[2 * BLK] = ray.d.z;
                    pq[3 * BLK] = rad.x; pq[4 * BLK] = rad.y; pq[5 * BLK] = rad.z;
                    pq[6 * BLK] = att.x; pq[7 * BLK] = att.y; pq[8 * BLK] = att.z;
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
                    const uint32_t slot = base + lane_rank(ho);
                    {   // slot < QS (ho_slots)
                        uint32_t* e = reinterpret_cast<uint32_t*>(qslab + 5 * (size_t)slot);
                        const uint32_t w[20] = {L.pix, L.xy, L.s.v0, L.s.v1, L.s.v2, L.s.v3, L.s.v4, L.s.d,
                                                __float_as_uint(L.sum.x), __float_as_uint(L.sum.y), __float_as_uint(L.sum.z),
                                                __float_as_uint(L.passes), __float_as_uint(first_normal.x),
                                                __float_as_uint(first_normal.y), __float_as_uint(first_normal.z),
                                                0u, (uint32_t)L.left, 0u, 0u, 0u};
#pragma unroll
                        for (int k = 0; k < 17; ++k)
                            if (AUX || k < 12 || k == 16) st_coherent(e + k, w[k]);
                        wait_stores();   // the payload is in memory before the flag
                        if (!(p.dbg & 2u)) *(volatile uint8_t*)(s_qflag + slot) = 1;
                        busy = false;
                    }
                    hand_over = false;
                }
            }
        }
        bool finished = false;
        if (busy && L.left == 0) {
            const KParams& p = kernarg_params();   // cold fields (see the refill)
            if (PROBE) {
                // ---- pilot: the pixel's work goes to its tile's cost ----------------------
                // the tile's key is its heaviest pixel's work, not the tile's sum (round 6): one long
                // chain in an otherwise light tile must start with the first tiles, not in the tail
                // (tools/timeline.py: C5 N = 8, the rank's last quarter ran a few hundred such chains)
                atomicMax(&p.tile_cost[L.tile], cnt.segments + cnt.nodes + cnt.prims - work_at_take);
            } else {
                // ---- pixel finished: write back (path_tracer.cu:172-174) -----------------
                execdiag::lanes(p.stats + 64, 11);
                p.accum[L.pix] = make_float4(L.sum.x, L.sum.y, L.sum.z, L.passes);
                if (AUX && p.spp > 0) {
                    p.normal[3 * (size_t)L.pix + 0] = first_normal.x;
                    p.normal[3 * (size_t)L.pix + 1] = first_normal.y;
                    p.normal[3 * (size_t)L.pix + 2] = first_normal.z;
                    p.depth[L.pix] = max_depth > 0 ? DEFAULT_RAY_TMAX : 0.f;   // a18
                }
                p.rng[L.pix] = L.s.v0;
                p.rng[npix + L.pix] = L.s.v1;
                p.rng[2 * npix + (size_t)L.pix] = L.s.v2;
                p.rng[3 * npix + (size_t)L.pix] = L.s.v3;
                p.rng[4 * npix + (size_t)L.pix] = L.s.v4;
                p.rng[5 * npix + (size_t)L.pix] = L.s.d;
            }
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
    if (STATS && !PROBE) {
        uint64_t a = wave_sum(cnt.segments), b = wave_sum(cnt.nodes), c = wave_sum(cnt.prims);
        uint64_t d = wave_sum(cnt.hits), e = wave_sum(cnt.misses);
        const uint64_t f = wave_sum(cnt.fallbacks);   // ordered walk: certificate fallbacks
        const uint64_t g = wave_sum(cnt.gnodes);      // wide nodes read from global memory
        if (lane == 0) {
            atomicAdd((unsigned long long*)&p.stats[0], (unsigned long long)a);
            atomicAdd((unsigned long long*)&p.stats[1], (unsigned long long)b);
            atomicAdd((unsigned long long*)&p.stats[2], (unsigned long long)c);
            atomicAdd((unsigned long long*)&p.stats[3], (unsigned long long)d);
            atomicAdd((unsigned long long*)&p.stats[4], (unsigned long long)e);
            if (f) atomicAdd((unsigned long long*)&p.stats[5], (unsigned long long)f);
            if (g) atomicAdd((unsigned long long*)&p.stats[6], (unsigned long long)g);
        }
    }
}

// ======================================================================================
// Self-test of qdiv against the hardware IEEE divide on hashed bit patterns.
// which = 0: all 2^32 x 2^32 patterns (NaN/inf/subnormal included); 1: a = box-plane
// differences (|a| < 2^20), d = unit-vector components; 2: a, d in [2^-30, 2^30]; 3: rcp_d(d)
// itself against 1.0 / (double)d for d = float bit pattern i; 4: rcp_f(d) against 1.0f / d on
// its domain and rcp_f(sqrtf(d)) against 1.0f / sqrtf(d) for every pattern.
// ======================================================================================
__device__ __forceinline__ uint32_t hash32(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return (uint32_t)x;
}

// out[0] = mismatch count; out[1..out_len) = (a bits << 32 | d bits) of some mismatches.
__global__ void k_selftest_qdiv(int which, uint64_t n, uint64_t seed, unsigned long long* out, int out_len) {
    uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t ua = hash32(seed * 0x9e3779b97f4a7c15ULL + 2 * i), ud = hash32(seed * 0x9e3779b97f4a7c15ULL + 2 * i + 1);
        float a, d;
        if (which == 0) {
            a = __uint_as_float(ua);
            d = __uint_as_float(ud);
        } else if (which == 1) {
            a = __uint_as_float((ua & 0x807fffffu) | ((100u + (ua >> 23) % 47u) << 23));   // 2^-27 .. 2^20
            d = __uint_as_float((ud & 0x807fffffu) | ((97u + (ud >> 23) % 30u) << 23));    // 2^-30 .. 2^-1
        } else {
            a = __uint_as_float((ua & 0x807fffffu) | ((97u + (ua >> 23) % 60u) << 23));
            d = __uint_as_float((ud & 0x807fffffu) | ((97u + (ud >> 23) % 60u) << 23));
        }
        bool same;
        if (which == 3) {   // rcp_d over the float bit patterns 0 .. n-1
            a = 1.0f;
            d = __uint_as_float((uint32_t)i);
            const double r_ref = 1.0 / (double)d, r = rcp_d(d);
            same = __double_as_longlong(r_ref) == __double_as_longlong(r) || (r_ref != r_ref && r != r);
        } else if (which == 4) {   // rcp_f over its domain, and over sqrtf of every pattern
            a = 1.0f;
            d = __uint_as_float((uint32_t)i);
            const uint32_t ex = ((uint32_t)i >> 23) & 0xffu;
            const bool dom = (ex >= 1u && ex <= 252u) || d == 0.0f || ex == 255u;
            const float r_ref = 1.0f / d, r = rcp_f(d);
            const float s = __builtin_sqrtf(d), rs_ref = 1.0f / s, rs = rcp_f(s);
            same = (!dom || __float_as_uint(r_ref) == __float_as_uint(r) || (r_ref != r_ref && r != r)) &&
                   (__float_as_uint(rs_ref) == __float_as_uint(rs) || (rs_ref != rs_ref && rs != rs));
        } else if (which == 5) {   // sqrt_nn over its domain: +-0, |x| >= 2^-96, inf, NaN
            a = 1.0f;
            d = __uint_as_float((uint32_t)i);
            const uint32_t ex = ((uint32_t)i >> 23) & 0xffu;
            const bool dom = ex >= 31u || ((uint32_t)i & 0x7fffffffu) == 0u;
            const float r_ref = __builtin_sqrtf(d), r = sqrt_nn_raw(d);
            same = !dom || __float_as_uint(r_ref) == __float_as_uint(r) || (r_ref != r_ref && r != r);
        } else {
            const float q_ref = a / d;
            const float q = qdiv(a, d, rcp_d(d));
            same = (__float_as_uint(q_ref) == __float_as_uint(q)) || (q_ref != q_ref && q != q);
        }
        if (!same) {
            unsigned long long k = atomicAdd(&out[0], 1ull);
            if ((long long)k + 1 < out_len) out[k + 1] = ((unsigned long long)__float_as_uint(a) << 32) | __float_as_uint(d);
        }
    }
}

// ======================================================================================
// Per-material constants: alpha = pow(1000.0f, s) (float pow), 1.0 / alpha in double
// (material.cu:43-45, 69-70, 103-104).
// ======================================================================================
// Completes the host-staged materials (cpt_device.hpp Mat): emission colour, GetKd(0, 0) of
// textured materials (tex_of_mat[i] >= 0: index into texs), 1/alpha.
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

// ======================================================================================
// InitCuRand (path_tracer.cu:36-42): curand_init(seed, (x<<32)|y, 0) per pixel, i.e.
// v = A^(2^67 * ((x<<32)|y)) v_seed.  Factored as v = M_y (N_x v_seed) with
// M_y = A^(2^67 y), N_x = A^(2^99 x) — GF(2) linear, exact.  jumps[t] = A^(2^67 * 2^t)
// (160x160 bits, column-major: column c = 5 words at [t][c*5..c*5+4]).
// All loops over matrix columns are wave-uniform, so the column loads are uniform too.
// ======================================================================================
__device__ __forceinline__ void matvec_uniform(const uint32_t* __restrict__ M, const uint32_t in[5], uint32_t out[5]) {
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
    for (int c = 0; c < 160; ++c) {
        uint32_t mask = 0u - ((in[c >> 5] >> (c & 31)) & 1u);
        const uint32_t* col = M + c * 5;
        r0 ^= mask & col[0];
        r1 ^= mask & col[1];
        r2 ^= mask & col[2];
        r3 ^= mask & col[3];
        r4 ^= mask & col[4];
    }
    out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3; out[4] = r4;
}

// w[x] = N_x v_seed for every column x of the frame (one thread per x).
__global__ void k_rng_columns(const uint32_t* __restrict__ jumps, uint32_t seed_v0, uint32_t seed_v1, uint32_t seed_v2,
                              uint32_t seed_v3, uint32_t seed_v4, int width, uint32_t* __restrict__ w) {
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t v[5] = {seed_v0, seed_v1, seed_v2, seed_v3, seed_v4};
    for (int t = 0; t < 31; ++t) {              // bits 32..62 of the subsequence
        uint32_t out[5];
        matvec_uniform(jumps + (size_t)(32 + t) * 800, v, out);
        bool take = x < width && ((x >> t) & 1);
        if (take) { v[0] = out[0]; v[1] = out[1]; v[2] = out[2]; v[3] = out[3]; v[4] = out[4]; }
        if (!__any(x < width && (x >> (t + 1)) != 0)) break;
    }
    if (x < width) for (int k = 0; k < 5; ++k) w[(size_t)k * width + x] = v[k];
}

// M_y for every distinct row: block = one row, 160 threads = the 160 columns.
__global__ void k_rng_rowmats(const uint32_t* __restrict__ jumps, const int32_t* __restrict__ rows,
                              uint32_t* __restrict__ mats) {
    const int ri = blockIdx.x;
    const int c = threadIdx.x;
    const uint32_t y = (uint32_t)rows[ri];
    uint32_t v[5] = {0, 0, 0, 0, 0};
    if (c < 160) v[c >> 5] = 1u << (c & 31);
    for (int t = 0; t < 32 && (y >> t) != 0; ++t) {
        if ((y >> t) & 1u) {
            uint32_t out[5];
            matvec_uniform(jumps + (size_t)t * 800, v, out);
            for (int k = 0; k < 5; ++k) v[k] = out[k];
        }
    }
    if (c < 160)
        for (int k = 0; k < 5; ++k) mats[(size_t)ri * 800 + c * 5 + k] = v[k];
}

// v_pixel = M_y w_x; d = the seed's d (2^67 k Weyl steps are 0 mod 2^32).  Grid: (x blocks, rows).
__global__ void k_rng_pixels(const uint32_t* __restrict__ rowmats, const uint32_t* __restrict__ w, int width,
                             int n_rows, uint32_t seed_d, uint32_t* __restrict__ rng) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int ri = blockIdx.y;
    const uint32_t* M = rowmats + (size_t)ri * 800;
    uint32_t in[5];
    const int xx = x < width ? x : width - 1;
    for (int k = 0; k < 5; ++k) in[k] = w[(size_t)k * width + xx];
    uint32_t out[5];
    matvec_uniform(M, in, out);
    if (x < width) {
        const size_t npix = (size_t)n_rows * width;
        const size_t pix = (size_t)ri * width + x;
        for (int k = 0; k < 5; ++k) rng[k * npix + pix] = out[k];
        rng[5 * npix + pix] = seed_d;
    }
}

// ======================================================================================
// Display path: Denoising + Mix (path_tracer.cu:177-254) fused into one stencil kernel.
//
// Input: the pass radiance (accumulator rgb / pass count) and first-hit normals of the
// last render; depth is the constant 1e30 (a18), so its weight is exp(0) = 1.  The
// reference's launch covers W' x H' = 16*floor(W/16) x 16*floor(H/16) pixels and indexes
// neighbours by LINEAR offset v*W' + u, so x +- 1, 2 wraps into the adjacent row and only
// offsets outside [0, W'*H') get zero weight (path_tracer.cu:205-216); reproduced here.
// Weights min(exp(-d2/M_PI), 1.0) are double (path_tracer.cu:215-222).  Mix:
// mix = lerp(mix, clamp(denoised, 0, 1), 1/cur_sample_idx); bytes 0..2 = 255.99*(b, g, r)
// (path_tracer.cu:241-254); the alpha byte, which the reference never writes (its frame copies
// whatever the device buffer held, :251-253,303), is stored as 0 in one 32-bit store.
// ======================================================================================
// min(exp(-(dist2) / M_PI), 1.0) in double, stored to float (path_tracer.cu:224,228,231), for a
// float dist2 -- the oracle's dm_exp(-(double)dist2 / REF_PI), branch-free.  The SLOW form (round 4),
// now only the fallback of dn_weights below near a float rounding boundary:
//  * dist2 in (0, 330): x = -dist2/pi in (-105.05, 0), the quotient from dm::div_pi's sequence
//    (correctly rounded: it depends only on dist2's significand, and every significand is
//    checked); then dm::exp's own steps -- k, the two-part reduction, the Horner polynomial --
//    and its ldexp, which for k in [-152, 0] is one exact multiplication by 2^k (v_ldexp_f64);
//  * dist2 == 0: exp(-0) = 1;  dist2 >= 330 (inf included): exp(x) < 2^-150, which rounds to
//    float 0;  NaN: exp(NaN) = NaN, and `w < 1.0 ? w : 1.0` gives 1.
// tests/test_exact_identities.py checks the whole function against the oracle's expression
// for every float in [0, 2341] and the special values.
__device__ __forceinline__ float dn_weight_slow_inl(float dist2) {
    constexpr double INV_PI = 1.0 / REF_PI;
    const double a = (double)dist2;
    const double q = a * INV_PI;
    const double x = -__builtin_fma(__builtin_fma(-q, REF_PI, a), INV_PI, q);
    const double k = __builtin_floor(__builtin_fma(x, dm::kc(dm::INV_LN2), 0.5));
    const double r = __builtin_fma(-k, dm::kc(dm::LN2_LO), __builtin_fma(-k, dm::kc(dm::LN2_HI), x));
    double p = 1.0 / 6227020800.0;
    p = __builtin_fma(r, p, dm::kc(1.0 / 479001600.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 39916800.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 3628800.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 362880.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 40320.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 5040.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 720.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 120.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 24.0));
    p = __builtin_fma(r, p, dm::kc(1.0 / 6.0));
    p = __builtin_fma(r, p, dm::kc(0.5));
    p = __builtin_fma(r, p, dm::kc(1.0));
    p = __builtin_fma(r, p, dm::kc(1.0));
    const double w = __builtin_ldexp(p, (int)k);
    float f = (float)(w < 1.0 ? w : 1.0);
    f = dist2 >= 330.0f ? 0.0f : f;
    return dist2 == 0.0f ? 1.0f : f;
}
// (out of line where a weight is evaluated alone; inlined in the batched weights, whose kernels
// would otherwise spill the caller-saved VGPRs live across the call)
__device__ __noinline__ float dn_weight_slow(float dist2) { return dn_weight_slow_inl(dist2); }


// The weight's short form (round 5): the same float, from a double approximation E' of
// exp(-dist2/pi) that is within 2^-46.3 (relative) of the oracle's double E, rounded to float
// only where that cannot matter:
//  * E' = 2^-(n>>S) * T[n & (N-1)] * P(r) (cpt_dn_exp.hpp: N = 2^S table entries, P of degree
//    DN_POLY_DEG):  z = dist2 * N/(pi ln2) (KN_HI + KN_LO), n = round(z) by the 1.5*2^52
//    shifter (n is t's low word), r = z - n in [-1/2, 1/2] (one fma against the exact product
//    dist2 * KN_HI, then the low part), T[j] = 2^(-j/N) correctly rounded from the LDS table,
//    P = the Taylor polynomial of 2^(-r/N), and 2^-(n>>S) applied to T's exponent field
//    (T >= 1/2 and n>>S <= 151: stays normal).  N = 1024, degree 3 (8 KB; truncation
//    < 2^-50.7); round 5's first table was N = 32, degree 5 (256 B, conflict-free in LDS,
//    truncation < 2^-48.7).  E' is within ~2^-48.5 of exp(-dist2/pi); the oracle's
//    E = dm_exp(RN(-dist2/pi)) is within 2^-47 (the quotient's rounding, |x| < 105.05) + 2^-52
//    of it.
//  * Guard (dn_near_midpoint): if no float rounding boundary lies within 2^-44 E' of E' (its
//    bits below float precision are not within 2^9 of the half-way pattern), every double in
//    between rounds alike, E included (rounding is monotone), so (float)E' is the oracle's float.
//    Otherwise (about 1 in 10^6 weights; also subnormal float results and NaN) the slow form
//    decides.  dist2 = 0 and dist2 >= 330 keep their shortcuts.
// tests/test_exact_identities.py restates it on the host against the oracle for every float in
// [0, 2341]; test_gpu_parity.py::test_dn_weight_exhaustive runs this device code against
// dn_weight_slow for all 2^31 non-negative float patterns.
__device__ const double g_dn_exp_table[DN_EXP_N] = CPT_DN_EXP_TABLE_INIT;

__device__ __forceinline__ double dn_exp_short(float dist2, const double* __restrict__ tab) {
    constexpr double SHIFT = 0x1.8p52;
    const double a = (double)dist2;
    const double t = __builtin_fma(a, DN_KN_HI, SHIFT);
    const double nd = t - SHIFT;
    const uint32_t n = (uint32_t)__double2loint(t);
    double r = __builtin_fma(a, DN_KN_HI, -nd);
    r = __builtin_fma(a, DN_KN_LO, r);
    double p = DN_POLY_DEG >= 4 ? (DN_POLY_DEG >= 5 ? __builtin_fma(r, DN_C5, DN_C4) : DN_C4) : DN_C3;
    if (DN_POLY_DEG >= 4) p = __builtin_fma(r, p, DN_C3);
    p = __builtin_fma(r, p, DN_C2);
    p = __builtin_fma(r, p, DN_C1);
    p = __builtin_fma(r, p, 1.0);
    const double T = tab[n & (uint32_t)(DN_EXP_N - 1)];
    const double Ts = __hiloint2double(__double2hiint(T) - (int)((n >> DN_EXP_SHIFT) << 20), __double2loint(T));
    return Ts * p;
}

// The guard on the bits of e: for e in [2^-126, 1] (a normal float result) rounding to float looks
// at the 29 mantissa bits below float precision, all in e's low word; e rounds like every double
// within 2^-44 e of it unless those bits lie within 2^9 (> 2^-44 / 2^-52 = 2^8 double ulps, with
// margin) of the half-way pattern 2^28.  Smaller e (a subnormal float result, dist2 > 274.5),
// larger e, NaN and inf are sent to the slow form, whose dist2 >= 330 shortcut the caller applies.
__device__ __forceinline__ bool dn_near_midpoint(double e) {
    const uint32_t lo = (uint32_t)__double2loint(e), hi = (uint32_t)__double2hiint(e);
    const int d = (int)(lo & 0x1fffffffu) - (1 << 28);
    const bool normal_f = hi >= 0x38100000u && hi <= 0x3ff00000u;   // 2^-126 <= e <= 1 (e > 0 here)
    return !normal_f || (d < 512 && d > -512);
}

// The winner certificate's quotient-free form (cpt_path.hpp cert_inside) against the exact slab
// test it stands in for (slab_reject<true> with exact quotients), on case i of a counter-hashed
// stream (seed, i): a box (sphere-like, or a platform's +-5e30 x/z slab), a ray (3% of axes with
// d == 0) and a distance t either within 16 float ulps of one of the six planes' exact quotients
// (the only place the two can disagree) or anywhere in (0, 200].  which = 14 counts the cases
// the certificate passes and the exact test rejects (0 expected); 15 counts the cases it
// certifies, 16 the cases the exact test passes (the test checks the form decides most of them).
__device__ __forceinline__ uint64_t cert_mix(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float cert_unit(uint64_t& st) {
    st = cert_mix(st);
    return (float)(uint32_t)(st >> 40) * 0x1p-24f;
}
__device__ bool cert_case(uint64_t seed, uint64_t i, int which) {
    uint64_t st = cert_mix(seed ^ cert_mix(i));
    float c[3], e[3], o[3], d[3];
    for (int k = 0; k < 3; ++k) {
        c[k] = -30.f + 60.f * cert_unit(st);
        const float u = cert_unit(st);
        e[k] = 1e-3f + 10.f * u * u * u;
        o[k] = -60.f + 120.f * cert_unit(st);
        d[k] = cert_unit(st) - 0.5f;
    }
    const float inv = 1.0f / __builtin_sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int k = 0; k < 3; ++k) d[k] = cert_unit(st) < 0.03f ? 0.0f : d[k] * inv;
    Node box{};
    box.a0 = c[0] - e[0]; box.a1 = c[1] - e[1]; box.a2 = c[2] - e[2];
    box.b0 = c[0] + e[0]; box.b1 = c[1] + e[1]; box.b2 = c[2] + e[2];
    if (cert_unit(st) < 0.1f) {   // a platform's box: unbounded in x and z, +-1e-4 in y
        box.a0 = box.a2 = -5e30f; box.b0 = box.b2 = 5e30f;
        box.a1 = c[1] - 1e-4f; box.b1 = c[1] + 1e-4f;
    }
    float t;
    if (cert_unit(st) < 0.5f) {
        const int ax = (int)(cert_unit(st) * 3.f) % 3;
        const bool lo_side = cert_unit(st) < 0.5f;
        const float pa[3] = {box.a0, box.a1, box.a2}, pb[3] = {box.b0, box.b1, box.b2};
        const float q = ((lo_side ? pa[ax] : pb[ax]) - o[ax]) / d[ax];
        const int k = (int)(cert_unit(st) * 33.f) - 16;
        t = __int_as_float(__float_as_int(q) + (q >= 0.f ? k : -k));
    } else {
        t = 200.f * cert_unit(st);
    }
    const float tmin = 1e-3f;
    if (!(t > tmin && t < DEFAULT_RAY_TMAX)) return false;   // not a winner's distance
    Ray r;
    r.o = mk(o[0], o[1], o[2]);
    r.d = mk(d[0], d[1], d[2]);
    r.tmin = tmin;
    r.tmax = DEFAULT_RAY_TMAX;
    const RayK rk = make_rayk(r);
    const bool cert = cert_inside(box, rk, t);
    const bool exact = !slab_reject<true>(box, with_slab(rk), t);
    return which == 14 ? cert && !exact : (which == 15 ? cert : exact);
}

// Exhaustive checks of the lobe's short transcendentals (cpt_device.hpp lobe_pow, lobe_sincos)
// against the full dm:: sequences, over the float patterns [0, n) (cpt_selftest_qdiv):
// which = 8: lobe_pow(x, y) vs (float)dm::pow(x, y), y = the double with the bits of `seed`;
// 9: how many x take pow's fallback; 10: lobe_sincos(phi) vs dm::sincosf_(phi), both results;
// 11: how many phi take sincos' fallback; 12: miss_atanf / miss_asinf vs dm::atanf_ / dm::asinf_;
// 13: how many x take either one's fallback (asinf: x in [-1, 1]); 17: lobe_pow vs (float)dm::pow
// at hashed material exponents, for the indices [0, n): smoothness s = a hash of (seed, i >> 20)
// in [0, 6], y = 1.0 / (double)dm::powf_(1000.0f, s) as k_prepare_materials forms it, x = a hash
// of (seed, i) over the float patterns of [2^-33, 1] (the lobe's x_1 range); 18: how many of the
// same (x, y) take pow's fallback.  out[0] = count, out[1..] = some of the floats' bits (17, 18:
// s in the low word).
__global__ void k_selftest_fm(int which, uint64_t n, uint64_t seed, unsigned long long* out, int out_len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const double y = __longlong_as_double((long long)seed);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float x = __uint_as_float((uint32_t)i);
        uint32_t low = 0u;
        bool flag;
        if (which >= 17) {
            const uint64_t key = seed * 0x9e3779b97f4a7c15ULL;
            const float s = (float)(hash32(key + (i >> 20)) >> 8) * (6.0f / 16777215.0f);
            const double ys = 1.0 / (double)dm::powf_(1000.0f, s);
            // 0x2f000000 = 2^-33 .. 0x3f800000 = 1.0f: 0x10800001 patterns
            x = __uint_as_float(0x2f000000u + (uint32_t)(((uint64_t)hash32(~key + i) * 0x10800001ull) >> 32));
            low = __float_as_uint(s);
            if (which == 17) {
                flag = __float_as_uint(lobe_pow(x, ys)) != __float_as_uint((float)dm::pow((double)x, ys));
            } else {
                bool ok;
                (void)fm::pow_unit(x, ys, ok);
                flag = !ok && !(ys == 0.5 && x >= 0x1p-42f);
            }
        } else if (which >= 14) {
            flag = cert_case(seed, i, which);
        } else if (which == 8) {
            flag = __float_as_uint(lobe_pow(x, y)) != __float_as_uint((float)dm::pow((double)x, y));
        } else if (which == 9) {
            bool ok;
            (void)fm::pow_unit(x, y, ok);
            flag = !ok && !(y == 0.5 && x >= 0x1p-42f);
        } else if (which == 12) {
            flag = __float_as_uint(miss_atanf(x)) != __float_as_uint(dm::atanf_(x)) ||
                   __float_as_uint(miss_asinf(x)) != __float_as_uint(dm::asinf_(x));
        } else if (which == 13) {
            bool ok1, ok2;
            (void)fm::atan_ratio(__builtin_fabs((double)x), 1.0, ok1);
            const double xd = (double)x;
            (void)fm::atan_ratio(__builtin_fabs(xd), __builtin_sqrt((1.0 - xd) * (1.0 + xd)), ok2);
            flag = !ok1 || (!ok2 && x >= -1.0f && x <= 1.0f);
        } else if (which == 10) {
            float s, c, s_ref, c_ref;
            lobe_sincos(x, &s, &c);
            dm::sincosf_(x, &s_ref, &c_ref);
            flag = __float_as_uint(s) != __float_as_uint(s_ref) || __float_as_uint(c) != __float_as_uint(c_ref);
        } else {
            double s, c;
            bool ok;
            fm::sincos_2pi(x, s, c, ok);
            flag = !ok;
        }
        if (flag) {
            unsigned long long k = atomicAdd(&out[0], 1ull);
            if ((long long)k + 1 < out_len) out[k + 1] = ((unsigned long long)__float_as_uint(x) << 32) | low;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// k_denoise_rows (round 5, the default): the same Denoising + Mix, bit for bit, as a sliding
// window down a strip of columns (path_tracer.cu:177-254).
//  * A block owns a strip of 60 output columns (lanes 2..61 of each wave; lanes 0, 1, 62, 63 carry
//    the two halo columns each side) and a run of output rows.  Lane j of row Y holds the pixel of
//    LINEAR index L = Y W' + c0 - 2 + j: the stencil's v W' + u offsets (path_tracer.cu:205-216),
//    so columns past either edge wrap into the adjacent row exactly as the reference's do.
//  * When row R enters, the 12 pair weights whose later pixel is (R, j) are computed: the two
//    same-row pairs (R, j+1), (R, j+2) and the pairs with rows R-1 and R-2 at columns j-2..j+2 --
//    every unordered pair of the stencil exactly once -- into a ring of weights in LDS.
//  * Row O = R - 2 is then complete: each output lane sums its 25 taps in the reference's order,
//    reading the weights it needs from the ring (its own, or a neighbour's at lane j +- u).
// The weights are evaluated in batches of DN_BATCH with one wave-wide fallback branch
// (dn_weight's guard), so the batch's exp chains overlap.
constexpr int DNS_LANES = 64, DNS_COLS = 60;
struct DnsPix { float4 rgbv; float4 nd; };   // (r, g, b, valid), (nx, ny, nz, depth)
// The ring is two SoA arrays of float4 (16-B lane stride): a wave's ds_read_b128 at consecutive
// lanes then covers all 64 banks once per 16-lane group (MI355X_MICROARCH.md §LDS), where the
// 32-B pixel struct put two lanes of a group on the same banks (57% of LDS cycles were conflicts).

// Pair weights c_w * n_w * p_w of N pairs (path_tracer.cu:219-233; dn_pair_weight's factors, in
// the same order), batched: N short exps in flight, and the guard's rare fallback as one branch.
template <int N>
__device__ __forceinline__ void dn_weights(const float d2[N], float w[N], const double* __restrict__ tab) {
    uint32_t slow = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double e = dn_exp_short(d2[i], tab);
        w[i] = (float)e;
        slow |= dn_near_midpoint(e) && !(d2[i] >= 330.0f) ? 1u << i : 0u;
    }
    // the fallback, one call site per batch: each trip serves every lane's lowest pending weight
    while (__builtin_expect(__builtin_amdgcn_ballot_w64(slow != 0) != 0, 0)) {
        const int k = slow ? __builtin_ctz(slow) : -1;
        float x = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) x = k == i ? d2[i] : x;
        float r = 0.0f;
        if (k >= 0) r = dn_weight_slow_inl(x);
#pragma unroll
        for (int i = 0; i < N; ++i) w[i] = k == i ? r : w[i];
        slow &= slow - 1u;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        w[i] = d2[i] >= 330.0f ? 0.0f : w[i];
        w[i] = d2[i] == 0.0f ? 1.0f : w[i];
    }
}

// The three squared differences of one pair (path_tracer.cu:221-231): colour, normal (clamped at
// 0: (float)max((double)dn, 0.0), the reference's clamp in double), depth.
__device__ __forceinline__ void dn_pair_dist(const DnsPix& a, const DnsPix& b, float& c2, float& n2, float& p2) {
    v3 t = mk(a.rgbv.x, a.rgbv.y, a.rgbv.z) - mk(b.rgbv.x, b.rgbv.y, b.rgbv.z);
    c2 = dot(t, t);
    t = mk(a.nd.x, a.nd.y, a.nd.z) - mk(b.nd.x, b.nd.y, b.nd.z);
    const float dn = dot(t, t);
    n2 = dn > 0.0f ? dn : 0.0f;
    p2 = (a.nd.w - b.nd.w) * (a.nd.w - b.nd.w);
}

// c_w * n_w * p_w (left to right) of N pairs from their squared differences.
template <int N>
__device__ __forceinline__ void dn_dist_weights(const float c2[N], const float n2[N], const float p2[N], float out[N],
                                                const double* __restrict__ tab) {
    bool any_n = false, any_p = false;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        any_n |= n2[i] != 0.0f;
        any_p |= p2[i] != 0.0f;
    }
    float cw[N], nw[N], pw[N];
    dn_weights<N>(c2, cw, tab);
    // a zero normal (depth) difference gives exactly 1 (dn_weight(0)); equal normals (the floor)
    // and the constant depth (a18) make whole batches of the wave skip the sequence
#pragma unroll
    for (int i = 0; i < N; ++i) nw[i] = pw[i] = 1.0f;
    if (__builtin_amdgcn_ballot_w64(any_n)) dn_weights<N>(n2, nw, tab);
    if (__builtin_amdgcn_ballot_w64(any_p)) dn_weights<N>(p2, pw, tab);
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = cw[i] * nw[i] * pw[i];
}

template <int N>
__device__ __forceinline__ void dn_pair_weights(const DnsPix a[N], const DnsPix& b, float out[N],
                                                const double* __restrict__ tab) {
    float c2[N], n2[N], p2[N];
#pragma unroll
    for (int i = 0; i < N; ++i) dn_pair_dist(a[i], b, c2[i], n2[i], p2[i]);
    dn_dist_weights<N>(c2, n2, p2, out, tab);
}

// Exhaustive check of the shipped weight (dn_weights: the short exp, the guard, the slow form's
// fallback and the 0 / >= 330 shortcuts) against dn_weight_slow (cpt_selftest_qdiv which = 6:
// mismatches over the float patterns [0, n); which = 7: how many of them take the fallback).
__global__ void k_selftest_dn_weight(int which, uint64_t n, unsigned long long* out, int out_len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float d = __uint_as_float((uint32_t)i);
        bool flag;
        if (which == 6) {
            float w;
            dn_weights<1>(&d, &w, g_dn_exp_table);
            const float w_ref = dn_weight_slow(d);
            flag = __float_as_uint(w) != __float_as_uint(w_ref);
        } else {
            const double e = dn_exp_short(d, g_dn_exp_table);
            flag = dn_near_midpoint(e) && !(d >= 330.0f);
        }
        if (flag) {
            unsigned long long k = atomicAdd(&out[0], 1ull);
            if ((long long)k + 1 < out_len) out[k + 1] = ((unsigned long long)__float_as_uint(d) << 32);
        }
    }
}

// The block's n waves (DNR_WAVES, 8) share the window: per super-step they take the next n
// rows, wave w row R = B + w:
//   1. each wave writes its row into the block's pixel ring (2n + 4 rows: the n new ones never
//      alias the n + 4 the other waves may still be reading for their taps);
//   barrier;
//   2. each wave computes its row's 12 pair weights into the block's weight ring (n + 2 rows),
//      then issues the loads of row R + n (the prefetch) and of its output row's mix;
//   barrier;
//   3. each wave finalizes output row O = R - 2 from the weights of rows O .. O + 2 and the pixel
//      rows O - 2 .. O + 2, in the reference's tap order, and stores it.
// Occupancy is the lever this kernel answered to (round 5, profiles/r05/ab_display_*.log, C4
// device frame): one wave per strip with its own 19.5 KB ring (k_denoise_strip, retired) 0.127 ms;
// 4-wave blocks sharing the rings, 3 waves per SIMD (150 VGPRs) 0.106-0.109; out-of-frame pairs
// stored as weight 0 so the taps need no branch (138 VGPRs) 0.097; 8-wave blocks at 4 waves per
// SIMD, batches of 4 pair weights and the loads issued after the pair weights (124 VGPRs, no
// spill) 0.090-0.092 (with the loads ahead of the pairs: 14 VGPRs spilled, 0.093-0.099).
// Loads are issued unconditionally (out-of-frame lanes read a valid address and discard it)
// and the stores sit in a branch-free tail (lanes without an output pixel store to `sink`), so
// the next row's wait does not drain a branch's worth of stores.
// pixel ring: the n new rows + the 2n + 4 - n rows a slower wave may still read for its taps;
// weight ring: the n + 2 rows the taps of one super-step read
constexpr int DNR_WAVES = 8, DNR_PIX_ROWS = 2 * DNR_WAVES + 4, DNR_W_ROWS = DNR_WAVES + 2;
constexpr int DNR_MINWAVES = 4;        // __launch_bounds__ waves per SIMD (<= 128 VGPRs)
constexpr int DNR_BLOCKS_PER_CU = 2;   // 8-wave blocks, 4 waves per SIMD
constexpr int DN_BATCH = 4;            // pair weights evaluated together (a divisor of 12)
// the static LDS of one block: the exp table, the two pixel rings, the weight ring (78 KB)
constexpr size_t DNR_LDS_BYTES = DN_EXP_N * sizeof(double) + 2 * DNR_PIX_ROWS * DNS_LANES * sizeof(float4) +
                                 DNR_W_ROWS * 12 * DNS_LANES * sizeof(float);
static_assert(DNR_LDS_BYTES * DNR_BLOCKS_PER_CU <= 160 * 1024, "k_denoise_rows: blocks per CU exceed the CU's LDS");

template <bool HOST>
__global__ void __launch_bounds__(DNS_LANES * DNR_WAVES, DNR_MINWAVES) k_denoise_rows(
    const float4* __restrict__ accum, const float* __restrict__ normal, const float* __restrict__ depth,
    float* __restrict__ mix, uint8_t* __restrict__ out, uint8_t* __restrict__ out_host, float4* __restrict__ sink,
    int width, int row0, int ctx_rows, int y0, int y1, int w_eff, int h_eff, int n_strips, int per_strip, float inv_idx) {
    __shared__ double s_tab[DN_EXP_N];
    __shared__ float4 rgbv[DNR_PIX_ROWS][DNS_LANES];
    __shared__ float4 ndr[DNR_PIX_ROWS][DNS_LANES];
    __shared__ float W[DNR_W_ROWS][12][DNS_LANES];
    for (int i = threadIdx.x; i < DN_EXP_N; i += DNS_LANES * DNR_WAVES) s_tab[i] = g_dn_exp_table[i];
    const int wv = (int)(threadIdx.x >> 6), j = (int)(threadIdx.x & 63);
    const int strip = (int)blockIdx.x % n_strips, part = (int)blockIdx.x / n_strips;
    const int nrow = y1 - y0;
    const int ra = y0 + (int)((long long)nrow * part / per_strip), rb = y0 + (int)((long long)nrow * (part + 1) / per_strip);
    const int c0 = strip * DNS_COLS;
    const int col = c0 - 2 + j;
    const int limit = w_eff * h_eff;
    const bool out_lane = j >= 2 && j < 2 + DNS_COLS && col < w_eff;
    float4* const sink_lane = sink + ((((uint32_t)blockIdx.x * DNR_WAVES + (uint32_t)wv) & 1023u) * 64u + (uint32_t)j);
    auto ring = [&](int row, int lane) {
        const int sl = (row + 4 * DNR_PIX_ROWS) % DNR_PIX_ROWS;
        return DnsPix{rgbv[sl][lane], ndr[sl][lane]};
    };
    auto cl = [](int l) { return l < 0 ? 0 : (l > 63 ? 63 : l); };
    auto load = [&](int Y, float4& a, float3& n, float& d, bool& valid) {
        const int L = Y * w_eff + col;
        valid = L >= 0 && L < limit;
        const int yy = col < 0 ? Y - 1 : (col >= w_eff ? Y + 1 : Y);
        const int xx = L - yy * w_eff;
        // the window reads up to a super-step past the rows it outputs; rows the context does not
        // hold (a band's, cpt_denoise_mix_band) are never a tap or pair of an output pixel, so
        // they read address 0 like the out-of-frame ones
        // (lanes past 2 W' of a narrow frame -- 16 or 32 columns -- wrap beyond the next row:
        // never a tap either, and outside the row they must not address)
        const bool held = yy - row0 >= 0 && yy - row0 < ctx_rows && xx >= 0 && xx < w_eff;
        const size_t px = valid && held ? (size_t)(yy - row0) * width + xx : (size_t)0;
        a = accum[px];
        n = make_float3(normal[3 * px], normal[3 * px + 1], normal[3 * px + 2]);
        d = depth[px];
    };
    auto put = [&](int Y, const float4& na, const float3& nn, float nd, bool nvalid) {
        const float4 a = nvalid ? na : make_float4(0.f, 0.f, 0.f, 0.f);
        const v3 c = a.w != 0.f ? mk(a.x, a.y, a.z) / a.w : mk(a.x, a.y, a.z);
        const int sl = (Y + 4 * DNR_PIX_ROWS) % DNR_PIX_ROWS;
        rgbv[sl][j] = make_float4(c.x, c.y, c.z, nvalid ? 1.f : 0.f);
        ndr[sl][j] = nvalid ? make_float4(nn.x, nn.y, nn.z, nd) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    constexpr float kernel5[5][5] = {{1.f, 4.f, 7.f, 4.f, 1.f},
                                     {4.f, 16.f, 26.f, 16.f, 4.f},
                                     {7.f, 26.f, 41.f, 26.f, 7.f},
                                     {4.f, 16.f, 26.f, 16.f, 4.f},
                                     {1.f, 4.f, 7.f, 4.f, 1.f}};
    // rows ra - 2 and ra - 1 (waves 0, 1): the pairs of rows ra, ra + 1 reach back into them
    float4 na;
    float3 nn;
    float nd;
    bool nvalid;
    if (wv < 2) {
        load(ra - 2 + wv, na, nn, nd, nvalid);
        put(ra - 2 + wv, na, nn, nd, nvalid);
    }
    load(ra + wv, na, nn, nd, nvalid);
#pragma unroll 1
    for (int B = ra; B - 2 < rb; B += DNR_WAVES) {
        const int R = B + wv;           // this wave's new row
        const int O = R - 2;            // the output row it finalizes
        float3 mix_cur;
        auto load_mix = [&]() {
            const int orow = min(max(O, ra), rb - 1);
            const int ocol = min(max(col, 0), w_eff - 1);
            const size_t b = (size_t)(orow - y0) * width + ocol;
            mix_cur = make_float3(mix[3 * b], mix[3 * b + 1], mix[3 * b + 2]);
        };
        put(R, na, nn, nd, nvalid);
        const DnsPix me = ring(R, j);   // (this lane's own write: ordered)
        __syncthreads();
        // ---- the 12 pair weights whose later pixel is (R, j) ---------------------------------------
        {
            float w12[12];
            // partner k of the 12 (k = 0, 1: (R, j + k + 1); 2..6: (R - 1, j + k - 4); 7..11:
            // (R - 2, j + k - 9)), in batches of DN_BATCH pairs
            auto partner = [&](int k) {
                return k < 2 ? ring(R, cl(j + k + 1)) : (k < 7 ? ring(R - 1, cl(j + k - 4)) : ring(R - 2, cl(j + k - 9)));
            };
#pragma unroll
            for (int k0 = 0; k0 < 12; k0 += DN_BATCH) {
                DnsPix a[DN_BATCH];
#pragma unroll
                for (int i = 0; i < DN_BATCH; ++i) a[i] = partner(k0 + i);
                dn_pair_weights<DN_BATCH>(a, me, w12 + k0, s_tab);
                // a pair with an out-of-frame pixel weighs +0 (the reference's c_w = n_w = p_w = 0),
                // so the taps need no branch: such a pixel's ring colour is +0 as well
#pragma unroll
                for (int i = 0; i < DN_BATCH; ++i)
                    w12[k0 + i] = a[i].rgbv.w != 0.f && me.rgbv.w != 0.f ? w12[k0 + i] : 0.f;
            }
            const int ws = (R + 4 * DNR_W_ROWS) % DNR_W_ROWS;
#pragma unroll
            for (int k = 0; k < 12; ++k) W[ws][k][j] = w12[k];
        }
        // the row a super-step ahead and the output row's mix, loaded after the pair weights (fewer
        // registers live through them)
        load(R + DNR_WAVES, na, nn, nd, nvalid);
        load_mix();
        __syncthreads();
        // ---- output row O (wave-uniform condition; every lane computes, out_lane stores) --------
        v3 st_m = mk1(0.f);
        uint32_t st_bgr = 0;
        bool st_real = false;
        if (O >= ra && O < rb) {
            const int wO = (O + 4 * DNR_W_ROWS) % DNR_W_ROWS, wO1 = (O + 1 + 4 * DNR_W_ROWS) % DNR_W_ROWS,
                      wO2 = (O + 2 + 4 * DNR_W_ROWS) % DNR_W_ROWS;
            const int jc = min(max(j, 2), 61);
            const DnsPix p = ring(O, jc);
            const bool finite = __builtin_isfinite(p.rgbv.x) && __builtin_isfinite(p.rgbv.y) &&
                                __builtin_isfinite(p.rgbv.z) && __builtin_isfinite(p.nd.x) &&
                                __builtin_isfinite(p.nd.y) && __builtin_isfinite(p.nd.z) && __builtin_isfinite(p.nd.w);
            float w_self = 1.0f;
            if (!finite) {
                float ws1[1];
                dn_pair_weights<1>(&p, p, ws1, s_tab);
                w_self = ws1[0];
            }
            v3 sum = mk1(0.f);
            float cum_w = 0.0f;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
#pragma unroll
                for (int jj = 0; jj < 5; ++jj) {
                    const int u = i - 2, v = jj - 2;
                    const float4 q = rgbv[(O + v + 4 * DNR_PIX_ROWS) % DNR_PIX_ROWS][jc + u];
                    // (an out-of-frame q holds colour +0 and its pair weight +0: the reference's
                    // zero weight, without a branch)
                    const v3 ctmp = mk(q.x, q.y, q.z);
                    // where the pair (O, j) - (O + v, j + u) was stored: same row -- by the lane
                    // of its left pixel, as that pixel's forward pair |u| - 1; other rows -- by
                    // the lane of its lower pixel, at index 2 + dx + 2 (dy 1) or 7 + dx + 2
                    // (dy 2), dx = upper column - lower column
                    float weight;
                    if (u == 0 && v == 0) weight = w_self;
                    else if (v == 0 && u > 0) weight = W[wO][u - 1][jc];
                    else if (v == 0) weight = W[wO][-u - 1][jc + u];
                    else if (v < 0) weight = W[wO][v == -1 ? 2 + (u + 2) : 7 + (u + 2)][jc];
                    else weight = W[v == 1 ? wO1 : wO2][v == 1 ? 2 + (-u + 2) : 7 + (-u + 2)][jc + u];
                    sum = sum + (weight * kernel5[i][jj]) * ctmp;
                    cum_w += weight * kernel5[i][jj];
                }
            }
            const v3 dn = sum / cum_w;
            const v3 clp = mk(__builtin_fmaxf(0.f, __builtin_fminf(dn.x, 1.f)), __builtin_fmaxf(0.f, __builtin_fminf(dn.y, 1.f)),
                              __builtin_fmaxf(0.f, __builtin_fminf(dn.z, 1.f)));
            v3 m = mk(mix_cur.x, mix_cur.y, mix_cur.z);
            m = m + inv_idx * (clp - m);   // lerp (helper_math.h:1154-1157)
            st_m = m;
            st_bgr = (uint32_t)(uint8_t)(255.99f * m.z) | ((uint32_t)(uint8_t)(255.99f * m.y) << 8) |
                     ((uint32_t)(uint8_t)(255.99f * m.x) << 16);
            st_real = out_lane;
        }
        {
            const size_t bself = st_real ? (size_t)(O - y0) * width + col : 0;
            float* const pm = st_real ? mix + 3 * bself : reinterpret_cast<float*>(sink_lane);
            uint32_t* const po = st_real ? reinterpret_cast<uint32_t*>(out) + bself : reinterpret_cast<uint32_t*>(sink_lane) + 3;
            pm[0] = st_m.x;
            pm[1] = st_m.y;
            pm[2] = st_m.z;
            *po = st_bgr;
            if (HOST) {
                uint32_t* const ph = st_real ? reinterpret_cast<uint32_t*>(out_host) + bself : reinterpret_cast<uint32_t*>(sink_lane) + 3;
                *ph = st_bgr;
            }
        }
    }
}

hipError_t launch_denoise_mix(const float4* accum, const float* normal, const float* depth, float* mix, uint8_t* out,
                              uint8_t* out_host, float4* sink, int width, int height, int row0, int ctx_rows, int y0, int y1,
                              uint32_t cur_sample_idx, hipStream_t stream) {
    const int w_eff = 16 * (width / 16), h_eff = 16 * (height / 16);
    if (w_eff == 0 || h_eff == 0 || y1 <= y0) return hipSuccess;
    const float inv_idx = 1.f / float(cur_sample_idx);
    static int cus2[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    if (cus2[dev] == 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus2[dev] = n;
    }
    const int n_strips = (w_eff + DNS_COLS - 1) / DNS_COLS;
    const int rows = y1 - y0;
    int per_strip = (cus2[dev] * DNR_BLOCKS_PER_CU + n_strips - 1) / n_strips;
    per_strip = per_strip < 1 ? 1 : (per_strip > rows ? rows : per_strip);
    const unsigned blocks = (unsigned)(n_strips * per_strip);
    if (out_host)
        hipLaunchKernelGGL(k_denoise_rows<true>, dim3(blocks), dim3(DNS_LANES * DNR_WAVES), 0, stream, accum, normal, depth, mix,
                           out, out_host, sink, width, row0, ctx_rows, y0, y1, w_eff, h_eff, n_strips, per_strip, inv_idx);
    else
        hipLaunchKernelGGL(k_denoise_rows<false>, dim3(blocks), dim3(DNS_LANES * DNR_WAVES), 0, stream, accum, normal, depth, mix,
                           out, out_host, sink, width, row0, ctx_rows, y0, y1, w_eff, h_eff, n_strips, per_strip, inv_idx);
    return hipGetLastError();
}

// ======================================================================================
// Row-tile gather (cpt_gather_rows): a source context's rows, copied to this device as one
// block (accumulator float4s, then first-hit normals and depths), are scattered to the rows
// the destination frame holds them at.  One thread per pixel; every access is coalesced.
// ======================================================================================
__global__ void __launch_bounds__(256) k_stitch_rows(const float4* __restrict__ src_acc, const float* __restrict__ src_nrm,
                                                     const float* __restrict__ src_dep, const int32_t* __restrict__ dst_row,
                                                     int width, float4* __restrict__ acc, float* __restrict__ nrm,
                                                     float* __restrict__ dep) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (x >= width) return;
    const size_t s = (size_t)r * width + x, d = (size_t)dst_row[r] * width + x;
    acc[d] = src_acc[s];
    if (src_nrm) {
        nrm[3 * d] = src_nrm[3 * s];
        nrm[3 * d + 1] = src_nrm[3 * s + 1];
        nrm[3 * d + 2] = src_nrm[3 * s + 2];
        dep[d] = src_dep[s];
    }
}

hipError_t launch_stitch_rows(const float4* src_acc, const float* src_nrm, const float* src_dep, const int32_t* dst_row,
                              int width, int n_rows, float4* acc, float* nrm, float* dep, hipStream_t stream) {
    if (width <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_stitch_rows, dim3((width + 255) / 256, n_rows), dim3(256), 0, stream, src_acc, src_nrm, src_dep,
                       dst_row, width, acc, nrm, dep);
    return hipGetLastError();
}

// ======================================================================================
// Device-math KAT (see cpt.h cpt_math_batch).
// ======================================================================================
__global__ void k_math_batch(int op, const float* a, const float* b, float* out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float x = a[i], y = b[i], r;
    switch (op) {
        case 0: r = dm::powf_(x, y); break;
        case 1: { float s, c; dm::sincosf_(x, &s, &c); r = s; break; }
        case 2: { float s, c; dm::sincosf_(x, &s, &c); r = c; break; }
        case 3: r = dm::asinf_(x); break;
        case 4: r = dm::atanf_(x); break;
        case 5: r = (float)dm::pow((double)x, 1.0 / (double)y); break;
        case 6: r = (float)((double)x / (double)y); break;
        case 7: r = x / y; break;
        case 8: r = __builtin_sqrtf(x); break;
        case 9: r = dm::pow5f(x); break;
        case 10: r = lobe_pow(x, 1.0 / (double)y); break;
        default: r = __builtin_nanf("");
    }
    out[i] = r;
}

// ======================================================================================
// Host-side launchers (called from cpt_capi.cpp).
// ======================================================================================
template <bool S, bool A, bool P, bool T, bool C = false, bool H = false>
static hipError_t launch_mk(const KParams& p, hipStream_t stream) {
    static int blocks_per_cu = -1, cus = 0;
    constexpr int block = mk_block<T>();
    if (blocks_per_cu < 0) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (e == hipSuccess)
            e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, k_megakernel<S, A, P, T, C, H>, block, 0);
        if (e != hipSuccess) return e;
        if (blocks_per_cu < 1) blocks_per_cu = 1;
    }
    // persistent grid: every resident slot once; lanes pull pixels from p.work
    const long long tiles = (long long)((p.width + 7) / 8) * ((p.n_rows + 7) / 8);
    // a wave holds p.lanes / p.replicate pixels at once (64 in normal use; fewer: DIAGNOSTIC)
    const int per_wave = std::max(1, p.lanes / std::max(1, p.replicate));
    long long want = (tiles * 64 * ((64 + per_wave - 1) / per_wave) + block - 1) / block;
    long long grid = std::min<long long>(want, (long long)blocks_per_cu * cus);
    if (grid < 1) return hipSuccess;
    hipLaunchKernelGGL((k_megakernel<S, A, P, T, C, H>), dim3((unsigned)grid), dim3(block), 0, stream, p);
    return hipGetLastError();
}

// The wide walk (ordered walk on a 4-wide tree) runs in the LDS kernels: the image's first
// LDS_TREE_NODES nodes in LDS, the rest of a larger tree from global memory.
static bool use_lds_tree(const KParams& p) { return p.ordered == 1 && p.n_wide > 0; }

template <bool S, bool A, bool P, bool H>
static hipError_t launch_mk_lds(const KParams& p, hipStream_t stream) {
    if constexpr (!P && ho_slots<mk_block<true>()>() > 0) {
        if (p.resume) return launch_mk<S, A, P, true, true, H>(p, stream);   // tail consolidation
    }
    return launch_mk<S, A, P, true, false, H>(p, stream);
}

template <bool S, bool A, bool P>
static hipError_t launch_mk_any(const KParams& p, hipStream_t stream) {
    if (!use_lds_tree(p)) return launch_mk<S, A, P, false>(p, stream);
    if (p.n_wide > LDS_TREE_NODES) return launch_mk_lds<S, A, P, true>(p, stream);
    return launch_mk_lds<S, A, P, false>(p, stream);
}

hipError_t launch_megakernel(const KParams& p, bool stats, bool aux, hipStream_t stream) {
    if (p.width <= 0 || p.n_rows <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(p.work, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (stats && aux) return launch_mk_any<true, true, false>(p, stream);
    if (stats) return launch_mk_any<true, false, false>(p, stream);
    if (aux) return launch_mk_any<false, true, false>(p, stream);
    return launch_mk_any<false, false, false>(p, stream);
}

// ======================================================================================
// Cost schedule (CPT_SCHEDULE_COST, DESIGN.md §Cost schedule).  A pilot of `passes` passes
// from the current RNG states (nothing written back) sums each 8x8 tile's work; the tiles are
// then sorted heaviest first and the render dequeues them in that order (longest processing
// time first), so the heaviest pixel chains start at once instead of behind the light ones.
// ======================================================================================
__global__ void k_iota(uint32_t* v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

size_t tile_schedule_scratch_bytes(int width, int n_rows) {
    const int n = ((width + 7) / 8) * ((n_rows + 7) / 8);
    size_t temp = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, n);
    return 3 * (size_t)n * sizeof(uint32_t) + temp + 256;
}

// CPT_SCHEDULE_PREVIOUS: one wave per 8x8 tile; lane k = pixel k of the tile (decode_pixel's
// layout).  A pixel's draws since the last call are (d - d_prev) / 362437 mod 2^32 (every
// curand() adds 362437 to d, an odd number: a multiplication by its inverse mod 2^32).
__global__ void __launch_bounds__(64) k_tile_draws(const uint32_t* __restrict__ d_now, uint32_t* __restrict__ d_prev,
                                                   int width, int n_rows, uint32_t* __restrict__ cost) {
    constexpr uint32_t WEYL = 362437u;
    constexpr uint32_t INV = [] {   // WEYL^-1 mod 2^32 (Newton: x <- x (2 - WEYL x))
        uint32_t x = WEYL;
        for (int i = 0; i < 5; ++i) x *= 2u - WEYL * x;
        return x;
    }();
    static_assert(WEYL * INV == 1u, "inverse of the Weyl step");
    const int tiles_x = (width + 7) >> 3;
    const uint32_t tile = blockIdx.x;
    const int k = threadIdx.x;
    const int x = (int)(tile % tiles_x) * 8 + (k & 7), ri = (int)(tile / tiles_x) * 8 + (k >> 3);
    uint32_t draws = 0;
    if (x < width && ri < n_rows) {
        const size_t pix = (size_t)ri * width + x;
        const uint32_t d = d_now[pix];
        draws = (d - d_prev[pix]) * INV;
        d_prev[pix] = d;
    }
    // (the sum: keying 1-spp tiles by their heaviest pixel's draws, as the cost pilot does, was
    // slower here, 1.59-1.62 vs 1.57-1.59 ms per pass, profiles/r06/ab_prevmax.log)
    const uint64_t sum = wave_sum(draws);
    if (k == 0) cost[tile] = (uint32_t)(sum < 0xffffffffull ? sum : 0xffffffffull);
}

hipError_t launch_tile_order_from_draws(const KParams& p, uint32_t* d_prev, void* scratch, size_t scratch_bytes,
                                        uint32_t* order, hipStream_t stream) {
    const int n = ((p.width + 7) / 8) * ((p.n_rows + 7) / 8);
    if (n <= 0) return hipSuccess;
    uint32_t* cost = (uint32_t*)scratch;
    uint32_t* cost_sorted = cost + n;
    uint32_t* ids = cost_sorted + n;
    void* temp = (void*)(((uintptr_t)(ids + n) + 255) & ~(uintptr_t)255);
    size_t temp_bytes = scratch_bytes - ((char*)temp - (char*)scratch);
    const size_t npix = (size_t)p.n_rows * p.width;
    hipLaunchKernelGGL(k_tile_draws, dim3((unsigned)n), dim3(64), 0, stream, p.rng + 5 * npix, d_prev, p.width,
                       p.n_rows, cost);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, stream, ids, (uint32_t)n);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairsDescending(temp, temp_bytes, cost, cost_sorted, ids, order, n, 0, 32,
                                                        stream);
}

hipError_t launch_tile_schedule(const KParams& p0, int passes, void* scratch, size_t scratch_bytes, uint32_t* order,
                                hipStream_t stream) {
    const int n = ((p0.width + 7) / 8) * ((p0.n_rows + 7) / 8);
    if (n <= 0) return hipSuccess;
    uint32_t* cost = (uint32_t*)scratch;
    uint32_t* cost_sorted = cost + n;
    uint32_t* ids = cost_sorted + n;
    void* temp = (void*)(((uintptr_t)(ids + n) + 255) & ~(uintptr_t)255);
    size_t temp_bytes = scratch_bytes - ((char*)temp - (char*)scratch);
    hipError_t e = hipMemsetAsync(cost, 0, (size_t)n * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p0.work, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    KParams p = p0;
    p.spp = passes;
    p.tile_cost = cost;
    p.tile_order = nullptr;
    p.accumulate = 0;
    e = launch_mk_any<false, false, true>(p, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, stream, ids, (uint32_t)n);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipcub::DeviceRadixSort::SortPairsDescending(temp, temp_bytes, cost, cost_sorted, ids, order, n, 0, 32,
                                                        stream);
}

// ======================================================================================
// Device refit (SceneBVH::UpdateObject / UpdateSceneBVH, bvh.cu:122-157).  The reference refits
// the updated leaf's ancestors on the host and copies the whole node array back to the GPU;
// here the host only names the updated leaves and their dirty ancestors (cpt_capi.cpp
// device_refit) and the boxes are recomputed where the nodes live, for both trees at once:
// the reference order, the walk tree's eight octant orders, its 4-wide image and leaf array.
// One thread per node; a launch per height, so a node's children are final before it runs.
// ======================================================================================
__device__ __forceinline__ float refit_min(float a, float b) { return a < b ? a : b; }   // MIN_ (ray_tracing_math.hpp:19-21)
__device__ __forceinline__ float refit_max(float a, float b) { return a > b ? a : b; }   // MAX_ (:15-17)

// A node's inline primitive into one of its copies (each copy keeps its own `miss`).
__device__ __forceinline__ void refit_put_prim(Node* n, const Node& v) {
    n->a0 = v.a0; n->a1 = v.a1; n->a2 = v.a2;
    n->b0 = v.b0; n->b1 = v.b1; n->b2 = v.b2;
    n->code = v.code;
}

// An internal node's box into one of its copies: octant form for the walk tree's octant
// orders (cpt_capi.cpp linearise: the planes a ray of the octant enters through in a).
__device__ __forceinline__ void refit_put_box(Node* n, const Box6& b, int oct) {
    const bool sx = oct & 1, sy = oct & 2, sz = oct & 4;
    n->a0 = sx ? b.hi[0] : b.lo[0]; n->b0 = sx ? b.lo[0] : b.hi[0];
    n->a1 = sy ? b.hi[1] : b.lo[1]; n->b1 = sy ? b.lo[1] : b.hi[1];
    n->a2 = sz ? b.hi[2] : b.lo[2]; n->b2 = sz ? b.lo[2] : b.hi[2];
}

// A slot of the 4-wide image (7 x 16 B per node: [min x][max x][min y][max y][min z][max z] of
// the four slots, then the refs; cpt_capi.cpp linearise_wide).
__device__ __forceinline__ void refit_put_slot(uint32_t* image, int slot, const Box6& b) {
    uint32_t* q = image + (size_t)(slot >> 2) * 28;
    const int k = slot & 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[(2 * a) * 4 + k] = __float_as_uint(b.lo[a]);
        q[(2 * a + 1) * 4 + k] = __float_as_uint(b.hi[a]);
    }
}

__global__ void __launch_bounds__(256) k_refit_leaves(const RefitLeaf* __restrict__ in, int n,
                                                      const RefitNode* __restrict__ plan, Box6* boxes, Node* nodes,
                                                      uint32_t* image, Node* leaves) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RefitLeaf r = in[i];
    boxes[r.ref_id] = r.box;
    refit_put_prim(nodes + plan[r.ref_id].pos[0], r.prim);
    if (r.walk_id < 0) return;
    boxes[r.walk_id] = r.box;
    const RefitNode w = plan[r.walk_id];
#pragma unroll
    for (int o = 0; o < 8; ++o)
        if (w.pos[o] >= 0) refit_put_prim(nodes + w.pos[o], r.prim);
    if (w.leaf >= 0 && leaves) refit_put_prim(leaves + w.leaf, r.prim);
    if (w.slot >= 0 && image) refit_put_slot(image, w.slot, r.box);
}

__global__ void __launch_bounds__(256) k_refit_nodes(const int32_t* __restrict__ ids, int n, int n_ref,
                                                     const RefitNode* __restrict__ plan, Box6* boxes, Node* nodes,
                                                     uint32_t* image) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    const RefitNode r = plan[id];
    const Box6 L = boxes[r.left], R = boxes[r.right];
    Box6 b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // UPDATE_AABB_FOR_CUR_NODE (bvh.cu:130-139): MAX_/MIN_(left, right)
        b.hi[a] = refit_max(L.hi[a], R.hi[a]);
        b.lo[a] = refit_min(L.lo[a], R.lo[a]);
    }
    boxes[id] = b;
    if (id < n_ref) {
        refit_put_box(nodes + r.pos[0], b, 0);
    } else {
#pragma unroll
        for (int o = 0; o < 8; ++o) refit_put_box(nodes + r.pos[o], b, o);
    }
    if (r.slot >= 0 && image) refit_put_slot(image, r.slot, b);
}

hipError_t launch_refit(const RefitLeaf* leaves_in, int n_leaves, const int32_t* dirty, const int32_t* level_end,
                        int n_levels, int n_ref, const RefitNode* plan, Box6* boxes, Node* nodes, uint32_t* image,
                        Node* leaves, hipStream_t stream) {
    if (n_leaves > 0)
        hipLaunchKernelGGL(k_refit_leaves, dim3((n_leaves + 255) / 256), dim3(256), 0, stream, leaves_in, n_leaves, plan,
                           boxes, nodes, image, leaves);
    int begin = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int n = level_end[l] - begin;
        if (n > 0)
            hipLaunchKernelGGL(k_refit_nodes, dim3((n + 255) / 256), dim3(256), 0, stream, dirty + begin, n, n_ref, plan,
                               boxes, nodes, image);
        begin = level_end[l];
    }
    return hipGetLastError();
}

hipError_t launch_prepare_materials(Mat* mats, const int32_t* tex_of_mat, const TexDesc* texs, int n,
                                    hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_prepare_materials, dim3((n + 63) / 64), dim3(64), 0, stream, mats, tex_of_mat, texs, n);
    return hipGetLastError();
}

hipError_t launch_init_rng(const uint32_t* jumps, const uint32_t seed_state[6], int width, const int32_t* rows, int n_rows,
                           uint32_t* scratch_w, uint32_t* scratch_mats, uint32_t* rng, hipStream_t stream) {
    if (width <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rng_columns, dim3((width + 63) / 64), dim3(64), 0, stream, jumps, seed_state[0], seed_state[1],
                       seed_state[2], seed_state[3], seed_state[4], width, scratch_w);
    hipLaunchKernelGGL(k_rng_rowmats, dim3(n_rows), dim3(192), 0, stream, jumps, rows, scratch_mats);
    hipLaunchKernelGGL(k_rng_pixels, dim3((width + 255) / 256, n_rows), dim3(256), 0, stream, scratch_mats, scratch_w,
                       width, n_rows, seed_state[5], rng);
    return hipGetLastError();
}

hipError_t launch_math_batch(int op, const float* a, const float* b, float* out, size_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_math_batch, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, op, a, b, out, n);
    return hipGetLastError();
}

// ======================================================================================
// HBM streaming-read ceiling (confirm the roofline's peak on the box).
// Grid-stride 16-B loads over a buffer far larger than the 256 MiB Infinity Cache; the sum
// is stored only under a condition that never holds, so the kernel moves read bytes only.
// ======================================================================================
__global__ void __launch_bounds__(256) k_stream_read(const float4* __restrict__ p, size_t n, float* out) {
    float acc = 0.f;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float4 v = p[i];
        acc += (v.x + v.y) + (v.z + v.w);
    }
    if (acc == 1.2345e-30f) out[0] = acc;
}

hipError_t launch_stream_read(const float4* p, size_t n, float* out, int grid, hipStream_t stream) {
    hipLaunchKernelGGL(k_stream_read, dim3(grid), dim3(256), 0, stream, p, n, out);
    return hipGetLastError();
}

// FETCH_SIZE calibration (cpt_measure_read_pattern): the same grid-stride read with BPL bytes per
// lane in the display kernel's access shapes: 4 (one float per lane: depth), 12 (three
// consecutive floats per lane at a 12-B stride: the first-hit normals), 16 (one float4: the
// accumulator).  One kernel per shape, so a rocprofv3 --pmc FETCH_SIZE pass reports each alone.
template <int BPL>
__global__ void __launch_bounds__(256) k_read_pattern(const float* __restrict__ p, size_t n_lanes, float* out) {
    float acc = 0.f;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lanes; i += stride) {
        if (BPL == 4) {
            acc += p[i];
        } else if (BPL == 12) {
            acc += (p[3 * i] + p[3 * i + 1]) + p[3 * i + 2];
        } else {
            const float4 v = reinterpret_cast<const float4*>(p)[i];
            acc += (v.x + v.y) + (v.z + v.w);
        }
    }
    if (acc == 1.2345e-30f) out[0] = acc;
}

hipError_t launch_read_pattern(int bpl, const float* p, size_t n_lanes, float* out, int grid, hipStream_t stream) {
    if (bpl == 4) hipLaunchKernelGGL(k_read_pattern<4>, dim3(grid), dim3(256), 0, stream, p, n_lanes, out);
    else if (bpl == 12) hipLaunchKernelGGL(k_read_pattern<12>, dim3(grid), dim3(256), 0, stream, p, n_lanes, out);
    else hipLaunchKernelGGL(k_read_pattern<16>, dim3(grid), dim3(256), 0, stream, p, n_lanes, out);
    return hipGetLastError();
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

hipError_t launch_selftest_qdiv(int which, uint64_t n, uint64_t seed, unsigned long long* out, int out_len,
                                hipStream_t stream) {
    if (which >= 8)
        hipLaunchKernelGGL(k_selftest_fm, dim3(8192), dim3(256), 0, stream, which, n, seed, out, out_len);
    else if (which >= 6)
        hipLaunchKernelGGL(k_selftest_dn_weight, dim3(8192), dim3(256), 0, stream, which, n, out, out_len);
    else
        hipLaunchKernelGGL(k_selftest_qdiv, dim3(4096), dim3(256), 0, stream, which, n, seed, out, out_len);
    return hipGetLastError();
}

}  // namespace cpt
