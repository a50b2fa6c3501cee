// cpt_adaptive.hip — the kernels around the megakernel in an adaptive render (cpt_render_adaptive,
// DESIGN.md §Adaptive sampling).
//
//   k_tile_noise      after a round: each active tile's pixels get the round's batch mean into
//                     their moments, the noise map and the snapshot; one keep flag per list position
//   k_compact_order   the tiles kept, in the order they had (stable), and how many
//
// The reference has no counterpart: every pixel runs the same passes (path_tracer.cu:124-175).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_adaptive.hpp"
#include "cpt_internal.hpp"
#include "cpt_tiles.hpp"

namespace cpt {

// One wave64 per position of the active list; lane k = pixel k of the tile
// (TileGrid::pixel).  Lanes outside the frame (partial tiles) do nothing and count as
// converged.  The tile's flag is a ballot: no LDS.
__global__ void __launch_bounds__(64) k_tile_noise(const AdaptiveRound a) {
    const uint32_t i = blockIdx.x;   // < a.n_active: the grid's size
    const uint32_t tile = a.order ? a.order[i] : i;
    const int k = threadIdx.x;
    int x, ri;
    bool open = false;
    if (TileGrid{a.width, a.n_rows}.pixel(tile, k, x, ri)) {
        const size_t npix = (size_t)a.n_rows * a.width;
        const size_t pix = (size_t)ri * a.width + x;
        const float4 S = a.accum[pix], P = a.snap[pix];
        float m1 = a.stat[pix], m2 = a.stat[npix + pix], kk = a.stat[2 * npix + pix];
        adaptive::add_batch(m1, m2, kk, adaptive::batch_luma(S.x, S.y, S.z, S.w, P.x, P.y, P.z, P.w));
        float rel;
        open = !adaptive::decide(m1, m2, kk, a.rel_error, rel);
        a.stat[pix] = m1;
        a.stat[npix + pix] = m2;
        a.stat[2 * npix + pix] = kk;
        a.stat[3 * npix + pix] = rel;
        a.snap[pix] = S;
    }
    const uint64_t any_open = __ballot(open);
    if (k == 0) a.keep[i] = (a.last || (a.eligible && any_open == 0)) ? 0u : 1u;
}

// dst := the src[i] (i itself without a src) with keep[i] set, in the order of i; out[0] = how
// many, out[1] = the frame pixels of all n tiles of the input list (what the round rendered).
// One workgroup of 1024 lanes walks the list in chunks of 1024: a ballot and mbcnt place a
// tile within its wave, the 16 waves' counts (LDS) within the chunk, a running offset the chunk.
// At most 129 600 tiles (3840 x 2160): 127 chunks.
constexpr int COMPACT_BLOCK = 1024;
__global__ void __launch_bounds__(COMPACT_BLOCK) k_compact_order(const uint32_t* __restrict__ src,
                                                                 const uint32_t* __restrict__ keep, uint32_t n, int width,
                                                                 int n_rows, uint32_t* __restrict__ dst,
                                                                 uint32_t* __restrict__ out) {
    constexpr int WAVES = COMPACT_BLOCK / 64;
    __shared__ uint32_t s_cnt[WAVES], s_px[WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const TileGrid grid{width, n_rows};
    uint32_t base = 0;   // uniform: tiles kept before this chunk
    uint32_t px = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += COMPACT_BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        bool kept = false;
        uint32_t tile = 0;
        if (i < n) {
            tile = src ? src[i] : i;
            kept = keep[i] != 0u;
            px += (uint32_t)grid.pixels_in(tile);
        }
        const uint64_t m = __ballot(kept);
        if (lane == 0) s_cnt[wave] = wave_count(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const uint32_t c = s_cnt[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        if (kept) dst[base + before + lane_rank(m)] = tile;   // < n: at most i tiles were kept before i
        base += total;
        __syncthreads();   // s_cnt is rewritten by the next chunk
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) px += __shfl_xor(px, off, 64);
    if (lane == 0) s_px[wave] = px;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < WAVES; ++w) sum += s_px[w];
        out[0] = base;
        out[1] = sum;
    }
}

hipError_t launch_tile_noise(const AdaptiveRound& a, hipStream_t stream) {
    if (a.n_active == 0) return hipSuccess;
    hipLaunchKernelGGL(k_tile_noise, dim3(a.n_active), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_compact_order(const uint32_t* src, const uint32_t* keep, uint32_t n, int width, int n_rows,
                                uint32_t* dst, uint32_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_compact_order, dim3(1), dim3(COMPACT_BLOCK), 0, stream, src, keep, n, width, n_rows, dst, out);
    return hipGetLastError();
}

}  // namespace cpt
