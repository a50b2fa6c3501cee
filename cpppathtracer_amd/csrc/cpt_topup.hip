// cpt_topup.hip — the plan of a top-up render (cpt_render_to_count).
//
//   k_tile_deficit      each 8x8 tile's key (its largest per-pixel deficit) and the plan's totals
//   launch_topup_plan   the keys, then the tiles sorted by key (cpt_schedule.hip's radix sort)
//
// The megakernel's TOPUP instantiations (cpt_megakernel.hip) dequeue the sorted order's active
// prefix, whose length they read from the plan's device record.  The reference has no counterpart:
// every pixel runs the same passes (path_tracer.cu:124-175).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_tiles.hpp"
#include "cpt_topup.hpp"

namespace cpt {

// One wave64 per tile; lane k = pixel k of the tile (TileGrid::pixel).  Lanes outside the frame
// (partial tiles) have no deficit.  A tile without a deficit writes its zero key and nothing else.
__global__ void __launch_bounds__(64) k_tile_deficit(const float4* __restrict__ accum, int width, int n_rows, int target,
                                                     uint32_t* __restrict__ key, uint32_t* __restrict__ words) {
    const uint32_t tile = blockIdx.x;   // < the grid's tiles: the launch's size
    const int k = threadIdx.x;
    int x, ri;
    uint32_t d = 0;
    if (TileGrid{width, n_rows}.pixel(tile, k, x, ri)) d = (uint32_t)topup::deficit(accum[(size_t)ri * width + x].w, target);
    const uint32_t pixels = wave_count(__ballot(d != 0u));
    uint32_t most = d, sum = d;   // the sum of 64 deficits of at most 2^20 fits 32 bits
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(most, off, 64);
        most = o > most ? o : most;
        sum += __shfl_xor(sum, off, 64);
    }
    if (k != 0) return;
    key[tile] = most;
    if (most == 0u) return;
    atomicAdd(&words[topup::PLAN_ACTIVE], 1u);
    atomicAdd(reinterpret_cast<unsigned long long*>(words + topup::PLAN_PIXELS), (unsigned long long)pixels);
    atomicAdd(reinterpret_cast<unsigned long long*>(words + topup::PLAN_PASSES), (unsigned long long)sum);
}

hipError_t launch_topup_plan(const TopupPlan& t, void* scratch, size_t scratch_bytes, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(t.words, 0, topup::PLAN_WORDS * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const int n = TileGrid{t.width, t.n_rows}.count();
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_tile_deficit, dim3((unsigned)n), dim3(64), 0, stream, t.accum, t.width, t.n_rows, t.target,
                       (uint32_t*)scratch, t.words);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return sort_tiles_by_key(scratch, scratch_bytes, n, t.order, stream);
}

}  // namespace cpt
