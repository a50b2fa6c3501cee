// cpt_schedule.hip — the cost schedule's tile orders (DESIGN.md §Cost schedule).
//
//   k_iota, k_tile_draws             tile ids; each 8x8 tile's RNG draws since the last call
//   tile_schedule_scratch_bytes      what launch_tile_* need as scratch
//   launch_tile_schedule             pilot (cpt_megakernel.hip launch_cost_pilot) + sort
//   launch_tile_order_from_draws     CPT_SCHEDULE_PREVIOUS: draws + sort
//   sort_tiles_by_key                the top-up plan's order (cpt_topup.hip): the sort alone
//
// The only unit that includes hipcub (its radix sort's rocprim kernels).  The reference has no
// counterpart: it launches one thread per pixel in raster order (path_tracer.cu:124-133).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>

#include "cpt_path.hpp"
#include "cpt_topup.hpp"

namespace cpt {

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
    const int n = TileGrid{width, n_rows}.count();
    size_t temp = 0;
    (void)hipcub::DeviceRadixSort::SortPairsDescending(nullptr, temp, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, n);
    return 3 * (size_t)n * sizeof(uint32_t) + temp + 256;
}

// CPT_SCHEDULE_PREVIOUS: one wave per 8x8 tile; lane k = pixel k of the tile (TileGrid::pixel).
//  A pixel's draws since the last call are (d - d_prev) / 362437 mod 2^32 (every
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
    const uint32_t tile = blockIdx.x;
    const int k = threadIdx.x;
    int x, ri;
    uint32_t draws = 0;
    if (TileGrid{width, n_rows}.pixel(tile, k, x, ri)) {
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

// The scratch of both tile orders: cost / cost_sorted / ids (n words each), then hipcub's temp.
struct TileScratch {
    uint32_t *cost, *cost_sorted, *ids;
    void* temp;
    size_t temp_bytes;
};
static TileScratch carve_tile_scratch(void* scratch, size_t scratch_bytes, int n) {
    TileScratch s;
    s.cost = (uint32_t*)scratch;
    s.cost_sorted = s.cost + n;
    s.ids = s.cost_sorted + n;
    s.temp = (void*)(((uintptr_t)(s.ids + n) + 255) & ~(uintptr_t)255);
    s.temp_bytes = scratch_bytes - ((char*)s.temp - (char*)scratch);
    return s;
}
// order := the tile ids by descending s.cost.
static hipError_t sort_tiles_by_cost(const TileScratch& s, int n, uint32_t* order, hipStream_t stream) {
    hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, stream, s.ids, (uint32_t)n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t temp_bytes = s.temp_bytes;
    return hipcub::DeviceRadixSort::SortPairsDescending(s.temp, temp_bytes, s.cost, s.cost_sorted, s.ids, order, n, 0, 32,
                                                        stream);
}

hipError_t launch_tile_order_from_draws(const KParams& p, uint32_t* d_prev, void* scratch, size_t scratch_bytes,
                                        uint32_t* order, hipStream_t stream) {
    const int n = TileGrid{p.width, p.n_rows}.count();
    if (n <= 0) return hipSuccess;
    const TileScratch s = carve_tile_scratch(scratch, scratch_bytes, n);
    const size_t npix = (size_t)p.n_rows * p.width;
    hipLaunchKernelGGL(k_tile_draws, dim3((unsigned)n), dim3(64), 0, stream, p.rng + 5 * npix, d_prev, p.width,
                       p.n_rows, s.cost);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return sort_tiles_by_cost(s, n, order, stream);
}

hipError_t launch_tile_schedule(const KParams& p0, int passes, void* scratch, size_t scratch_bytes, uint32_t* order,
                                LaunchGrid& grid, hipStream_t stream) {
    const int n = TileGrid{p0.width, p0.n_rows}.count();
    if (n <= 0) return hipSuccess;
    const TileScratch s = carve_tile_scratch(scratch, scratch_bytes, n);
    hipError_t e = hipMemsetAsync(s.cost, 0, (size_t)n * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(p0.work, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    KParams p = p0;
    p.spp = passes;
    p.tile_cost = s.cost;
    p.tile_order = nullptr;
    p.n_active = 0;
    p.accumulate = 0;
    e = launch_cost_pilot(p, grid, stream);
    if (e != hipSuccess) return e;
    return sort_tiles_by_cost(s, n, order, stream);
}

// The top-up plan's order (cpt_topup.hip): the same sort on keys the caller left in the scratch's
// first n words.  The radix sort is stable and the ids ascend, so equal keys stay row-major.
hipError_t sort_tiles_by_key(void* scratch, size_t scratch_bytes, int n, uint32_t* order, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    return sort_tiles_by_cost(carve_tile_scratch(scratch, scratch_bytes, n), n, order, stream);
}
}  // namespace cpt
