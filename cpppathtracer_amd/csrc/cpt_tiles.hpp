// cpt_tiles.hpp — the 8x8 tile grid of a frame's rows, the contract between the kernels that walk
// the frame in tiles (k_megakernel, k_tile_draws, k_tile_noise, k_compact_order, k_wf_ident) and
// their host launchers, and the two wave64 helpers those kernels share.  Host and device code.
//
// Tiles are numbered row-major over the frame's rows (the context's rows, not the image's); a tile
// is one wave: pixel k of a tile is column k & 7, row k >> 3 of it.  Tiles at the right and bottom
// edges may lie partly outside the frame.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cpt {

struct TileGrid {
    int width, n_rows;
    __host__ __device__ constexpr int tiles_x() const { return (width + 7) >> 3; }
    __host__ __device__ constexpr int tiles_y() const { return (n_rows + 7) >> 3; }
    __host__ __device__ constexpr int count() const { return tiles_x() * tiles_y(); }
    // Pixel k (0..63) of `tile`: its column x and its row index ri; whether it is in the frame.
    __host__ __device__ constexpr bool pixel(uint32_t tile, uint32_t k, int& x, int& ri) const {
        x = (int)(tile % tiles_x()) * 8 + (int)(k & 7);
        ri = (int)(tile / tiles_x()) * 8 + (int)(k >> 3);
        return x < width && ri < n_rows;
    }
    // The pixels of `tile` that are in the frame.
    __host__ __device__ constexpr int pixels_in(uint32_t tile) const {
        const int w = width - (int)(tile % tiles_x()) * 8, h = n_rows - (int)(tile / tiles_x()) * 8;
        return (w < 8 ? w : 8) * (h < 8 ? h : 8);
    }
};

namespace tiles_check {
constexpr bool pixel_is(TileGrid g, uint32_t tile, uint32_t k, int want_x, int want_ri) {
    int x = -1, ri = -1;
    return g.pixel(tile, k, x, ri) && x == want_x && ri == want_ri;
}
constexpr bool pixel_outside(TileGrid g, uint32_t tile, uint32_t k) {
    int x = -1, ri = -1;
    return !g.pixel(tile, k, x, ri);
}
constexpr TileGrid EXACT{16, 8}, PARTIAL{17, 9};
static_assert(EXACT.tiles_x() == 2 && EXACT.tiles_y() == 1 && EXACT.count() == 2, "16 x 8: two whole tiles");
static_assert(EXACT.pixels_in(0) == 64 && EXACT.pixels_in(1) == 64 && pixel_is(EXACT, 1, 63, 15, 7), "16 x 8");
static_assert(PARTIAL.tiles_x() == 3 && PARTIAL.tiles_y() == 2 && PARTIAL.count() == 6, "17 x 9: 3 x 2 tiles");
static_assert(PARTIAL.pixels_in(0) == 64 && PARTIAL.pixels_in(2) == 1 * 8 && PARTIAL.pixels_in(3) == 8 * 1 &&
                  PARTIAL.pixels_in(5) == 1 * 1,
              "17 x 9: the edge tiles");
static_assert(pixel_is(PARTIAL, 0, 9, 1, 1) && pixel_is(PARTIAL, 2, 8, 16, 1) && pixel_outside(PARTIAL, 2, 1), "17 x 9: tile 2");
static_assert(pixel_is(PARTIAL, 5, 0, 16, 8) && pixel_outside(PARTIAL, 5, 1) && pixel_outside(PARTIAL, 5, 8), "17 x 9: tile 5");
}  // namespace tiles_check

#if defined(__HIPCC__)
// The set lanes of `mask` below this one: a lane's rank among the lanes of a ballot.
__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// Number of set bits of a wave-uniform mask as a 32-bit value (two 32-bit popcounts: the
// compiler then compares it with SALU s_cmp_*_u32; a 64-bit popcount it compares with VALU
// v_cmp_*_u64).  (Not inline asm: s_bcnt1 writes SCC, which an asm statement cannot declare.)
__device__ __forceinline__ uint32_t wave_count(uint64_t m) {
    return (uint32_t)__builtin_popcount((uint32_t)m) + (uint32_t)__builtin_popcount((uint32_t)(m >> 32));
}
#endif

}  // namespace cpt
