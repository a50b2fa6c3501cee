// cpt_topup.hpp — the top-up render's deficit rule, shared by the device
// (cpt_topup.hip k_tile_deficit, cpt_megakernel.hip's TOPUP take) and the host
// (cpt_topup_deficit_host), and the plan's launcher.
//
// The reference has no counterpart: it gives every pixel the same number of passes
// (path_tracer.cu:124-175).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cpt {
namespace topup {

constexpr int MAX_TARGET = 1 << 20;

// The passes a pixel whose accumulator holds `count` passes (its .w) still needs to reach
// `target` (1..MAX_TARGET): target - (int)count for a finite count in [0, target), truncated as
// the cast does; 0 for every other count (at or past the target, negative, NaN, +-inf).  A
// fractional count (a reprojected pixel of partial weight) is topped up to just past the target.
__host__ __device__ inline int deficit(float count, int target) {
    // (count >= 0 && count < target is false for a NaN; an infinity fails one side; target is
    // exact as a float, and a count below it fits an int)
    return (count >= 0.0f && count < (float)target) ? target - (int)count : 0;
}

// The words of a plan's device record (TopupPlan::words).
enum : int {
    PLAN_ACTIVE = 0,   // u32: tiles with a deficit (the megakernel's top-up launches read it)
    PLAN_PIXELS = 2,   // u64 (words 2, 3): pixels with a deficit
    PLAN_PASSES = 4,   // u64 (words 4, 5): the sum of the deficits
    PLAN_WORDS = 6,
};

}  // namespace topup

// The plan of a top-up launch: k_tile_deficit keys every 8x8 tile of the frame by its largest
// deficit and counts the record's three totals; the tiles are then sorted by key, descending and
// stable, into `order` (cpt_schedule.hip's radix sort), so the tiles with a deficit are its first
// words[PLAN_ACTIVE] entries.  `scratch` holds tile_schedule_scratch_bytes() bytes.
struct TopupPlan {
    const float4* accum;   // [n_rows*width]
    int width, n_rows, target;
    uint32_t* order;       // [tiles]
    uint32_t* words;       // [topup::PLAN_WORDS], 8-byte aligned
};
hipError_t launch_topup_plan(const TopupPlan& t, void* scratch, size_t scratch_bytes, hipStream_t stream);
// cpt_schedule.hip: order := the tile ids 0..n-1 by descending key (stable), the keys being the
// first n words of `scratch`.
hipError_t sort_tiles_by_key(void* scratch, size_t scratch_bytes, int n, uint32_t* order, hipStream_t stream);

}  // namespace cpt
