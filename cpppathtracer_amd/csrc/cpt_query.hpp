// cpt_query.hpp — the ray-query kernel's arguments and launcher (cpt_query.hip), shared with the
// C-ABI's query entry points (cpt_capi_query.cpp): cpt_gbuffer, cpt_trace_rays, cpt_pick.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_internal.hpp"

namespace cpt {

// Explicit rays (device arrays): origin3 / dir3 [n][3], tmin [n] (nullptr: 0 for every ray).
struct QueryRays {
    const float* origin3;
    const float* dir3;
    const float* tmin;
    uint32_t n;
};

// Camera rays: the frame's pixels (pick_x < 0: pixel i = (i % width, rows[i / width]) writes slot
// i), or the one pixel (pick_x, pick_y) of the image, which writes slot 0.
struct QueryPixels {
    int pick_x, pick_y;
};

// Per ray or pixel: the object index in AddObject order (-1: miss), the hit distance
// (DEFAULT_RAY_TMAX on a miss), the normal (-dir on a miss) and, for camera rays, the material's
// GetKd(0, 0) (0 on a miss).  albedo3 may be nullptr.
struct QueryOut {
    int32_t* id;
    float* t;
    float* normal3;
    float* albedo3;
};

// One ray per lane through the walk p.ordered selects (cpt_path.hpp trace_segment).  Only the scene
// part of `p`, its camera and its rows are read; rank_obj maps a leaf's reference-order position
// to its object index.  rays == nullptr: camera rays as `pixels` says.
hipError_t launch_ray_query(const KParams& p, const int32_t* rank_obj, const QueryRays* rays, QueryPixels pixels,
                            const QueryOut& out, hipStream_t stream);

}  // namespace cpt
