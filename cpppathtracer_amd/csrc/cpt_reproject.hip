// cpt_reproject.hip — the kernels of cpt_reproject_accum, cpt_reproject_display
// (§22) and their tracked variants (§23): the accumulated frame looked up at a moved camera.  The
// arithmetic is cpt_reproject.hpp's, shared with the host entry; this file only decides where a
// tap's operands come from.
//
//   k_reproject_accum   a plain grid, one new pixel per lane, wave w = 8x8 tile w of the frame
//                       (cpt_tiles.hpp, as k_ray_query's camera rays): a wave's four-tap footprints
//                       then fall in one compact window of the old frame.  A tap's accumulator
//                       pixel is one 16-byte load, its id and distance 4-byte gathers, its ray
//                       direction ray_gen_centre of the old camera; the output is one 16-byte
//                       store per lane, to a second plane (taps read neighbours).  No LDS.
//
//   k_reproject_display the same shape for cpt_reproject_display: the display
//                       state, the Mix mean and the per-pixel sample count, looked up at the moved
//                       camera.  A tap is three 4-byte mean loads and the count, id and distance
//                       gathers; the output is three 4-byte mean stores and the count, to second
//                       planes.  Every pixel of the frame is written (zeros outside the display's
//                       launch region).  No LDS.
//
//   k_reproject_accum_tracked, k_reproject_display_tracked
//                       the same two for the tracked calls: each lane that hit an
//                       object gathers that object's 40-byte motion record and looks up the point
//                       the object held at the capture; the lane's id and distance also go to the
//                       planes that become the next call's history.  No LDS.
//
// The reference has no counterpart (MotionalCamera::Refresh restarts the running mean).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_path.hpp"
#include "cpt_reproject.hpp"
#include "cpt_tiles.hpp"

namespace cpt {

namespace {

namespace rp = reproject;

__device__ __forceinline__ rp::V3 as_v3(const v3 a) { return rp::V3{a.x, a.y, a.z}; }

// The old frame in device memory; a tap's direction is the old camera's centre ray of its pixel.
struct DeviceSrc {
    const float4* in;
    const int32_t* id;
    const float* t;
    const CamK* cam0;
    __device__ rp::Px accum(size_t k) const {
        const float4 a = in[k];
        return rp::Px{a.x, a.y, a.z, a.w};
    }
    __device__ int32_t id0(size_t k) const { return id[k]; }
    __device__ float t0(size_t k) const { return t[k]; }
    __device__ rp::V3 dir0(int x, int y, size_t) const { return as_v3(ray_gen_centre(*cam0, x, y).d); }
};

// The old frame's display state in device memory.
struct DeviceDisplaySrc {
    const float* mean;
    const float* count;
    const int32_t* id;
    const float* t;
    const CamK* cam0;
    __device__ rp::Px shown(size_t k) const { return rp::Px{mean[3 * k], mean[3 * k + 1], mean[3 * k + 2], count[k]}; }
    __device__ int32_t id0(size_t k) const { return id[k]; }
    __device__ float t0(size_t k) const { return t[k]; }
    __device__ rp::V3 dir0(int x, int y, size_t) const { return as_v3(ray_gen_centre(*cam0, x, y).d); }
};

}  // namespace

__global__ void __launch_bounds__(256) k_reproject_accum(const ReprojectArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const TileGrid grid{a.width, a.height};
    int x = 0, y = 0;
    if ((i >> 6) >= (uint32_t)grid.count() || !grid.pixel(i >> 6, i & 63, x, y)) return;
    const size_t pix = (size_t)y * a.width + x;
    const DeviceSrc src{a.in, a.id0, a.t0, &a.cam0};
    const rp::V3 n1{a.normal1[3 * pix], a.normal1[3 * pix + 1], a.normal1[3 * pix + 2]};
    const rp::V3 o1{a.cam1.origin[0], a.cam1.origin[1], a.cam1.origin[2]};
    const rp::Px r = rp::pixel(src, a.view0, o1, a.width, a.height, a.id1[pix], a.t1[pix], n1,
                               as_v3(ray_gen_centre(a.cam1, x, y).d), a.max_history, a.plane_tol);
    a.out[pix] = make_float4(r.r, r.g, r.b, r.n);
}

__global__ void __launch_bounds__(256) k_reproject_display(const ReprojectDisplayArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const TileGrid grid{a.width, a.height};
    int x = 0, y = 0;
    if ((i >> 6) >= (uint32_t)grid.count() || !grid.pixel(i >> 6, i & 63, x, y)) return;
    const size_t pix = (size_t)y * a.width + x;
    const DeviceDisplaySrc src{a.mean_in, a.count_in, a.id0, a.t0, &a.cam0};
    const rp::V3 n1{a.normal1[3 * pix], a.normal1[3 * pix + 1], a.normal1[3 * pix + 2]};
    const rp::V3 o1{a.cam1.origin[0], a.cam1.origin[1], a.cam1.origin[2]};
    const rp::Px r = rp::display_pixel(src, a.view0, o1, a.width, a.height, a.w_eff, a.h_eff, x, y, a.id1[pix], a.t1[pix], n1,
                                       as_v3(ray_gen_centre(a.cam1, x, y).d), a.max_history, a.plane_tol);
    a.mean_out[3 * pix] = r.r;
    a.mean_out[3 * pix + 1] = r.g;
    a.mean_out[3 * pix + 2] = r.b;
    a.count_out[pix] = r.n;
}

// The tracked pair: the same lanes, taps and stores; each lane that hit an object
// first gathers that object's motion record (40 bytes, mostly one record per wave, the table in
// L2) and looks up the point the object held at the capture.  The lane also writes its id and
// distance to the planes that become the next call's history.
__global__ void __launch_bounds__(256) k_reproject_accum_tracked(const ReprojectTrackedArgs ta) {
    const ReprojectArgs& a = ta.look;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const TileGrid grid{a.width, a.height};
    int x = 0, y = 0;
    if ((i >> 6) >= (uint32_t)grid.count() || !grid.pixel(i >> 6, i & 63, x, y)) return;
    const size_t pix = (size_t)y * a.width + x;
    const DeviceSrc src{a.in, a.id0, a.t0, &a.cam0};
    const rp::V3 n1{a.normal1[3 * pix], a.normal1[3 * pix + 1], a.normal1[3 * pix + 2]};
    const rp::V3 o1{a.cam1.origin[0], a.cam1.origin[1], a.cam1.origin[2]};
    const int32_t id1 = a.id1[pix];
    const float t1 = a.t1[pix];
    const rp::Px r = rp::pixel<false, DeviceSrc, rp::TableMotion>(src, a.view0, o1, a.width, a.height, id1, t1, n1,
                                                                  as_v3(ray_gen_centre(a.cam1, x, y).d), a.max_history,
                                                                  a.plane_tol, 0, 0, rp::TableMotion{ta.motion});
    a.out[pix] = make_float4(r.r, r.g, r.b, r.n);
    ta.id_next[pix] = id1;
    ta.t_next[pix] = t1;
}

__global__ void __launch_bounds__(256) k_reproject_display_tracked(const ReprojectDisplayTrackedArgs ta) {
    const ReprojectDisplayArgs& a = ta.look;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const TileGrid grid{a.width, a.height};
    int x = 0, y = 0;
    if ((i >> 6) >= (uint32_t)grid.count() || !grid.pixel(i >> 6, i & 63, x, y)) return;
    const size_t pix = (size_t)y * a.width + x;
    const DeviceDisplaySrc src{a.mean_in, a.count_in, a.id0, a.t0, &a.cam0};
    const rp::V3 n1{a.normal1[3 * pix], a.normal1[3 * pix + 1], a.normal1[3 * pix + 2]};
    const rp::V3 o1{a.cam1.origin[0], a.cam1.origin[1], a.cam1.origin[2]};
    const int32_t id1 = a.id1[pix];
    const float t1 = a.t1[pix];
    const rp::Px r = rp::display_pixel(src, a.view0, o1, a.width, a.height, a.w_eff, a.h_eff, x, y, id1, t1, n1,
                                       as_v3(ray_gen_centre(a.cam1, x, y).d), a.max_history, a.plane_tol,
                                       rp::TableMotion{ta.motion});
    a.mean_out[3 * pix] = r.r;
    a.mean_out[3 * pix + 1] = r.g;
    a.mean_out[3 * pix + 2] = r.b;
    a.count_out[pix] = r.n;
    ta.id_next[pix] = id1;
    ta.t_next[pix] = t1;
}

hipError_t launch_reproject_tracked(const ReprojectTrackedArgs& a, hipStream_t stream) {
    const size_t lanes = (size_t)TileGrid{a.look.width, a.look.height}.count() * 64;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reproject_accum_tracked, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_reproject_display_tracked(const ReprojectDisplayTrackedArgs& a, hipStream_t stream) {
    const size_t lanes = (size_t)TileGrid{a.look.width, a.look.height}.count() * 64;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reproject_display_tracked, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_reproject_display(const ReprojectDisplayArgs& a, hipStream_t stream) {
    const size_t lanes = (size_t)TileGrid{a.width, a.height}.count() * 64;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reproject_display, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_reproject(const ReprojectArgs& a, hipStream_t stream) {
    const size_t lanes = (size_t)TileGrid{a.width, a.height}.count() * 64;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reproject_accum, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace cpt
