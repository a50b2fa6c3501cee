// cpt_reproject.hip — the kernels of cpt_reproject_accum, cpt_reproject_display
// (§22) and their tracked variants (§23): the accumulated frame looked up at a moved camera.  The
// arithmetic is cpt_reproject.hpp's, shared with the host entry; this file only decides where a
// tap's operands come from.
//
//   k_reproject<Args>   one body for the four argument structs of cpt_reproject.hpp.  A plain grid,
//                       one new pixel per lane, wave w = 8x8 tile w of the frame (cpt_tiles.hpp, as
//                       k_ray_query's camera rays): a wave's four-tap footprints then fall in one
//                       compact window of the old frame.  A tap's id and distance are 4-byte
//                       gathers, its ray direction ray_gen_centre of the old camera.  No LDS.
//     ReprojectArgs         (§21) a tap's accumulator pixel is one 16-byte load; the output is one
//                           16-byte store per lane, to a second plane (taps read neighbours).
//     ReprojectDisplayArgs  (§22) the display state, the Mix mean and the per-pixel sample count:
//                           a tap is three 4-byte mean loads and the count; the output is three
//                           4-byte mean stores and the count, to second planes.  Every pixel of the
//                           frame is written (zeros outside the display's launch region).
//     ReprojectTracked<..>  (§23) either of the two: each lane that hit an object first gathers
//                           that object's motion record (40 bytes, mostly one record per wave, the
//                           table in L2) and looks up the point the object held at the capture; the
//                           lane's id and distance also go to the planes that become the next
//                           call's history.
//
// The reference has no counterpart (MotionalCamera::Refresh restarts the running mean).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

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

__device__ __forceinline__ rp::NoMotion motion_of(const ReprojectArgs&) { return {}; }
__device__ __forceinline__ rp::NoMotion motion_of(const ReprojectDisplayArgs&) { return {}; }
template <typename Look>
__device__ __forceinline__ rp::TableMotion motion_of(const ReprojectTracked<Look>& args) { return rp::TableMotion{args.motion}; }

}  // namespace

// The look-up and its stores are written out in the body, not behind functions taking the argument
// struct: with those the compiler commuted a few multiplies and rescheduled the display's address
// arithmetic, and the four streams would no longer be the ones of the four kernels this replaced.
template <typename Args>
__global__ void __launch_bounds__(256) k_reproject(const Args args) {
    const auto& a = look_of(args);
    constexpr bool DISPLAY = std::is_same_v<std::decay_t<decltype(a)>, ReprojectDisplayArgs>;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const TileGrid grid{a.width, a.height};
    int x = 0, y = 0;
    if ((i >> 6) >= (uint32_t)grid.count() || !grid.pixel(i >> 6, i & 63, x, y)) return;
    const size_t pix = (size_t)y * a.width + x;
    const rp::V3 n1{a.normal1[3 * pix], a.normal1[3 * pix + 1], a.normal1[3 * pix + 2]};
    const rp::V3 o1{a.cam1.origin[0], a.cam1.origin[1], a.cam1.origin[2]};
    const int32_t id1 = a.id1[pix];
    const float t1 = a.t1[pix];
    const rp::V3 d1 = as_v3(ray_gen_centre(a.cam1, x, y).d);
    const auto motion = motion_of(args);
    if constexpr (DISPLAY) {
        const DeviceDisplaySrc src{a.mean_in, a.count_in, a.id0, a.t0, &a.cam0};
        const rp::Px r = rp::display_pixel(src, a.view0, o1, a.width, a.height, a.w_eff, a.h_eff, x, y, id1, t1, n1, d1,
                                           a.max_history, a.plane_tol, motion);
        a.mean_out[3 * pix] = r.r;
        a.mean_out[3 * pix + 1] = r.g;
        a.mean_out[3 * pix + 2] = r.b;
        a.count_out[pix] = r.n;
    } else {
        const DeviceSrc src{a.in, a.id0, a.t0, &a.cam0};
        const rp::Px r = rp::pixel<false>(src, a.view0, o1, a.width, a.height, id1, t1, n1, d1, a.max_history, a.plane_tol, 0,
                                          0, motion);
        a.out[pix] = make_float4(r.r, r.g, r.b, r.n);
    }
    if constexpr (is_tracked<Args>) {   // the next call's history
        args.id_next[pix] = id1;
        args.t_next[pix] = t1;
    }
}

template <typename Args>
hipError_t launch_reproject(const Args& args, hipStream_t stream) {
    const size_t lanes = (size_t)TileGrid{look_of(args).width, look_of(args).height}.count() * 64;
    if (lanes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_reproject<Args>, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, args);
    return hipGetLastError();
}
template hipError_t launch_reproject(const ReprojectArgs&, hipStream_t);
template hipError_t launch_reproject(const ReprojectDisplayArgs&, hipStream_t);
template hipError_t launch_reproject(const ReprojectTracked<ReprojectArgs>&, hipStream_t);
template hipError_t launch_reproject(const ReprojectTracked<ReprojectDisplayArgs>&, hipStream_t);

}  // namespace cpt

