// cpt_filter.hip — the kernels of cpt_filter_frame: the variance-guided a-trous
// filter of an adaptive render's final frame.  The arithmetic is cpt_filter.hpp's, shared with the
// host hooks; this file only decides where a tap's operands come from.
//
//   k_filter_prepare   level 0: each pixel's mean, variance of the mean and validity from the
//                      accumulator and the adaptive render's moments
//   k_filter_level     one level: a 256-lane workgroup owns a 64 x 4 pixel block, each wave one
//                      64-pixel row segment (a float4 load or store of a wave is 1 KB, coalesced).
//                      LDS_STEP > 0 (steps 1 and 2): the block's pixels, normals and validity are
//                      staged in LDS with their 2 * step halo and every tap reads the tile;
//                      LDS_STEP == 0: the taps read global memory (L2 serves the strided ones)
//
// The reference has no counterpart (its only filter is Denoising + Mix, path_tracer.cu:177-254).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_filter.hpp"
#include "cpt_internal.hpp"
#include "cpt_tuning.hpp"

namespace cpt {

namespace {

constexpr int BLOCK_W = 64, BLOCK_H = 4;

__device__ __forceinline__ filter::Px as_px(const float4 v) { return filter::Px{v.x, v.y, v.z, v.w}; }
__device__ __forceinline__ float4 as_f4(const filter::Px& p) { return make_float4(p.r, p.g, p.b, p.v); }

struct GlobalSrc {
    const float4* in;
    const float* normal3;
    const uint8_t* ok;
    int width;
    __device__ bool valid(int x, int y) const { return ok[(size_t)y * width + x] != 0; }
    __device__ filter::Px px(int x, int y) const { return as_px(in[(size_t)y * width + x]); }
    __device__ void normal(int x, int y, float n[3]) const {
        const float* p = normal3 + 3 * ((size_t)y * width + x);
        n[0] = p[0];
        n[1] = p[1];
        n[2] = p[2];
    }
};

// The tile of a block: TW x TH entries from (x0, y0) = the block's corner less the halo; entries
// outside the frame are invalid.  nv = (normal, validity as 1 or 0).
template <int TW>
struct TileSrc {
    const float4* cv;
    const float4* nv;
    int x0, y0;
    __device__ int at(int x, int y) const { return (y - y0) * TW + (x - x0); }
    __device__ bool valid(int x, int y) const { return nv[at(x, y)].w != 0.0f; }
    __device__ filter::Px px(int x, int y) const { return as_px(cv[at(x, y)]); }
    __device__ void normal(int x, int y, float n[3]) const {
        const float4 v = nv[at(x, y)];
        n[0] = v.x;
        n[1] = v.y;
        n[2] = v.z;
    }
};

}  // namespace

__global__ void __launch_bounds__(256) k_filter_prepare(const float4* __restrict__ accum, const float* __restrict__ stat,
                                                        size_t npix, float4* __restrict__ plane, uint8_t* __restrict__ ok) {
    const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= npix) return;
    const float4 S = accum[pix];
    filter::Px c;
    const bool valid = filter::prepare(S.x, S.y, S.z, S.w, stat[pix], stat[npix + pix], stat[2 * npix + pix], c);
    plane[pix] = as_f4(c);
    ok[pix] = valid ? 1 : 0;
}

template <int LDS_STEP>
__global__ void __launch_bounds__(BLOCK_W* BLOCK_H) k_filter_level(const float4* __restrict__ in, const float* __restrict__ normal3,
                                                                  const uint8_t* __restrict__ ok, float4* __restrict__ out,
                                                                  int width, int height, int step, float sig2, int sharpness_log2) {
    const int bx = blockIdx.x * BLOCK_W, by = blockIdx.y * BLOCK_H;
    const int x = bx + (int)(threadIdx.x & 63), y = by + (int)(threadIdx.x >> 6);
    const bool inside = x < width && y < height;
    const size_t pix = (size_t)y * width + x;   // read only when inside
    if constexpr (LDS_STEP > 0) {
        constexpr int HALO = 2 * LDS_STEP, TW = BLOCK_W + 2 * HALO, TH = BLOCK_H + 2 * HALO;
        __shared__ float4 s_cv[TW * TH], s_nv[TW * TH];
        for (int i = threadIdx.x; i < TW * TH; i += BLOCK_W * BLOCK_H) {
            const int gx = bx - HALO + i % TW, gy = by - HALO + i / TW;
            float4 cv = make_float4(0.f, 0.f, 0.f, 0.f), nv = cv;
            if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
                const size_t g = (size_t)gy * width + gx;
                if (ok[g] != 0) {
                    cv = in[g];
                    nv = make_float4(normal3[3 * g], normal3[3 * g + 1], normal3[3 * g + 2], 1.0f);
                }
            }
            s_cv[i] = cv;
            s_nv[i] = nv;
        }
        __syncthreads();
        if (!inside) return;
        const TileSrc<TW> src{s_cv, s_nv, bx - HALO, by - HALO};
        out[pix] = src.valid(x, y) ? as_f4(filter::level_pixel(src, x, y, width, height, LDS_STEP, sig2, sharpness_log2))
                                   : in[pix];
    } else {
        if (!inside) return;
        const GlobalSrc src{in, normal3, ok, width};
        out[pix] = src.valid(x, y) ? as_f4(filter::level_pixel(src, x, y, width, height, step, sig2, sharpness_log2)) : in[pix];
    }
}

hipError_t launch_filter_prepare(const float4* accum, const float* stat, size_t npix, float4* plane, uint8_t* ok,
                                 hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(k_filter_prepare, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, accum, stat, npix, plane, ok);
    return hipGetLastError();
}

hipError_t launch_filter_level(const float4* in, const float* normal3, const uint8_t* ok, float4* out, int width, int height,
                               int step, float sig2, int sharpness_log2, hipStream_t stream) {
    const dim3 grid((unsigned)((width + BLOCK_W - 1) / BLOCK_W), (unsigned)((height + BLOCK_H - 1) / BLOCK_H)),
        block(BLOCK_W * BLOCK_H);
    if (step == 1 && FILTER_LDS_MAX_STEP >= 1)
        hipLaunchKernelGGL(k_filter_level<1>, grid, block, 0, stream, in, normal3, ok, out, width, height, step, sig2, sharpness_log2);
    else if (step == 2 && FILTER_LDS_MAX_STEP >= 2)
        hipLaunchKernelGGL(k_filter_level<2>, grid, block, 0, stream, in, normal3, ok, out, width, height, step, sig2, sharpness_log2);
    else
        hipLaunchKernelGGL(k_filter_level<0>, grid, block, 0, stream, in, normal3, ok, out, width, height, step, sig2, sharpness_log2);
    return hipGetLastError();
}

}  // namespace cpt
