// cpt_filter.hip — the kernels of cpt_filter_frame, the variance-guided a-trous
// filter of an adaptive render's final frame, and of cpt_filter_frame_spatial (§25), the same
// filter for frames without moments.  The arithmetic is cpt_filter.hpp's, shared with the
// host hooks; this file only decides where a tap's operands come from.
//
//   k_filter_prepare   level 0: each pixel's mean, variance of the mean and validity from the
//                      accumulator and the adaptive render's moments
//   k_filter_level     one level: a 256-lane workgroup owns a 64 x 4 pixel block, each wave one
//                      64-pixel row segment (a float4 load or store of a wave is 1 KB, coalesced).
//                      LDS_STEP > 0 (steps 1 and 2): the block's pixels, normals and validity are
//                      staged in LDS with their 2 * step halo and every tap reads the tile;
//                      LDS_STEP == 0: the taps read global memory (L2 serves the strided ones).
//                      ID_STOP (§25): a tap of another object of the G-buffer's id plane is
//                      skipped; the id has a tile of its own beside the normal and validity entry
//   k_filter_prepare_spatial   level 0 without moments: the level kernel's block, its operands
//                      (luminance, count, normal, id, base validity) staged once in LDS with a halo
//                      of 3 as two 16-byte slots per entry, both passes over the 49 taps read the tile
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

struct GlobalIdSrc : GlobalSrc {
    const int32_t* ids;
    __device__ int id(int x, int y) const { return ids[(size_t)y * width + x]; }
};

template <int TW>
struct TileIdSrc : TileSrc<TW> {
    const int32_t* ids;
    __device__ int id(int x, int y) const { return ids[this->at(x, y)]; }
};

// The tile of k_filter_prepare_spatial: nl = (normal, luminance), cb = (count, id as bits, base
// validity as 1 or 0, unused); entries outside the frame are not base-valid.
constexpr int SP_HALO = filter::SPATIAL_RADIUS, SP_TW = BLOCK_W + 2 * SP_HALO, SP_TH = BLOCK_H + 2 * SP_HALO;

struct SpatialTileSrc {
    const float4* nl;
    const float4* cb;
    int x0, y0;
    __device__ int at(int x, int y) const { return (y - y0) * SP_TW + (x - x0); }
    // both slots whole: consecutive lanes read consecutive 16-byte entries
    __device__ filter::SpatialTap tap(int x, int y) const {
        const int i = at(x, y);
        const float4 a = nl[i], b = cb[i];
        return filter::SpatialTap{a.x, a.y, a.z, a.w, b.x, __float_as_int(b.y), b.z != 0.0f};
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

__global__ void __launch_bounds__(BLOCK_W* BLOCK_H) k_filter_prepare_spatial(const float4* __restrict__ accum,
                                                                            const int32_t* __restrict__ id,
                                                                            const float* __restrict__ normal3, int width, int height,
                                                                            int sharpness_log2, float4* __restrict__ plane,
                                                                            uint8_t* __restrict__ ok) {
    const int bx = blockIdx.x * BLOCK_W, by = blockIdx.y * BLOCK_H;
    const int x = bx + (int)(threadIdx.x & 63), y = by + (int)(threadIdx.x >> 6);
    __shared__ float4 s_nl[SP_TW * SP_TH], s_cb[SP_TW * SP_TH];
    for (int i = threadIdx.x; i < SP_TW * SP_TH; i += BLOCK_W * BLOCK_H) {
        const int gx = bx - SP_HALO + i % SP_TW, gy = by - SP_HALO + i / SP_TW;
        float4 nl = make_float4(0.f, 0.f, 0.f, 0.f), cb = nl;
        if (gx >= 0 && gx < width && gy >= 0 && gy < height) {
            const size_t g = (size_t)gy * width + gx;
            const float4 S = accum[g];
            filter::Px c;
            if (filter::spatial_base(S.x, S.y, S.z, S.w, c)) {
                nl = make_float4(normal3[3 * g], normal3[3 * g + 1], normal3[3 * g + 2], filter::luma(c));
                cb = make_float4(S.w, __int_as_float(id[g]), 1.0f, 0.f);
            }
        }
        s_nl[i] = nl;
        s_cb[i] = cb;
    }
    __syncthreads();
    if (x >= width || y >= height) return;
    const size_t pix = (size_t)y * width + x;
    const float4 S = accum[pix];
    const SpatialTileSrc src{s_nl, s_cb, bx - SP_HALO, by - SP_HALO};
    filter::Px c;
    const bool valid = filter::prepare_spatial(src, x, y, width, height, S.x, S.y, S.z, S.w, sharpness_log2, c);
    plane[pix] = as_f4(c);
    ok[pix] = valid ? 1 : 0;
}

// `id` is read by the ID_STOP instantiations only.
template <int LDS_STEP, bool ID_STOP = false>
__global__ void __launch_bounds__(BLOCK_W* BLOCK_H) k_filter_level(const float4* __restrict__ in, const float* __restrict__ normal3,
                                                                  const uint8_t* __restrict__ ok, float4* __restrict__ out,
                                                                  int width, int height, int step, float sig2, int sharpness_log2,
                                                                  const int32_t* __restrict__ id) {
    const int bx = blockIdx.x * BLOCK_W, by = blockIdx.y * BLOCK_H;
    const int x = bx + (int)(threadIdx.x & 63), y = by + (int)(threadIdx.x >> 6);
    const bool inside = x < width && y < height;
    const size_t pix = (size_t)y * width + x;   // read only when inside
    if constexpr (LDS_STEP > 0) {
        constexpr int HALO = 2 * LDS_STEP, TW = BLOCK_W + 2 * HALO, TH = BLOCK_H + 2 * HALO;
        __shared__ float4 s_cv[TW * TH], s_nv[TW * TH];
        __shared__ int32_t s_id[ID_STOP ? TW * TH : 1];
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
            if constexpr (ID_STOP) s_id[i] = nv.w != 0.0f ? id[(size_t)gy * width + gx] : 0;
        }
        __syncthreads();
        if (!inside) return;
        if constexpr (ID_STOP) {
            const TileIdSrc<TW> src{{s_cv, s_nv, bx - HALO, by - HALO}, s_id};
            out[pix] = src.valid(x, y)
                           ? as_f4(filter::level_pixel<TileIdSrc<TW>, true>(src, x, y, width, height, LDS_STEP, sig2, sharpness_log2))
                           : in[pix];
        } else {
            const TileSrc<TW> src{s_cv, s_nv, bx - HALO, by - HALO};
            out[pix] = src.valid(x, y) ? as_f4(filter::level_pixel(src, x, y, width, height, LDS_STEP, sig2, sharpness_log2))
                                       : in[pix];
        }
    } else {
        if (!inside) return;
        if constexpr (ID_STOP) {
            const GlobalIdSrc src{{in, normal3, ok, width}, id};
            out[pix] = src.valid(x, y) ? as_f4(filter::level_pixel<GlobalIdSrc, true>(src, x, y, width, height, step, sig2, sharpness_log2))
                                       : in[pix];
        } else {
            const GlobalSrc src{in, normal3, ok, width};
            out[pix] = src.valid(x, y) ? as_f4(filter::level_pixel(src, x, y, width, height, step, sig2, sharpness_log2)) : in[pix];
        }
    }
}

hipError_t launch_filter_prepare(const float4* accum, const float* stat, size_t npix, float4* plane, uint8_t* ok,
                                 hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(k_filter_prepare, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, accum, stat, npix, plane, ok);
    return hipGetLastError();
}

hipError_t launch_filter_prepare_spatial(const float4* accum, const int32_t* id, const float* normal3, int width, int height,
                                         int sharpness_log2, float4* plane, uint8_t* ok, hipStream_t stream) {
    if (width <= 0 || height <= 0) return hipSuccess;
    const dim3 grid((unsigned)((width + BLOCK_W - 1) / BLOCK_W), (unsigned)((height + BLOCK_H - 1) / BLOCK_H)),
        block(BLOCK_W * BLOCK_H);
    hipLaunchKernelGGL(k_filter_prepare_spatial, grid, block, 0, stream, accum, id, normal3, width, height, sharpness_log2, plane, ok);
    return hipGetLastError();
}

namespace {

template <bool ID_STOP>
hipError_t launch_level(const float4* in, const float* normal3, const int32_t* id, const uint8_t* ok, float4* out, int width,
                        int height, int step, float sig2, int sharpness_log2, hipStream_t stream) {
    const dim3 grid((unsigned)((width + BLOCK_W - 1) / BLOCK_W), (unsigned)((height + BLOCK_H - 1) / BLOCK_H)),
        block(BLOCK_W * BLOCK_H);
    if (step == 1 && FILTER_LDS_MAX_STEP >= 1)
        hipLaunchKernelGGL((k_filter_level<1, ID_STOP>), grid, block, 0, stream, in, normal3, ok, out, width, height, step, sig2,
                           sharpness_log2, id);
    else if (step == 2 && FILTER_LDS_MAX_STEP >= 2)
        hipLaunchKernelGGL((k_filter_level<2, ID_STOP>), grid, block, 0, stream, in, normal3, ok, out, width, height, step, sig2,
                           sharpness_log2, id);
    else
        hipLaunchKernelGGL((k_filter_level<0, ID_STOP>), grid, block, 0, stream, in, normal3, ok, out, width, height, step, sig2,
                           sharpness_log2, id);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_filter_level(const float4* in, const float* normal3, const uint8_t* ok, float4* out, int width, int height,
                               int step, float sig2, int sharpness_log2, hipStream_t stream) {
    return launch_level<false>(in, normal3, nullptr, ok, out, width, height, step, sig2, sharpness_log2, stream);
}

hipError_t launch_filter_level_id(const float4* in, const float* normal3, const int32_t* id, const uint8_t* ok, float4* out,
                                  int width, int height, int step, float sig2, int sharpness_log2, hipStream_t stream) {
    return launch_level<true>(in, normal3, id, ok, out, width, height, step, sig2, sharpness_log2, stream);
}

}  // namespace cpt
