// cpt_bloom.hip — the kernels of cpt_bloom and cpt_present_bloom.  The definition
// is cpt_bloom.hpp's, shared with the host hooks; this file decides where the operands come from
// and how the results are stored.
//
//   k_bloom_first      the only pass over the full-resolution plane: a workgroup makes a 32 x 8 tile
//                      of level-1 texels from a 66 x 18 patch of source pixels.  Each lane issues its
//                      float4 loads of the patch (five at most) before any arithmetic, runs the bright
//                      pass once per loaded pixel into three LDS planes and filters from them with
//                      8-byte LDS reads; only the patch's one-pixel halo is read by two workgroups
//   k_bloom_down       one level step, a lane per texel of the coarser level (sixteen float4 loads)
//   k_bloom_up         U_l = B_l + up(U_{l+1}) in place, a lane per texel of level l: B_l is read at
//                      the lane's own texel only
//   k_present_bloom    k_present's structure (thresholds in LDS, four pixels and one 16-byte store per
//                      lane) with the four-texel up(U_1) fetch per pixel
//
// Every level step is a launch of its own.  A kernel that ran the small levels in one workgroup's
// LDS between barriers was measured and lost to the launches it replaced.
//
// The reference has no counterpart.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_bloom.hpp"
#include "cpt_internal.hpp"
#include "cpt_present_tables.hpp"

namespace cpt {

namespace {

namespace prs = present;
using bloom::Rgb;

constexpr int BLOCK = 256;
constexpr int EXPOSURE_WORD = prs::HIST_WORDS;   // the exposure's bits, behind the histogram (cpt_present.hip)
static_assert(BLOCK == PRESENT_SRGB_N, "one lane per threshold when the table is staged");

// k_bloom_first's tile of level-1 texels and the patch of source pixels under it
constexpr int TILE_W = 32, TILE_H = 8;
constexpr int PATCH_W = 2 * TILE_W + 2, PATCH_H = 2 * TILE_H + 2, PATCH = PATCH_W * PATCH_H;
constexpr int PATCH_LOADS = (PATCH + BLOCK - 1) / BLOCK;
static_assert(TILE_W * TILE_H == BLOCK, "one lane per texel of the tile");
static_assert(PATCH_W % 2 == 0, "a lane's taps are two aligned 8-byte LDS reads");

// This file's own copy of the 1 KB table, as cpt_antialias.hip's: a device variable does not cross
// translation units in this build.
__device__ const float g_bloom_srgb_t[PRESENT_SRGB_N] = CPT_PRESENT_SRGB_TABLE_INIT;

// a level in device memory: float4 texels (rgb, 0), row-major
struct FetchPlane {
    const float4* t;
    int w;
    __device__ Rgb operator()(int x, int y) const {
        const float4 v = t[(size_t)y * w + x];
        return Rgb{v.x, v.y, v.z};
    }
};

}  // namespace

__global__ void __launch_bounds__(BLOCK) k_bloom_first(const float4* __restrict__ src, int W, int H, int source, float threshold,
                                                       const uint32_t* __restrict__ words, float4* __restrict__ out, int w1, int h1) {
    __shared__ __align__(16) float s_c[3][PATCH];
    const float e = prs::float_of(words[EXPOSURE_WORD]);
    const int x0 = 2 * (int)blockIdx.x * TILE_W - 1, y0 = 2 * (int)blockIdx.y * TILE_H - 1;   // the patch's first column and row
    // every load first: the clamped coordinates are inside the frame, whatever the tile
    float4 S[PATCH_LOADS];
#pragma unroll
    for (int k = 0; k < PATCH_LOADS; ++k) {
        const int i = min((int)threadIdx.x + k * BLOCK, PATCH - 1);
        const int x = bloom::clampi(x0 + i % PATCH_W, W - 1), y = bloom::clampi(y0 + i / PATCH_W, H - 1);
        S[k] = src[(size_t)y * W + x];
    }
#pragma unroll
    for (int k = 0; k < PATCH_LOADS; ++k) {
        const int i = (int)threadIdx.x + k * BLOCK;
        if (i < PATCH) {
            const Rgb b = bloom::bright(bloom::exposed(source, S[k].x, S[k].y, S[k].z, S[k].w, e), threshold);
            s_c[0][i] = b.r;
            s_c[1][i] = b.g;
            s_c[2][i] = b.b;
        }
    }
    __syncthreads();
    const int tx = threadIdx.x % TILE_W, ty = threadIdx.x / TILE_W;
    const int X = (int)blockIdx.x * TILE_W + tx, Y = (int)blockIdx.y * TILE_H + ty;
    if (X >= w1 || Y >= h1) return;
    // the patch holds the clamped columns 2X - 1 .. 2X + 2 at 2 tx .. 2 tx + 3, rows alike
    float c[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2* row = reinterpret_cast<const float2*>(&s_c[ch][(2 * ty + j) * PATCH_W + 2 * tx]);
            const float2 a = row[0], b = row[1];
            r[j] = bloom::tap4(a.x, a.y, b.x, b.y);
        }
        c[ch] = bloom::tap4(r[0], r[1], r[2], r[3]) * 0.015625f;
    }
    out[(size_t)Y * w1 + X] = make_float4(c[0], c[1], c[2], 0.0f);
}

__global__ void __launch_bounds__(BLOCK) k_bloom_down(const float4* __restrict__ fine, int w, int h, float4* __restrict__ coarse, int wc,
                                                      int hc) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);   // a level's texels fit an int: at most a quarter of the frame's
    if (i >= wc * hc) return;
    const Rgb v = bloom::down(FetchPlane{fine, w}, w, h, i % wc, i / wc);
    coarse[i] = make_float4(v.r, v.g, v.b, 0.0f);
}

__global__ void __launch_bounds__(BLOCK) k_bloom_up(float4* __restrict__ fine, int w, int h, const float4* __restrict__ coarse, int wc,
                                                    int hc) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i >= w * h) return;
    const float4 own = fine[i];
    const Rgb v = bloom::sum(Rgb{own.x, own.y, own.z}, bloom::up(FetchPlane{coarse, wc}, wc, hc, i % w, i / w));
    fine[i] = make_float4(v.r, v.g, v.b, 0.0f);
}

__global__ void __launch_bounds__(BLOCK) k_present_bloom(const float4* __restrict__ src, const float4* __restrict__ u1, int W, int H,
                                                         int source, int tone, float white, int transfer, float intensity,
                                                         const uint32_t* __restrict__ words, uint32_t* __restrict__ bgra) {
    __shared__ float s_t[PRESENT_SRGB_N];
    s_t[threadIdx.x] = g_bloom_srgb_t[threadIdx.x];
    __syncthreads();
    const size_t npix = (size_t)W * H;
    const float e = prs::float_of(words[EXPOSURE_WORD]);
    const size_t first = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (first >= npix) return;
    const int w1 = (W + 1) / 2, h1 = (H + 1) / 2;
    const FetchPlane glow{u1, w1};
    // the lane's first pixel by one division; its others step along the row and wrap
    int y = (int)(first / (size_t)W), x = (int)(first - (size_t)y * W);
    auto word = [&](const float4& S) {
        const Rgb g = bloom::up(glow, w1, h1, x, y);
        if (++x == W) {
            x = 0;
            ++y;
        }
        return bloom::pixel_word(bloom::exposed(source, S.x, S.y, S.z, S.w, e), g, intensity, tone, white, transfer, s_t);
    };
    if (first + 4 <= npix) {
        // the four loads first, so that all are in flight before the first pixel's arithmetic
        const float4 S[4] = {src[first], src[first + 1], src[first + 2], src[first + 3]};
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = word(S[k]);
        // 16-byte aligned: the plane is an allocation's start and `first` a multiple of 4
        *reinterpret_cast<uint4*>(bgra + first) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (size_t pix = first; pix < npix; ++pix) bgra[pix] = word(src[pix]);
    }
}

hipError_t launch_bloom(const float4* src, int W, int H, int source, float threshold, int levels, const uint32_t* words, float4* pyr,
                        hipStream_t stream) {
    if (W <= 0 || H <= 0) return hipSuccess;
    const bloom::Pyramid p = bloom::pyramid_of(W, H);
    const auto blocks = [](int texels) { return dim3((unsigned)((texels + BLOCK - 1) / BLOCK)); };
    hipLaunchKernelGGL(k_bloom_first, dim3((unsigned)((p.w[1] + TILE_W - 1) / TILE_W), (unsigned)((p.h[1] + TILE_H - 1) / TILE_H)),
                       dim3(BLOCK), 0, stream, src, W, H, source, threshold, words, pyr, p.w[1], p.h[1]);
    hipError_t e = hipGetLastError();
    for (int l = 1; l < levels && e == hipSuccess; ++l) {
        hipLaunchKernelGGL(k_bloom_down, blocks(p.w[l + 1] * p.h[l + 1]), dim3(BLOCK), 0, stream, pyr + p.off[l], p.w[l], p.h[l],
                           pyr + p.off[l + 1], p.w[l + 1], p.h[l + 1]);
        e = hipGetLastError();
    }
    for (int l = levels - 1; l >= 1 && e == hipSuccess; --l) {
        hipLaunchKernelGGL(k_bloom_up, blocks(p.w[l] * p.h[l]), dim3(BLOCK), 0, stream, pyr + p.off[l], p.w[l], p.h[l], pyr + p.off[l + 1],
                           p.w[l + 1], p.h[l + 1]);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_present_bloom(const float4* src, const float4* pyr, int W, int H, int source, int tone, float white, int transfer,
                                float intensity, const uint32_t* words, uint8_t* bgra, hipStream_t stream) {
    const size_t npix = (size_t)W * H;
    if (npix == 0) return hipSuccess;
    const size_t groups = (npix + 3) / 4;
    hipLaunchKernelGGL(k_present_bloom, dim3((unsigned)((groups + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, src, pyr, W, H, source,
                       tone, white, transfer, intensity, words, reinterpret_cast<uint32_t*>(bgra));
    return hipGetLastError();
}

}  // namespace cpt
