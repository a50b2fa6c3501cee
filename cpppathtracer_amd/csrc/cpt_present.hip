// cpt_present.hip — the kernels of cpt_meter_exposure and cpt_present.  The
// arithmetic is cpt_present.hpp's, shared with the host hooks; this file only decides where the
// operands come from and how the results are stored.
//
//   k_meter            a grid-stride pass over the source plane: each workgroup fills a 257-word
//                      histogram in LDS with LDS atomic adds and flushes its non-zero words once, with
//                      global atomic adds (integers: any order gives the same words)
//   k_meter_resolve    one workgroup, a second launch: an inclusive scan of the 256 bins in LDS, the
//                      bin of the percentile, the new exposure written behind the histogram
//   k_present          each lane takes four consecutive pixels (four float4 loads) and stores their
//                      BGRA8 as one 16-byte word, so a wave's store is 1 KB, contiguous; the pixels
//                      past the last whole group of four are stored as 4-byte words.  The 256 sRGB
//                      thresholds are staged in LDS and searched there, eight probes per component
//
// The reference has no counterpart (its display loop writes 255.99 * clamp(linear),
// path_tracer.cu:241-254).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_internal.hpp"
#include "cpt_present.hpp"

namespace cpt {

namespace {

namespace prs = present;

constexpr int BLOCK = 256;
constexpr int EXPOSURE_WORD = prs::HIST_WORDS;   // the exposure's bits, behind the histogram
static_assert(BLOCK == prs::HIST_BINS, "one lane per bin in the scan");
static_assert(BLOCK == PRESENT_SRGB_N, "one lane per threshold when the table is staged");

__device__ const float g_srgb_t[PRESENT_SRGB_N] = CPT_PRESENT_SRGB_TABLE_INIT;

}  // namespace

__global__ void __launch_bounds__(BLOCK) k_meter(const float4* __restrict__ src, size_t npix, int source,
                                                 uint32_t* __restrict__ words) {
    __shared__ uint32_t s_hist[prs::HIST_WORDS];
    for (int i = threadIdx.x; i < prs::HIST_WORDS; i += BLOCK) s_hist[i] = 0;
    __syncthreads();
    for (size_t pix = (size_t)blockIdx.x * BLOCK + threadIdx.x; pix < npix; pix += (size_t)gridDim.x * BLOCK) {
        const float4 S = src[pix];
        atomicAdd(&s_hist[prs::meter_word(source, S.x, S.y, S.z, S.w)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < prs::HIST_WORDS; i += BLOCK) {
        const uint32_t v = s_hist[i];
        if (v != 0) atomicAdd(&words[i], v);
    }
}

__global__ void __launch_bounds__(BLOCK) k_meter_resolve(uint32_t* __restrict__ words, float key, int permille, float adapt) {
    // cumulative counts as 64-bit sums: the frame's pixels need not fit 32 bits here
    __shared__ unsigned long long s_cum[2][BLOCK];
    const int b = threadIdx.x;
    s_cum[0][b] = words[b];
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < BLOCK; d <<= 1) {
        s_cum[cur ^ 1][b] = s_cum[cur][b] + (b >= d ? s_cum[cur][b - d] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long n = s_cum[cur][BLOCK - 1];
    if (n == 0) return;   // nothing metered: the exposure stays
    const unsigned long long rank = prs::meter_rank(n, permille);
    const unsigned long long below = b > 0 ? s_cum[cur][b - 1] : 0ull;
    if (s_cum[cur][b] > rank && below <= rank)   // the least bin whose cumulative count exceeds rank: one lane
        words[EXPOSURE_WORD] = prs::bits_of(prs::adapted(prs::float_of(words[EXPOSURE_WORD]), b, key, adapt));
}

__global__ void __launch_bounds__(BLOCK) k_present(const float4* __restrict__ src, size_t npix, int source, int tone, float white,
                                                   int transfer, const uint32_t* __restrict__ words, uint32_t* __restrict__ bgra) {
    __shared__ float s_t[PRESENT_SRGB_N];
    s_t[threadIdx.x] = g_srgb_t[threadIdx.x];
    __syncthreads();
    const float e = prs::float_of(words[EXPOSURE_WORD]);
    const size_t first = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (first >= npix) return;
    if (first + 4 <= npix) {
        // the four loads first, so that all are in flight before the first pixel's arithmetic
        const float4 S[4] = {src[first], src[first + 1], src[first + 2], src[first + 3]};
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = prs::pixel_word(source, S[k].x, S[k].y, S[k].z, S[k].w, e, tone, white, transfer, s_t);
        // 16-byte aligned: the plane is an allocation's start and `first` a multiple of 4
        *reinterpret_cast<uint4*>(bgra + first) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (size_t pix = first; pix < npix; ++pix) {
            const float4 S = src[pix];
            bgra[pix] = prs::pixel_word(source, S.x, S.y, S.z, S.w, e, tone, white, transfer, s_t);
        }
    }
}

hipError_t launch_meter(const float4* src, size_t npix, int source, float key, int permille, float adapt, uint32_t* words,
                        int cus, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(words, 0, prs::HIST_WORDS * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    if (npix != 0) {
        const size_t want = (npix + BLOCK - 1) / BLOCK, most = (size_t)(cus > 0 ? cus : 1) * 4;
        hipLaunchKernelGGL(k_meter, dim3((unsigned)(want < most ? want : most)), dim3(BLOCK), 0, stream, src, npix, source, words);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_meter_resolve, dim3(1), dim3(BLOCK), 0, stream, words, key, permille, adapt);
    return hipGetLastError();
}

hipError_t launch_present(const float4* src, size_t npix, int source, int tone, float white, int transfer,
                          const uint32_t* words, uint8_t* bgra, hipStream_t stream) {
    if (npix == 0) return hipSuccess;
    const size_t groups = (npix + 3) / 4;
    hipLaunchKernelGGL(k_present, dim3((unsigned)((groups + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, src, npix, source, tone,
                       white, transfer, words, reinterpret_cast<uint32_t*>(bgra));
    return hipGetLastError();
}

}  // namespace cpt
