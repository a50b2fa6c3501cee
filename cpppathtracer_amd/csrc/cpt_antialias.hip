// cpt_antialias.hip — the kernels of cpt_aa_coverage and cpt_present_aa.  The
// definition is cpt_antialias.hpp's, shared with the host hooks; this file decides which lane takes
// which sub-sample, how a pixel's counts are gathered and how the results are stored.
//
//   k_aa_edges            one pass over the G-buffer's id and normal planes, a lane per pixel: the
//                         coverage word of every non-edge pixel (all on itself) and the edge pixels
//                         appended to a list, one __ballot + mbcnt prefix and one atomic per wave
//   k_aa_coverage<LDST>   grid-stride over the list, whose length is read from device memory: a
//                         lane is one (pixel, sub-sample), so a wave holds 64 / S^2 pixels and a
//                         pixel's coherent rays sit in adjacent lanes.  The walk is the one
//                         k_ray_query calls (trace_segment, the LDS image under use_lds_tree).  A
//                         pixel's nine counts are nine ballots masked to its lane group, no LDS and
//                         no atomics; the group's first lane stores the 16-byte word
//   k_present_aa          k_present's structure (thresholds in LDS, four pixels and one 16-byte
//                         store per lane): a lane whose four pixels are all covered by themselves
//                         runs k_present's arithmetic, an edge pixel loads its neighbours' sources
//
// The reference has no counterpart (RayGen has no pixel offset, motional_camera.cu:202-213).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_antialias.hpp"
#include "cpt_path.hpp"
#include "cpt_present_tables.hpp"

namespace cpt {

namespace {

namespace aa = antialias;
namespace prs = present;

constexpr int BLOCK = 256;
constexpr int EXPOSURE_WORD = prs::HIST_WORDS;   // the exposure's bits, behind the histogram (cpt_present.hip)
static_assert(BLOCK == PRESENT_SRGB_N, "one lane per threshold when the table is staged");

// This file's own copy of the 1 KB table: k_present's (cpt_present.hip) is local to its translation
// unit, and a device variable is shared between units only by relocatable device code, which the
// build does not use, or by a symbol look-up at run time, which the runtime refuses for it.
__device__ const float g_aa_srgb_t[PRESENT_SRGB_N] = CPT_PRESENT_SRGB_TABLE_INIT;

// as k_ray_query's blocks (cpt_query.hip): LDS_BLOCK lanes with the LDS image, else WIDE_LANES
template <bool LDST> constexpr int coverage_block() { return LDST ? LDS_BLOCK : WIDE_LANES; }

struct FetchPlane {
    const float4* src;
    __device__ void operator()(size_t q, float s4[4]) const {
        const float4 v = src[q];
        s4[0] = v.x;
        s4[1] = v.y;
        s4[2] = v.z;
        s4[3] = v.w;
    }
};

}  // namespace

__global__ void __launch_bounds__(BLOCK) k_aa_edges(const int32_t* __restrict__ id, const float* __restrict__ normal3, int width,
                                                    int height, float normal_cos, uint32_t s2, uint4* __restrict__ cov,
                                                    uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
    const size_t npix = (size_t)width * height;
    const size_t pix = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    bool edge = false;
    if (pix < npix) {
        edge = aa::is_edge(width, height, (int)(pix % width), (int)(pix / width), id, normal3, normal_cos);
        if (!edge) cov[pix] = aa::pack_self(s2);
    }
    // every lane of the wave is here: the wave's edge pixels take consecutive list slots
    const uint64_t m = __ballot(edge);
    uint32_t base = 0;
    if ((threadIdx.x & 63) == 0 && m != 0) base = atomicAdd(count, wave_count(m));
    base = __shfl(base, 0, 64);
    if (edge) list[base + lane_rank(m)] = (uint32_t)pix;
}

template <bool LDST>
__global__ void __launch_bounds__(coverage_block<LDST>()) k_aa_coverage(const KParams p, const int32_t* __restrict__ rank_obj,
                                                                         const int32_t* __restrict__ gid,
                                                                         const float* __restrict__ gnormal3, int S, float normal_cos,
                                                                         const uint32_t* __restrict__ list,
                                                                         const uint32_t* __restrict__ count, uint4* __restrict__ cov) {
    constexpr int BLK = coverage_block<LDST>();
    __shared__ uint4 s_tree[LDST ? LDS_TREE_NODES * 7 : 1];
    const uint32_t s2 = (uint32_t)(S * S);
    const uint64_t total = (uint64_t)*count * s2;
    // the grid is sized for every pixel, the list is usually a few percent of them: a workgroup
    // whose first sub-sample lies past the list leaves before it stages the tree (all its lanes do:
    // the condition is the workgroup's)
    if ((uint64_t)blockIdx.x * BLK >= total) return;
    if (LDST) {
        stage_wide_tree<BLK>(s_tree, p);
    }
    const uint32_t lane = threadIdx.x & 63u;
    // the lanes of this lane's pixel: S^2 adjacent ones (BLK and the stride are multiples of 64)
    const uint64_t group = (s2 == 16u ? 0xFFFFull : 0xFull) << (lane & ~(s2 - 1u));
    // `base` is the same in every lane of a workgroup, so a wave's lanes stay together for the ballots
    for (uint64_t base = (uint64_t)blockIdx.x * BLK; base < total; base += (uint64_t)gridDim.x * BLK) {
        const uint64_t i = base + threadIdx.x;
        const bool have = i < total;   // whole lane groups: total is a multiple of S^2
        uint32_t pix = 0;
        int k = -2;                    // -2: no sub-sample; -1: unmatched
        if (have) {
            pix = list[i / s2];
            const int s = (int)(i % s2), x = (int)(pix % (uint32_t)p.width), y = (int)(pix / (uint32_t)p.width);
            float o[3], d[3];
            aa::sub_ray(p.cam, S, x, y, s, o, d);
            Ray ray;
            ray.o = mk(o[0], o[1], o[2]);
            ray.d = mk(d[0], d[1], d[2]);
            ray.tmin = 0.f;
            ray.tmax = DEFAULT_RAY_TMAX;
            const RayK rk = make_rayk(ray);
            const bool finite = ray_is_finite(ray);
            Hit h;
            Winner win{-1, -1, DEFAULT_RAY_TMAX};
            Counters cnt{};
            bool hit;
            if (LDST) hit = trace_segment<false, BLK, true>(p, rk, finite, h, win, cnt, s_tree);
            else hit = trace_segment<false>(p, rk, finite, h, win, cnt);
            // as k_ray_query reports it: a miss is -1 with the normal -dir
            const v3 n = hit ? h.normal : -ray.d;
            const float n_s[3] = {n.x, n.y, n.z};
            k = aa::attribute(p.width, p.cam.height, x, y, S, s, hit ? rank_obj[win.rank] : -1, n_s, gid, gnormal3, normal_cos);
        }
        aa::Coverage v;
#pragma unroll
        for (int kk = 0; kk < 9; ++kk) v.c[kk] = wave_count(__ballot(k == kk) & group);
        const uint32_t unmatched = wave_count(__ballot(k == -1) & group);
        v.c[aa::SELF] += unmatched;
        v.flags = aa::FLAG_EDGE | (unmatched ? aa::FLAG_UNMATCHED : 0u);
        if (have && (lane & (s2 - 1u)) == 0u) cov[pix] = aa::pack(v);
    }
}

__global__ void __launch_bounds__(BLOCK) k_present_aa(const float4* __restrict__ src, const uint4* __restrict__ cov, int width, int height,
                                                      int S, int source, int tone, float white, int transfer,
                                                      const uint32_t* __restrict__ words, uint32_t* __restrict__ bgra) {
    __shared__ float s_t[PRESENT_SRGB_N];
    s_t[threadIdx.x] = g_aa_srgb_t[threadIdx.x];
    __syncthreads();
    const size_t npix = (size_t)width * height;
    const float e = prs::float_of(words[EXPOSURE_WORD]);
    const uint32_t s2 = (uint32_t)(S * S);
    const size_t first = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * 4;
    if (first >= npix) return;
    const FetchPlane fetch{src};
    auto edge_word = [&](size_t pix, const uint4& c) {
        return aa::pixel_word(fetch, width, height, (int)(pix % width), (int)(pix / width), aa::unpack(c), S, source, e, tone, white,
                              transfer, s_t);
    };
    if (first + 4 <= npix) {
        const uint4 C[4] = {cov[first], cov[first + 1], cov[first + 2], cov[first + 3]};
        const float4 P[4] = {src[first], src[first + 1], src[first + 2], src[first + 3]};
        uint32_t w[4];
        if (aa::all_on_self(C[0], s2) && aa::all_on_self(C[1], s2) && aa::all_on_self(C[2], s2) && aa::all_on_self(C[3], s2)) {
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = prs::pixel_word(source, P[k].x, P[k].y, P[k].z, P[k].w, e, tone, white, transfer, s_t);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = aa::all_on_self(C[k], s2) ? prs::pixel_word(source, P[k].x, P[k].y, P[k].z, P[k].w, e, tone, white, transfer, s_t)
                                                 : edge_word(first + k, C[k]);
        }
        // 16-byte aligned: the plane is an allocation's start and `first` a multiple of 4
        *reinterpret_cast<uint4*>(bgra + first) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (size_t pix = first; pix < npix; ++pix) bgra[pix] = edge_word(pix, cov[pix]);
    }
}

hipError_t launch_aa_edges(const int32_t* id, const float* normal3, int width, int height, int samples, float normal_cos, uint4* cov,
                           uint32_t* list, uint32_t* count, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(count, 0, sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const size_t npix = (size_t)width * height;
    if (npix == 0) return hipSuccess;
    hipLaunchKernelGGL(k_aa_edges, dim3((unsigned)((npix + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, id, normal3, width, height,
                       normal_cos, (uint32_t)(samples * samples), cov, list, count);
    return hipGetLastError();
}

template <bool LDST>
static hipError_t launch_coverage_t(const KParams& p, const int32_t* rank_obj, const int32_t* id, const float* normal3, int samples,
                                    float normal_cos, const uint32_t* list, const uint32_t* count, uint4* cov, LaunchGrid& g,
                                    hipStream_t stream) {
    constexpr int block = coverage_block<LDST>();
    // the list's length is the device's: at most every pixel, so at most this many workgroups have
    // work, and every resident slot is taken at most once (the test hook's cap applies)
    const long long lanes = (long long)p.width * p.cam.height * samples * samples;
    int grid = 0;
    const hipError_t e = g.size((const void*)k_aa_coverage<LDST>, block, (lanes + block - 1) / block, true, &grid);
    if (e != hipSuccess || grid < 1) return e;
    hipLaunchKernelGGL((k_aa_coverage<LDST>), dim3((unsigned)grid), dim3(block), 0, stream, p, rank_obj, id, normal3, samples, normal_cos,
                       list, count, cov);
    return hipGetLastError();
}

hipError_t launch_aa_coverage(const KParams& p, const int32_t* rank_obj, const int32_t* id, const float* normal3, int samples,
                              float normal_cos, const uint32_t* list, const uint32_t* count, uint4* cov, LaunchGrid& grid,
                              hipStream_t stream) {
    return use_lds_tree(p) ? launch_coverage_t<true>(p, rank_obj, id, normal3, samples, normal_cos, list, count, cov, grid, stream)
                           : launch_coverage_t<false>(p, rank_obj, id, normal3, samples, normal_cos, list, count, cov, grid, stream);
}

hipError_t launch_present_aa(const float4* src, const uint4* cov, int width, int height, int samples, int source, int tone, float white,
                             int transfer, const uint32_t* words, uint8_t* bgra, hipStream_t stream) {
    const size_t npix = (size_t)width * height;
    if (npix == 0) return hipSuccess;
    const size_t groups = (npix + 3) / 4;
    hipLaunchKernelGGL(k_present_aa, dim3((unsigned)((groups + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, stream, src, cov, width, height,
                       samples, source, tone, white, transfer, words, reinterpret_cast<uint32_t*>(bgra));
    return hipGetLastError();
}

}  // namespace cpt
