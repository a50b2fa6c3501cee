// cpt_kernels.hip — scene-preparation kernels of the MI355X integrator (gfx950, wave64).
//
//   k_rng_*              InitCuRand (path_tracer.cu:36-42) as three GF(2) kernels
//   k_refit_leaves/nodes SceneBVH::UpdateObject / UpdateSceneBVH (bvh.cu:122-157) on the device
//   launch_init_rng, launch_refit
//
// The megakernel (and k_prepare_materials, beside it) is in cpt_megakernel.hip, the cost
// schedule in cpt_schedule.hip, the display path in cpt_display.hip, the self-tests and probes
// in cpt_selftest.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_path.hpp"

namespace cpt {

// ======================================================================================
// InitCuRand (path_tracer.cu:36-42): curand_init(seed, (x<<32)|y, 0) per pixel, i.e.
// v = A^(2^67 * ((x<<32)|y)) v_seed.  Factored as v = M_y (N_x v_seed) with
// M_y = A^(2^67 y), N_x = A^(2^99 x) — GF(2) linear, exact.  jumps[t] = A^(2^67 * 2^t)
// (160x160 bits, column-major: column c = 5 words at [t][c*5..c*5+4]).
// All loops over matrix columns are wave-uniform, so the column loads are uniform too.
// ======================================================================================
__device__ __forceinline__ void matvec_uniform(const uint32_t* __restrict__ M, const uint32_t in[5], uint32_t out[5]) {
    uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0;
    for (int c = 0; c < 160; ++c) {
        uint32_t mask = 0u - ((in[c >> 5] >> (c & 31)) & 1u);
        const uint32_t* col = M + c * 5;
        r0 ^= mask & col[0];
        r1 ^= mask & col[1];
        r2 ^= mask & col[2];
        r3 ^= mask & col[3];
        r4 ^= mask & col[4];
    }
    out[0] = r0; out[1] = r1; out[2] = r2; out[3] = r3; out[4] = r4;
}

// w[x] = N_x v_seed for every column x of the frame (one thread per x).
__global__ void k_rng_columns(const uint32_t* __restrict__ jumps, uint32_t seed_v0, uint32_t seed_v1, uint32_t seed_v2,
                              uint32_t seed_v3, uint32_t seed_v4, int width, uint32_t* __restrict__ w) {
    int x = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t v[5] = {seed_v0, seed_v1, seed_v2, seed_v3, seed_v4};
    for (int t = 0; t < 31; ++t) {              // bits 32..62 of the subsequence
        uint32_t out[5];
        matvec_uniform(jumps + (size_t)(32 + t) * 800, v, out);
        bool take = x < width && ((x >> t) & 1);
        if (take) { v[0] = out[0]; v[1] = out[1]; v[2] = out[2]; v[3] = out[3]; v[4] = out[4]; }
        if (!__any(x < width && (x >> (t + 1)) != 0)) break;
    }
    if (x < width) for (int k = 0; k < 5; ++k) w[(size_t)k * width + x] = v[k];
}

// M_y for every distinct row: block = one row, 160 threads = the 160 columns.
__global__ void k_rng_rowmats(const uint32_t* __restrict__ jumps, const int32_t* __restrict__ rows,
                              uint32_t* __restrict__ mats) {
    const int ri = blockIdx.x;
    const int c = threadIdx.x;
    const uint32_t y = (uint32_t)rows[ri];
    uint32_t v[5] = {0, 0, 0, 0, 0};
    if (c < 160) v[c >> 5] = 1u << (c & 31);
    for (int t = 0; t < 32 && (y >> t) != 0; ++t) {
        if ((y >> t) & 1u) {
            uint32_t out[5];
            matvec_uniform(jumps + (size_t)t * 800, v, out);
            for (int k = 0; k < 5; ++k) v[k] = out[k];
        }
    }
    if (c < 160)
        for (int k = 0; k < 5; ++k) mats[(size_t)ri * 800 + c * 5 + k] = v[k];
}

// v_pixel = M_y w_x; d = the seed's d (2^67 k Weyl steps are 0 mod 2^32).  Grid: (x blocks, rows).
__global__ void k_rng_pixels(const uint32_t* __restrict__ rowmats, const uint32_t* __restrict__ w, int width,
                             int n_rows, uint32_t seed_d, uint32_t* __restrict__ rng) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int ri = blockIdx.y;
    const uint32_t* M = rowmats + (size_t)ri * 800;
    uint32_t in[5];
    const int xx = x < width ? x : width - 1;
    for (int k = 0; k < 5; ++k) in[k] = w[(size_t)k * width + xx];
    uint32_t out[5];
    matvec_uniform(M, in, out);
    if (x < width) {
        const size_t npix = (size_t)n_rows * width;
        const size_t pix = (size_t)ri * width + x;
        for (int k = 0; k < 5; ++k) rng[k * npix + pix] = out[k];
        rng[5 * npix + pix] = seed_d;
    }
}

// ======================================================================================
// Device refit (SceneBVH::UpdateObject / UpdateSceneBVH, bvh.cu:122-157).  The reference refits
// the updated leaf's ancestors on the host and copies the whole node array back to the GPU;
// here the host only names the updated leaves and their dirty ancestors (cpt_scene.cpp
// device_refit) and the boxes are recomputed where the nodes live, for both trees at once:
// the reference order, the walk tree's eight octant orders, its 4-wide image and leaf array.
// One thread per node; a launch per height, so a node's children are final before it runs.
// ======================================================================================
__device__ __forceinline__ float refit_min(float a, float b) { return a < b ? a : b; }   // MIN_ (ray_tracing_math.hpp:19-21)
__device__ __forceinline__ float refit_max(float a, float b) { return a > b ? a : b; }   // MAX_ (:15-17)

// A node's inline primitive into one of its copies (each copy keeps its own `miss`).
__device__ __forceinline__ void refit_put_prim(Node* n, const Node& v) {
    n->a0 = v.a0; n->a1 = v.a1; n->a2 = v.a2;
    n->b0 = v.b0; n->b1 = v.b1; n->b2 = v.b2;
    n->code = v.code;
}

// An internal node's box into one of its copies: octant form for the walk tree's octant
// orders (cpt_host_bvh.cpp linearise: the planes a ray of the octant enters through in a).
__device__ __forceinline__ void refit_put_box(Node* n, const Box6& b, int oct) {
    const bool sx = oct & 1, sy = oct & 2, sz = oct & 4;
    n->a0 = sx ? b.hi[0] : b.lo[0]; n->b0 = sx ? b.lo[0] : b.hi[0];
    n->a1 = sy ? b.hi[1] : b.lo[1]; n->b1 = sy ? b.lo[1] : b.hi[1];
    n->a2 = sz ? b.hi[2] : b.lo[2]; n->b2 = sz ? b.lo[2] : b.hi[2];
}

// A slot of the 4-wide image (7 x 16 B per node: [min x][max x][min y][max y][min z][max z] of
// the four slots, then the refs; cpt_host_bvh.cpp linearise_wide).
__device__ __forceinline__ void refit_put_slot(uint32_t* image, int slot, const Box6& b) {
    uint32_t* q = image + (size_t)(slot >> 2) * 28;
    const int k = slot & 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[(2 * a) * 4 + k] = __float_as_uint(b.lo[a]);
        q[(2 * a + 1) * 4 + k] = __float_as_uint(b.hi[a]);
    }
}

__global__ void __launch_bounds__(256) k_refit_leaves(const RefitLeaf* __restrict__ in, int n,
                                                      const RefitNode* __restrict__ plan, Box6* boxes, Node* nodes,
                                                      uint32_t* image, Node* leaves) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const RefitLeaf r = in[i];
    boxes[r.ref_id] = r.box;
    refit_put_prim(nodes + plan[r.ref_id].pos[0], r.prim);
    if (r.walk_id < 0) return;
    boxes[r.walk_id] = r.box;
    const RefitNode w = plan[r.walk_id];
#pragma unroll
    for (int o = 0; o < 8; ++o)
        if (w.pos[o] >= 0) refit_put_prim(nodes + w.pos[o], r.prim);
    if (w.leaf >= 0 && leaves) refit_put_prim(leaves + w.leaf, r.prim);
    if (w.slot >= 0 && image) refit_put_slot(image, w.slot, r.box);
}

__global__ void __launch_bounds__(256) k_refit_nodes(const int32_t* __restrict__ ids, int n, int n_ref,
                                                     const RefitNode* __restrict__ plan, Box6* boxes, Node* nodes,
                                                     uint32_t* image) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    const RefitNode r = plan[id];
    const Box6 L = boxes[r.left], R = boxes[r.right];
    Box6 b;
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // UPDATE_AABB_FOR_CUR_NODE (bvh.cu:130-139): MAX_/MIN_(left, right)
        b.hi[a] = refit_max(L.hi[a], R.hi[a]);
        b.lo[a] = refit_min(L.lo[a], R.lo[a]);
    }
    boxes[id] = b;
    if (id < n_ref) {
        refit_put_box(nodes + r.pos[0], b, 0);
    } else {
#pragma unroll
        for (int o = 0; o < 8; ++o) refit_put_box(nodes + r.pos[o], b, o);
    }
    if (r.slot >= 0 && image) refit_put_slot(image, r.slot, b);
}

hipError_t launch_refit(const RefitLeaf* leaves_in, int n_leaves, const int32_t* dirty, const int32_t* level_end,
                        int n_levels, int n_ref, const RefitNode* plan, Box6* boxes, Node* nodes, uint32_t* image,
                        Node* leaves, hipStream_t stream) {
    if (n_leaves > 0)
        hipLaunchKernelGGL(k_refit_leaves, dim3((n_leaves + 255) / 256), dim3(256), 0, stream, leaves_in, n_leaves, plan,
                           boxes, nodes, image, leaves);
    int begin = 0;
    for (int l = 0; l < n_levels; ++l) {
        const int n = level_end[l] - begin;
        if (n > 0)
            hipLaunchKernelGGL(k_refit_nodes, dim3((n + 255) / 256), dim3(256), 0, stream, dirty + begin, n, n_ref, plan,
                               boxes, nodes, image);
        begin = level_end[l];
    }
    return hipGetLastError();
}

hipError_t launch_init_rng(const uint32_t* jumps, const uint32_t seed_state[6], int width, const int32_t* rows, int n_rows,
                           uint32_t* scratch_w, uint32_t* scratch_mats, uint32_t* rng, hipStream_t stream) {
    if (width <= 0 || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_rng_columns, dim3((width + 63) / 64), dim3(64), 0, stream, jumps, seed_state[0], seed_state[1],
                       seed_state[2], seed_state[3], seed_state[4], width, scratch_w);
    hipLaunchKernelGGL(k_rng_rowmats, dim3(n_rows), dim3(192), 0, stream, jumps, rows, scratch_mats);
    hipLaunchKernelGGL(k_rng_pixels, dim3((width + 255) / 256, n_rows), dim3(256), 0, stream, scratch_mats, scratch_w,
                       width, n_rows, seed_state[5], rng);
    return hipGetLastError();
}
}  // namespace cpt
