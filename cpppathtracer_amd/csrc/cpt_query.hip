// cpt_query.hip — first-hit queries outside the integrator (cpt_gbuffer, cpt_trace_rays, cpt_pick;
// DESIGN.md §20): one ray per lane through SceneBVH::TraceRay (bvh.cu:167-205) as the integrator's
// kernels walk it, and per ray the object hit, its distance, normal and albedo.  The reference has
// no counterpart: its only first-hit data are the normal and the constant depth SamplePixel writes
// (path_tracer.cu:172-174).
//
//   k_ray_query<LDST, CAMERA>   CAMERA: the frame's pixels, each with RayGen's ray at zero lens
//                               offset; else rays from device arrays.  No RNG state is touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpt_path.hpp"
#include "cpt_query.hpp"

namespace cpt {

// LDST: the wide walk on the workgroup's LDS image of the tree, in the megakernel's LDS block shape
// (LDS_BLOCK lanes, one workgroup per CU: the image and the 16-bit walk stacks, CPT_WSTACK entries
// per lane, take 120 KB of the CU's 160 KB); else WIDE_LANES blocks and the binary walks.
template <bool LDST> constexpr int query_block() { return LDST ? LDS_BLOCK : WIDE_LANES; }

// A plain grid, one ray per lane.  CAMERA: wave w of the grid is 8x8 tile w of the frame's rows
// (cpt_tiles.hpp), so a wave's rays are coherent; else lane i of the grid is ray i.  A lane
// without a ray (an edge tile's pixels outside the frame, the last wave past the ray list) leaves
// after the image is staged, as k_wf_extend's lanes past its queue do: the wide walk's wave-wide
// leaf rounds are ballots over the lanes still there, so it counts in none of them.
template <bool LDST, bool CAMERA>
__global__ void __launch_bounds__(query_block<LDST>()) k_ray_query(const KParams p, const int32_t* __restrict__ rank_obj,
                                                                   const QueryRays in, const QueryPixels px,
                                                                   const QueryOut out) {
    constexpr int BLK = query_block<LDST>();
    __shared__ uint4 s_tree[LDST ? LDS_TREE_NODES * 7 : 1];
    if (LDST) {
        stage_wide_tree<BLK>(s_tree, p);
    }
    const uint32_t i = blockIdx.x * (uint32_t)BLK + threadIdx.x;
    size_t slot;
    Ray ray;
    if (CAMERA) {
        if (px.pick_x >= 0) {
            if (i != 0) return;
            slot = 0;
            ray = ray_gen_centre(p.cam, px.pick_x, px.pick_y);
        } else {
            const TileGrid grid{p.width, p.n_rows};
            int x = 0, ri = 0;
            if ((i >> 6) >= (uint32_t)grid.count() || !grid.pixel(i >> 6, i & 63, x, ri)) return;
            slot = (size_t)ri * p.width + x;
            ray = ray_gen_centre(p.cam, x, p.rows[ri]);
        }
    } else {
        if (i >= in.n) return;
        slot = i;
        ray.o = mk(in.origin3[3 * slot], in.origin3[3 * slot + 1], in.origin3[3 * slot + 2]);
        ray.d = mk(in.dir3[3 * slot], in.dir3[3 * slot + 1], in.dir3[3 * slot + 2]);   // as given (TraceRay)
        ray.tmin = in.tmin ? in.tmin[slot] : 0.f;
        ray.tmax = DEFAULT_RAY_TMAX;
    }
    const RayK rk = make_rayk(ray);
    const bool finite = ray_is_finite(ray);
    Hit h;
    Winner win{-1, -1, DEFAULT_RAY_TMAX};
    Counters cnt{};
    bool hit;
    if (LDST) hit = trace_segment<false, BLK, true>(p, rk, finite, h, win, cnt, s_tree);
    else hit = trace_segment<false>(p, rk, finite, h, win, cnt);
    // a miss: -1, the ray's tmax, the integrator's miss normal -dir (path_tracer.cu:117-122), black
    const v3 n = hit ? h.normal : -ray.d;
    out.id[slot] = hit ? rank_obj[win.rank] : -1;
    out.t[slot] = hit ? win.t : DEFAULT_RAY_TMAX;
    out.normal3[3 * slot] = n.x;
    out.normal3[3 * slot + 1] = n.y;
    out.normal3[3 * slot + 2] = n.z;
    if (CAMERA && out.albedo3) {
        v3 kd = mk1(0.f);
        if (hit) {
            const Mat m = p.mats[win.code >> 2];
            kd = mk(m.att_x, m.att_y, m.att_z);   // GetKd(0, 0), prepared (k_prepare_materials)
        }
        out.albedo3[3 * slot] = kd.x;
        out.albedo3[3 * slot + 1] = kd.y;
        out.albedo3[3 * slot + 2] = kd.z;
    }
}

template <bool LDST>
static hipError_t launch_query_t(const KParams& p, const int32_t* rank_obj, const QueryRays* rays, QueryPixels px,
                                 const QueryOut& out, hipStream_t stream) {
    constexpr int block = query_block<LDST>();
    // lanes: the rays, or a tile's 64 lanes per 8x8 tile of the frame (one lane for a single pixel)
    const size_t lanes = rays ? rays->n : (px.pick_x >= 0 ? 1 : (size_t)TileGrid{p.width, p.n_rows}.count() * 64);
    if (lanes == 0) return hipSuccess;
    const dim3 grid((unsigned)((lanes + block - 1) / block));
    if (rays) hipLaunchKernelGGL((k_ray_query<LDST, false>), grid, dim3(block), 0, stream, p, rank_obj, *rays, px, out);
    else hipLaunchKernelGGL((k_ray_query<LDST, true>), grid, dim3(block), 0, stream, p, rank_obj, QueryRays{}, px, out);
    return hipGetLastError();
}

hipError_t launch_ray_query(const KParams& p, const int32_t* rank_obj, const QueryRays* rays, QueryPixels pixels,
                            const QueryOut& out, hipStream_t stream) {
    return use_lds_tree(p) ? launch_query_t<true>(p, rank_obj, rays, pixels, out, stream)
               : launch_query_t<false>(p, rank_obj, rays, pixels, out, stream);
}

}  // namespace cpt
