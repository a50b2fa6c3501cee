// cpt_capi_gather.cpp — the C-ABI's row-tile gather: the rows `src` rendered,
// placed into `dst`'s frame at the same global rows by one stitch kernel on dst's stream, ordered
// by events (no host wait; see cpt_gather_rows below for the three ways the stitch reaches src's
// buffers).
#include <hip/hip_runtime.h>

#include <mutex>
#include <utility>
#include <vector>

#include "cpt_context.hpp"

using namespace cpt::ctx;

namespace {
// Peer access from `dev` to `peer`'s memory, enabled once per ordered pair for the process.
// Returns false when the pair has no peer path (the gather then stages through a peer copy).
bool ensure_peer_access(int dev, int peer) {
    static std::mutex mu;
    static std::vector<std::pair<std::pair<int, int>, bool>> known;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& k : known)
        if (k.first == std::make_pair(dev, peer)) return k.second;
    int can = 0;
    bool ok = hipDeviceCanAccessPeer(&can, dev, peer) == hipSuccess && can;
    if (ok) {
        int cur = 0;
        (void)hipGetDevice(&cur);
        ok = hipSetDevice(dev) == hipSuccess;
        if (ok) {
            const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
            ok = e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled;
            if (!ok) (void)hipGetLastError();   // clear the sticky error
        }
        (void)hipSetDevice(cur);
    }
    known.emplace_back(std::make_pair(dev, peer), ok);
    return ok;
}
}  // namespace

extern "C" {

// The row map of a (dst, src) frame pair lives in a device buffer of dst, uploaded when either
// frame changes (cpt_set_frame bumps frame_gen).  src's work is ordered before the stitch by an
// event (no host wait), and src's later work after it by another, so N gathers queue back to
// back on dst's stream and one synchronisation of dst covers them all.  On two devices the
// stitch kernel reads src's buffers directly over xGMI (peer access, enabled once per pair);
// without a peer path it stages them through hipMemcpyPeerAsync.
int cpt_gather_rows(cpt_ctx* dst, cpt_ctx* src) {
    if (!dst || !src || dst == src) return dst ? fail(dst, CPT_ERR_INVALID_ARG, "cpt_gather_rows: bad contexts") : CPT_ERR_INVALID_ARG;
    if (!dst->frame.set || !src->frame.set) return fail(dst, CPT_ERR_STATE, "cpt_gather_rows: both contexts need a frame");
    if (dst->width != src->width || dst->height != src->height)
        return fail(dst, CPT_ERR_INVALID_ARG, "cpt_gather_rows: frame %dx%d vs %dx%d", dst->width, dst->height, src->width,
                    src->height);
    // a pending adaptive render's rounds still write src's buffers (and would write dst's)
    if (src->frame.adaptive.pending.on || dst->frame.adaptive.pending.on)
        return fail(dst, CPT_ERR_STATE, "cpt_gather_rows: an adaptive render is pending on the %s (cpt_adaptive_step until 0)",
                    src->frame.adaptive.pending.on ? "source" : "destination");
    cpt_ctx::GatherMap* gm = nullptr;
    for (auto& g : dst->gather_maps)
        if (g.src == src) gm = &g;
    if (!gm) {
        dst->gather_maps.push_back(cpt_ctx::GatherMap{});
        gm = &dst->gather_maps.back();
        gm->src = src;
    }
    if (gm->src_gen != src->frame_gen || gm->dst_gen != dst->frame_gen || gm->src_device != src->device) {
        std::vector<int32_t> at(dst->height, -1);   // dst row index of each global row (first occurrence)
        for (int j = dst->n_rows - 1; j >= 0; --j) at[dst->rows_h[j]] = j;
        std::vector<int32_t> map(src->n_rows);
        for (int i = 0; i < src->n_rows; ++i) {
            const int32_t j = at[src->rows_h[i]];
            if (j < 0)
                return fail(dst, CPT_ERR_INVALID_ARG, "cpt_gather_rows: row %d is not in the destination frame", src->rows_h[i]);
            map[i] = j;
        }
        HIP_TRY(dst, hipSetDevice(dst->device));
        // always a fresh buffer: a stitch queued earlier may still read the old one (its release
        // waits for the device, the blocking copy below does not wait for dst's stream)
        gm->d_map.reset();
        if (int rc = gm->d_map.ensure(dst, map.size())) return rc;
        if (int rc = write_in(dst, gm->d_map, map.data(), map.size())) return rc;
        gm->src_gen = src->frame_gen;
        gm->dst_gen = dst->frame_gen;
        gm->src_device = src->device;
        gm->peer = src->device == dst->device || ensure_peer_access(dst->device, src->device);
    }
    const bool staged = !gm->peer || dst->force_staged_gather;
    gm->mode = staged ? CPT_GATHER_STAGED : src->device == dst->device ? CPT_GATHER_SAME_DEVICE : CPT_GATHER_PEER;
    if (src->n_rows == 0) return CPT_OK;
    const size_t npix = src->npix();
    Frame &sf = src->frame, &df = dst->frame;
    const bool aux = sf.d_normal && sf.d_depth;
    // an adaptive result on src: its moment planes travel with its rows
    const bool moments = sf.adaptive.has_result(npix);
    // src's queued work (its render) before the stitch
    HIP_TRY(src, hipSetDevice(src->device));
    HIP_TRY(src, hipEventRecord(src->ev_ready, src->stream()));
    HIP_TRY(dst, hipSetDevice(dst->device));
    hipStream_t s = dst->stream();
    HIP_TRY(dst, hipStreamWaitEvent(s, src->ev_ready, 0));
    const size_t dst_npix = dst->npix();
    if (aux) {
        // rows no source covers read as zero normals and depths
        if (!df.d_normal) {
            if (int rc = df.d_normal.ensure(dst, dst_npix * 3)) return rc;
            HIP_TRY(dst, hipMemsetAsync(df.d_normal, 0, dst_npix * 3 * sizeof(float), s));
        }
        if (!df.d_depth) {
            if (int rc = df.d_depth.ensure(dst, dst_npix)) return rc;
            HIP_TRY(dst, hipMemsetAsync(df.d_depth, 0, dst_npix * sizeof(float), s));
        }
    }
    if (moments) {
        // a destination without an adaptive result of its own starts as pixels before their second
        // batch: m1 = m2 = k = 0 (invalid for the filter) and +inf noise, where no source covers a row
        const bool fresh = !df.adaptive.has_result(dst_npix);
        if (int rc = df.adaptive.d_stat.ensure(dst, 4 * dst_npix)) return rc;
        if (fresh) {
            HIP_TRY(dst, hipMemsetAsync(df.adaptive.d_stat, 0, 3 * dst_npix * sizeof(float), s));
            HIP_TRY(dst, hipMemsetD32Async((hipDeviceptr_t)(df.adaptive.d_stat + 3 * dst_npix), 0x7f800000, dst_npix, s));
        }
        df.adaptive.adopt_result();
    }
    const float4* s_acc = sf.d_accum;
    const float* s_nrm = aux ? sf.d_normal.get() : nullptr;
    const float* s_dep = aux ? sf.d_depth.get() : nullptr;
    const float* s_stat = moments ? sf.adaptive.d_stat.get() : nullptr;
    if (staged) {
        // staging: accumulator (npix float4), then normals (3 npix floats) and depths (npix floats)
        if (int rc = dst->d_gather.ensure(dst, aux ? 2 * npix : npix)) return rc;
        float* st_nrm = reinterpret_cast<float*>(dst->d_gather + npix);
        float* st_dep = st_nrm + 3 * npix;
        HIP_TRY(dst, hipMemcpyPeerAsync(dst->d_gather, dst->device, sf.d_accum, src->device, npix * sizeof(float4), s));
        if (aux) {
            HIP_TRY(dst, hipMemcpyPeerAsync(st_nrm, dst->device, sf.d_normal, src->device, npix * 3 * sizeof(float), s));
            HIP_TRY(dst, hipMemcpyPeerAsync(st_dep, dst->device, sf.d_depth, src->device, npix * sizeof(float), s));
        }
        s_acc = dst->d_gather;
        s_nrm = aux ? st_nrm : nullptr;
        s_dep = aux ? st_dep : nullptr;
        if (moments) {
            // a staging buffer of their own: the layout above is that of a source without moments
            if (int rc = dst->d_gather_stat.ensure(dst, 4 * npix)) return rc;
            HIP_TRY(dst, hipMemcpyPeerAsync(dst->d_gather_stat, dst->device, sf.adaptive.d_stat, src->device,
                                            4 * npix * sizeof(float), s));
            s_stat = dst->d_gather_stat;
        }
    }
    HIP_TRY(dst, cpt::launch_stitch_rows(s_acc, s_nrm, s_dep, gm->d_map, dst->width, src->n_rows, df.d_accum,
                                         df.d_normal, df.d_depth, s));
    if (moments)
        HIP_TRY(dst, cpt::launch_stitch_moments(s_stat, npix, gm->d_map, dst->width, src->n_rows, df.adaptive.d_stat, dst_npix, s));
    // src's later work (a next render into the buffers just read) after the stitch
    HIP_TRY(dst, hipEventRecord(dst->ev_gathered, s));
    HIP_TRY(src, hipSetDevice(src->device));
    HIP_TRY(src, hipStreamWaitEvent(src->stream(), dst->ev_gathered, 0));
    HIP_TRY(dst, hipSetDevice(dst->device));
    return CPT_OK;
}

int cpt_last_gather_mode(cpt_ctx* dst, cpt_ctx* src, int* mode) {
    if (!dst || !src || !mode) return dst ? fail(dst, CPT_ERR_INVALID_ARG, "cpt_last_gather_mode: null argument") : CPT_ERR_INVALID_ARG;
    *mode = -1;
    for (const auto& g : dst->gather_maps)
        if (g.src == src) *mode = g.mode;
    return CPT_OK;
}

int cpt_set_debug_gather(cpt_ctx* c, int force_staged) {
    if (!c) return CPT_ERR_INVALID_ARG;
    c->force_staged_gather = force_staged != 0;
    return CPT_OK;
}

}  // extern "C"
