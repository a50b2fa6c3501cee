// cpt_antialias_capi.cpp — the C-ABI's antialiased presentation (include/cpt.h):
// cpt_aa_coverage and its read-out, cpt_present_aa, their timing and the host-only hooks on the
// same arithmetic.  The kernels are cpt_antialias.hip's; the definition is cpt_antialias.hpp's on
// both sides.  The G-buffer is cpt_gbuffer's and the present plane cpt_present's, so their
// read-outs serve these calls too.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "cpt_antialias.hpp"
#include "cpt_context.hpp"

using namespace cpt::ctx;
namespace aa = cpt::antialias;
namespace prs = cpt::present;

namespace {

// cpt_present_host's thresholds (cpt_capi_present.cpp holds the host's one copy)
const float* srgb_thresholds() {
    static const struct Table {
        float t[cpt::PRESENT_SRGB_N];
        Table() { cpt_present_srgb_thresholds_host(t); }
    } table;
    return table.t;
}

bool coverage_args_ok(int samples, float normal_cos) { return aa::samples_ok(samples) && aa::normal_cos_ok(normal_cos); }

// RayGen's view of a camera (fill_params' copy), for a W x H image.
cpt::CamK cam_of(const cpt_camera& cam, int W, int H) {
    cpt::CamK k;
    std::memset(&k, 0, sizeof(k));
    for (int a = 0; a < 3; ++a) {
        k.origin[a] = (&cam.origin.x)[a];
        k.u[a] = (&cam.u.x)[a];
        k.v[a] = (&cam.v.x)[a];
        k.top_left[a] = (&cam.top_left_corner.x)[a];
        k.horizontal[a] = (&cam.horizontal.x)[a];
        k.vertical[a] = (&cam.vertical.x)[a];
    }
    k.lens_radius = cam.lens_radius;
    k.width = W;
    k.height = H;
    k.inv_w = 1.0 / (double)(float)W;
    k.inv_h = 1.0 / (double)(float)H;
    return k;
}

// The host hooks' source plane, as cpt_present_host reads it.
struct FetchHost {
    int source;
    const float* src;
    void operator()(size_t q, float s4[4]) const { prs::host_pixel(source, src, q, s4); }
};

}  // namespace

extern "C" {

int cpt_aa_coverage(cpt_ctx* c, const cpt_camera* cam, uint32_t flags, int samples, float normal_cos) {
    if (!c || !cam) return c ? fail(c, CPT_ERR_INVALID_ARG, "cpt_aa_coverage: camera is NULL") : CPT_ERR_INVALID_ARG;
    if (!coverage_args_ok(samples, normal_cos))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_aa_coverage: samples %d (2 or 4), normal_cos %g (-1..1)", samples, (double)normal_cos);
    if (int rc = walk_flags_only(c, "cpt_aa_coverage", flags)) return rc;
    if (!c->scene_set) return fail(c, CPT_ERR_STATE, "cpt_aa_coverage: cpt_set_scene first");
    if (int rc = require_full_frame(c, "cpt_aa_coverage")) return rc;
    if (cam->width != c->width || cam->height != c->height)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_aa_coverage: camera %dx%d vs frame %dx%d", cam->width, cam->height, c->width, c->height);
    CPT_REFUSE_PENDING(c, "cpt_aa_coverage");
    HIP_TRY(c, hipSetDevice(c->device));
    AntialiasState& a = c->frame.antialias;
    const size_t npix = c->npix();
    // all device memory first: nothing is allocated between the G-buffer's trace and the kernels
    if (int rc = ensure_all(c, a.d_cov, npix, a.d_list, npix, a.d_count, 1)) return rc;
    if (int rc = cpt_gbuffer(c, cam, flags)) return rc;   // the frame's G-buffer at `cam`: the documented side effect
    const GBufferState& g = c->frame.gbuffer;
    cpt::KParams p;
    fill_params(c, cam, 0, 0, flags, p);
    hipStream_t s = c->stream();
    if (int rc = c->t_aa.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_aa_edges(g.d_id, g.d_normal, c->width, c->height, samples, normal_cos, a.d_cov, a.d_list, a.d_count, s));
    HIP_TRY(c, cpt::launch_aa_coverage(p, c->d_rank_obj, g.d_id, g.d_normal, samples, normal_cos, a.d_list, a.d_count, a.d_cov, c->grid, s));
    if (int rc = c->t_aa.end(c, s)) return rc;
    a.samples = samples;
    return CPT_OK;
}

int cpt_read_aa_coverage(cpt_ctx* c, uint8_t* counts9, uint8_t* flags, size_t capacity_pixels) {
    if (!c) return CPT_ERR_INVALID_ARG;
    const AntialiasState& a = c->frame.antialias;
    if (!c->frame.set || a.samples == 0) return fail(c, CPT_ERR_STATE, "cpt_read_aa_coverage: cpt_aa_coverage first");
    const size_t n = c->npix();
    if (capacity_pixels < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_aa_coverage: %zu < %zu pixels", capacity_pixels, n);
    if (int rc = sync_checked(c)) return rc;
    std::vector<uint4> words(n);
    if (int rc = read_back(c, words.data(), a.d_cov, n)) return rc;
    for (size_t i = 0; i < n; ++i) {
        const aa::Coverage v = aa::unpack(words[i]);
        if (counts9)
            for (int k = 0; k < 9; ++k) counts9[9 * i + k] = (uint8_t)v.c[k];
        if (flags) flags[i] = (uint8_t)v.flags;
    }
    return CPT_OK;
}

int cpt_present_aa(cpt_ctx* c, int source, int tone, float white, int transfer, uint8_t* bgra_host) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!prs::args_ok(source, tone, white, transfer))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_present_aa: source %d, tone %d, white %g (> 0), transfer %d", source, tone, (double)white,
                    transfer);
    const float4* src = nullptr;
    if (int rc = present_source(c, "cpt_present_aa", source, &src)) return rc;
    const AntialiasState& a = c->frame.antialias;
    if (a.samples == 0) return fail(c, CPT_ERR_STATE, "cpt_present_aa: no coverage (cpt_aa_coverage first)");
    if (int rc = present_state(c)) return rc;
    PresentState& p = c->frame.present;
    hipStream_t s = c->stream();
    const size_t npix = c->npix();
    if (int rc = c->t_present.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_present_aa(src, a.d_cov, c->width, c->height, a.samples, source, tone, white, transfer, p.d_words, p.d_bgra, s));
    if (int rc = c->t_present.end(c, s)) return rc;
    p.presented = true;
    if (bgra_host && npix) HIP_TRY(c, hipMemcpyAsync(bgra_host, p.d_bgra, npix * 4, hipMemcpyDeviceToHost, s));
    return CPT_OK;
}

int cpt_last_aa_ms(cpt_ctx* c, float* ms) { return last_span_ms(c, &cpt_ctx::t_aa, ms, "cpt_last_aa_ms: no cpt_aa_coverage yet"); }

int cpt_aa_rays_host(const cpt_camera* cam, int W, int H, int samples, int x, int y, float* origin3, float* dir3) {
    if (!cam || W <= 0 || H <= 0 || !aa::samples_ok(samples) || x < 0 || x >= W || y < 0 || y >= H || !origin3 || !dir3)
        return CPT_ERR_INVALID_ARG;
    const cpt::CamK k = cam_of(*cam, W, H);
    for (int s = 0; s < samples * samples; ++s) aa::sub_ray(k, samples, x, y, s, origin3 + 3 * s, dir3 + 3 * s);
    return CPT_OK;
}

int cpt_aa_coverage_host(int W, int H, int samples, float normal_cos, const int32_t* id, const float* normal3, const int32_t* sub_id,
                         const float* sub_normal3, uint8_t* counts9, uint8_t* flags) {
    if (W <= 0 || H <= 0 || !coverage_args_ok(samples, normal_cos) || !id || !normal3 || !sub_id || !sub_normal3 || !counts9 || !flags)
        return CPT_ERR_INVALID_ARG;
    const int s2 = samples * samples;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            aa::Coverage v{};
            if (!aa::is_edge(W, H, x, y, id, normal3, normal_cos)) {
                v.c[aa::SELF] = (uint32_t)s2;
            } else {
                v.flags = aa::FLAG_EDGE;
                for (int s = 0; s < s2; ++s) {
                    const int k = aa::attribute(W, H, x, y, samples, s, sub_id[p * s2 + s], sub_normal3 + 3 * (p * s2 + s), id, normal3,
                                                normal_cos);
                    if (k < 0) v.flags |= aa::FLAG_UNMATCHED;
                    ++v.c[k < 0 ? aa::SELF : k];
                }
            }
            for (int k = 0; k < 9; ++k) counts9[9 * p + k] = (uint8_t)v.c[k];
            flags[p] = (uint8_t)v.flags;
        }
    return CPT_OK;
}

int cpt_present_aa_host(int W, int H, int samples, int source, const float* src, const uint8_t* counts9, float exposure, int tone,
                        float white, int transfer, uint8_t* bgra) {
    if (W <= 0 || H <= 0 || !aa::samples_ok(samples) || !src || !counts9 || !bgra || !prs::args_ok(source, tone, white, transfer))
        return CPT_ERR_INVALID_ARG;
    const FetchHost fetch{source, src};
    // a count on a pixel outside the frame has no source
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int k = 0; k < 9; ++k) {
                const int qx = x + k % 3 - 1, qy = y + k / 3 - 1;
                if (counts9[9 * ((size_t)y * W + x) + k] && (qx < 0 || qx >= W || qy < 0 || qy >= H)) return CPT_ERR_INVALID_ARG;
            }
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            aa::Coverage v{};
            for (int k = 0; k < 9; ++k) v.c[k] = counts9[9 * p + k];
            const uint32_t w = aa::pixel_word(fetch, W, H, x, y, v, samples, source, exposure, tone, white, transfer, srgb_thresholds());
            for (int b = 0; b < 4; ++b) bgra[4 * p + b] = (uint8_t)(w >> (8 * b));
        }
    return CPT_OK;
}

}  // extern "C"
