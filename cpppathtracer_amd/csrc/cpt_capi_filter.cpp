// cpt_capi_filter.cpp — the C-ABI's variance-guided a-trous filter of an adaptive render's final
// frame (include/cpt.h): cpt_filter_frame and its read-outs, the moments'
// checkpoint pair, and the host-only hooks on the filter's arithmetic; and the same filter for frames
// without moments (§25): cpt_filter_frame_spatial and its two host hooks.  The kernels are
// cpt_filter.hip's; the arithmetic is cpt_filter.hpp's on both sides.
#include <hip/hip_runtime.h>

#include <vector>

#include "cpt_context.hpp"
#include "cpt_filter.hpp"

using namespace cpt::ctx;
namespace flt = cpt::filter;

namespace {

bool args_ok(float sigma_l, int sharpness_log2) {
    return flt::finite(sigma_l) && sigma_l >= 0.f && sharpness_log2 >= 0 && sharpness_log2 <= flt::MAX_SHARPNESS_LOG2;
}

// cpt_filter_frame and, `spatial`, cpt_filter_frame_spatial: they differ in the guides they need
// (the moments and the frame's normals, or the G-buffer) and in the kernels those feed.
int filter_frame(cpt_ctx* c, const char* who, bool spatial, int levels, float sigma_l, int normal_sharpness_log2) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (levels < 0 || levels > flt::MAX_LEVELS || !args_ok(sigma_l, normal_sharpness_log2))
        return fail(c, CPT_ERR_INVALID_ARG, "%s: levels %d (0..8), sigma_l %g (finite, >= 0), normal_sharpness_log2 %d (0..10)", who,
                    levels, (double)sigma_l, normal_sharpness_log2);
    CPT_REFUSE_PENDING(c, who);
    if (int rc = require_full_frame(c, who)) return rc;
    Frame& f = c->frame;
    const GBufferState& g = f.gbuffer;
    const size_t npix = c->npix();
    if (spatial) {
        if (!g.valid || g.d_id.capacity() < npix || g.d_normal.capacity() < 3 * npix)
            return fail(c, CPT_ERR_STATE, "%s: no G-buffer (cpt_gbuffer, a reprojection or cpt_write_gbuffer first)", who);
    } else {
        if (!f.adaptive.has_result(npix))
            return fail(c, CPT_ERR_STATE, "%s: no moments (cpt_render_adaptive or cpt_write_moments first)", who);
        if (f.d_normal.capacity() < 3 * npix)
            return fail(c, CPT_ERR_STATE, "%s: no normals (render with CPT_RENDER_AUX or cpt_write_aux first)", who);
    }
    HIP_TRY(c, hipSetDevice(c->device));
    FilterState& ft = f.filter;
    if (int rc = ensure_all(c, ft.d_plane[0], npix, ft.d_plane[1], npix, ft.d_ok, npix)) return rc;
    ft.result = -1;
    hipStream_t s = c->stream();
    const float sigma2 = sigma_l * sigma_l;
    if (int rc = c->t_filter.begin(c, s)) return rc;
    if (spatial)
        HIP_TRY(c, cpt::launch_filter_prepare_spatial(f.d_accum, g.d_id, g.d_normal, c->width, c->height, normal_sharpness_log2,
                                                      ft.d_plane[0], ft.d_ok, s));
    else
        HIP_TRY(c, cpt::launch_filter_prepare(f.d_accum, f.adaptive.d_stat, npix, ft.d_plane[0], ft.d_ok, s));
    for (int l = 0; l < levels; ++l) {
        if (spatial)
            HIP_TRY(c, cpt::launch_filter_level_id(ft.d_plane[l & 1], g.d_normal, g.d_id, ft.d_ok, ft.d_plane[(l + 1) & 1], c->width,
                                                  c->height, 1 << l, sigma2, normal_sharpness_log2, s));
        else
            HIP_TRY(c, cpt::launch_filter_level(ft.d_plane[l & 1], f.d_normal, ft.d_ok, ft.d_plane[(l + 1) & 1], c->width, c->height,
                                               1 << l, sigma2, normal_sharpness_log2, s));
    }
    if (int rc = c->t_filter.end(c, s)) return rc;
    ft.result = levels & 1;
    return CPT_OK;
}

}  // namespace

extern "C" {

int cpt_filter_frame(cpt_ctx* c, int levels, float sigma_l, int normal_sharpness_log2) {
    return filter_frame(c, "cpt_filter_frame", false, levels, sigma_l, normal_sharpness_log2);
}

int cpt_filter_frame_spatial(cpt_ctx* c, int levels, float sigma_l, int normal_sharpness_log2) {
    return filter_frame(c, "cpt_filter_frame_spatial", true, levels, sigma_l, normal_sharpness_log2);
}

int cpt_read_filtered(cpt_ctx* c, float* rgb, float* variance, size_t capacity_pixels) {
    if (!c) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.set || f.filter.result < 0) return fail(c, CPT_ERR_STATE, "cpt_read_filtered: cpt_filter_frame first");
    const size_t n = c->npix();
    if (capacity_pixels < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_filtered: %zu < %zu pixels", capacity_pixels, n);
    if (int rc = sync_checked(c)) return rc;
    std::vector<float> plane(4 * n);
    if (int rc = read_back(c, plane.data(), f.filter.d_plane[f.filter.result], n)) return rc;
    for (size_t i = 0; i < n; ++i) {
        if (rgb) {
            rgb[3 * i] = plane[4 * i];
            rgb[3 * i + 1] = plane[4 * i + 1];
            rgb[3 * i + 2] = plane[4 * i + 2];
        }
        if (variance) variance[i] = plane[4 * i + 3];
    }
    return CPT_OK;
}

int cpt_last_filter_ms(cpt_ctx* c, float* ms) {
    return last_span_ms(c, &cpt_ctx::t_filter, ms, "cpt_last_filter_ms: no cpt_filter_frame yet");
}

int cpt_read_moments(cpt_ctx* c, float* planar4, size_t capacity) {
    if (!c || !planar4) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.set || !f.adaptive.done) return fail(c, CPT_ERR_STATE, "cpt_read_moments: cpt_render_adaptive or cpt_write_moments first");
    const size_t n = 4 * c->npix();
    if (capacity < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_moments: %zu < %zu floats", capacity, n);
    if (int rc = sync_checked(c)) return rc;
    return read_back(c, planar4, f.adaptive.d_stat, n);
}

int cpt_write_moments(cpt_ctx* c, const float* planar4, size_t count) {
    if (!c || !planar4) return CPT_ERR_INVALID_ARG;
    Frame& f = c->frame;
    if (!f.set) return fail(c, CPT_ERR_STATE, "cpt_write_moments: no frame");
    const size_t n = 4 * c->npix();
    if (count < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_write_moments: %zu < %zu floats", count, n);
    if (int rc = drain(c)) return rc;
    if (int rc = f.adaptive.d_stat.ensure(c, n)) return rc;
    if (int rc = write_in(c, f.adaptive.d_stat, planar4, n)) return rc;
    f.adaptive.adopt_result();
    return CPT_OK;
}

int cpt_filter_prepare_host(size_t npix, const float* accum_rgba, const float* moments_planar4, float* out_rgbv,
                            uint8_t* out_valid) {
    if (!accum_rgba || !moments_planar4 || !out_rgbv || !out_valid) return CPT_ERR_INVALID_ARG;
    for (size_t i = 0; i < npix; ++i) {
        flt::Px c;
        const float* S = accum_rgba + 4 * i;
        out_valid[i] = flt::prepare(S[0], S[1], S[2], S[3], moments_planar4[i], moments_planar4[npix + i],
                                    moments_planar4[2 * npix + i], c)
                           ? 1
                           : 0;
        out_rgbv[4 * i] = c.r;
        out_rgbv[4 * i + 1] = c.g;
        out_rgbv[4 * i + 2] = c.b;
        out_rgbv[4 * i + 3] = c.v;
    }
    return CPT_OK;
}

int cpt_filter_level_host(int width, int height, int step, const float* in_rgbv, const float* normal3, const uint8_t* valid,
                          float sigma_l, int normal_sharpness_log2, float* out_rgbv) {
    if (width <= 0 || height <= 0 || step < 1 || step > (1 << (flt::MAX_LEVELS - 1)) || !in_rgbv || !normal3 || !valid ||
        !out_rgbv || in_rgbv == out_rgbv || !args_ok(sigma_l, normal_sharpness_log2))
        return CPT_ERR_INVALID_ARG;
    const flt::PlaneSrc src{reinterpret_cast<const flt::Px*>(in_rgbv), normal3, valid, width};
    flt::Px* out = reinterpret_cast<flt::Px*>(out_rgbv);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x)
            out[(size_t)y * width + x] = src.valid(x, y) ? flt::level_pixel(src, x, y, width, height, step, sigma_l * sigma_l,
                                                                            normal_sharpness_log2)
                                                         : src.px(x, y);
    return CPT_OK;
}

int cpt_filter_prepare_spatial_host(int width, int height, const float* accum_rgba, const int32_t* id, const float* normal3,
                                    int normal_sharpness_log2, float* out_rgbv, uint8_t* out_valid) {
    if (width <= 0 || height <= 0 || !accum_rgba || !id || !normal3 || !out_rgbv || !out_valid || normal_sharpness_log2 < 0 ||
        normal_sharpness_log2 > flt::MAX_SHARPNESS_LOG2)
        return CPT_ERR_INVALID_ARG;
    const size_t npix = (size_t)width * height;
    std::vector<float> l(npix), n(npix);
    std::vector<uint8_t> b(npix);
    for (size_t i = 0; i < npix; ++i) {
        const float* S = accum_rgba + 4 * i;
        flt::Px c;
        b[i] = flt::spatial_base(S[0], S[1], S[2], S[3], c) ? 1 : 0;
        l[i] = flt::luma(c);
        n[i] = S[3];
    }
    const flt::SpatialPlaneSrc src{l.data(), n.data(), b.data(), id, normal3, width};
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x) {
            const size_t i = (size_t)y * width + x;
            const float* S = accum_rgba + 4 * i;
            flt::Px c;
            out_valid[i] = flt::prepare_spatial(src, x, y, width, height, S[0], S[1], S[2], S[3], normal_sharpness_log2, c) ? 1 : 0;
            out_rgbv[4 * i] = c.r;
            out_rgbv[4 * i + 1] = c.g;
            out_rgbv[4 * i + 2] = c.b;
            out_rgbv[4 * i + 3] = c.v;
        }
    return CPT_OK;
}

int cpt_filter_level_id_host(int width, int height, int step, const float* in_rgbv, const float* normal3, const int32_t* id,
                             const uint8_t* valid, float sigma_l, int normal_sharpness_log2, float* out_rgbv) {
    if (width <= 0 || height <= 0 || step < 1 || step > (1 << (flt::MAX_LEVELS - 1)) || !in_rgbv || !normal3 || !id || !valid ||
        !out_rgbv || in_rgbv == out_rgbv || !args_ok(sigma_l, normal_sharpness_log2))
        return CPT_ERR_INVALID_ARG;
    const flt::PlaneIdSrc src{{reinterpret_cast<const flt::Px*>(in_rgbv), normal3, valid, width}, id};
    flt::Px* out = reinterpret_cast<flt::Px*>(out_rgbv);
    for (int y = 0; y < height; ++y)
        for (int x = 0; x < width; ++x)
            out[(size_t)y * width + x] =
                src.valid(x, y) ? flt::level_pixel<flt::PlaneIdSrc, true>(src, x, y, width, height, step, sigma_l * sigma_l,
                                                                          normal_sharpness_log2)
                                : src.px(x, y);
    return CPT_OK;
}

}  // extern "C"
