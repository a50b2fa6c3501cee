// cpt_bloom_capi.cpp — the C-ABI's bloom for presented frames (include/cpt.h):
// cpt_bloom and its read-out, cpt_present_bloom, the timing and the host-only hooks on the same
// arithmetic.  The kernels are cpt_bloom.hip's; the definition is cpt_bloom.hpp's on both sides.
// The present plane and the exposure word are cpt_present's, so its read-outs serve these calls too.
#include <hip/hip_runtime.h>

#include <vector>

#include "cpt_bloom.hpp"
#include "cpt_context.hpp"

using namespace cpt::ctx;
namespace blm = cpt::bloom;
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

bool build_args_ok(int source, float threshold, int levels) {
    return prs::source_ok(source) && blm::amount_ok(threshold) && blm::levels_ok(levels);
}

// a host level: [h][w][3] floats
struct FetchHost {
    const float* t;
    int w;
    blm::Rgb operator()(int x, int y) const {
        const float* v = t + 3 * ((size_t)y * w + x);
        return blm::Rgb{v[0], v[1], v[2]};
    }
};

void store(std::vector<float>& level, size_t i, const blm::Rgb& v) {
    level[3 * i] = v.r;
    level[3 * i + 1] = v.g;
    level[3 * i + 2] = v.b;
}

// The exposed pixels x ([H][W][3]) and U_1..U_levels (U[0] is left empty) of a host source plane.
void build_host(int W, int H, int source, const float* src, float exposure, float threshold, int levels, std::vector<float>& x,
                std::vector<std::vector<float>>& U) {
    const blm::Pyramid p = blm::pyramid_of(W, H);
    const size_t npix = (size_t)W * H;
    x.resize(3 * npix);
    std::vector<float> b(3 * npix);
    for (size_t i = 0; i < npix; ++i) {
        float S[4];
        prs::host_pixel(source, src, i, S);
        const blm::Rgb xi = blm::exposed(source, S[0], S[1], S[2], S[3], exposure);
        store(x, i, xi);
        store(b, i, blm::bright(xi, threshold));
    }
    U.assign(levels + 1, {});
    for (int l = 1; l <= levels; ++l) {
        const FetchHost fine{l == 1 ? b.data() : U[l - 1].data(), p.w[l - 1]};
        U[l].resize(3 * (size_t)p.w[l] * p.h[l]);
        for (int Y = 0; Y < p.h[l]; ++Y)
            for (int X = 0; X < p.w[l]; ++X) store(U[l], (size_t)Y * p.w[l] + X, blm::down(fine, p.w[l - 1], p.h[l - 1], X, Y));
    }
    for (int l = levels - 1; l >= 1; --l) {
        const FetchHost coarse{U[l + 1].data(), p.w[l + 1]};
        for (int y = 0; y < p.h[l]; ++y)
            for (int xx = 0; xx < p.w[l]; ++xx) {
                const size_t i = (size_t)y * p.w[l] + xx;
                store(U[l], i, blm::sum(FetchHost{U[l].data(), p.w[l]}(xx, y), blm::up(coarse, p.w[l + 1], p.h[l + 1], xx, y)));
            }
    }
}

}  // namespace

extern "C" {

int cpt_bloom(cpt_ctx* c, int source, float threshold, int levels) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!build_args_ok(source, threshold, levels))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_bloom: source %d, threshold %g (finite, >= 0), levels %d (1..%d)", source, (double)threshold,
                    levels, blm::MAX_LEVELS);
    const float4* src = nullptr;
    if (int rc = present_source(c, "cpt_bloom", source, &src)) return rc;
    if (int rc = require_full_frame(c, "cpt_bloom")) return rc;
    // all device memory first (room for every level, so that a later call with more allocates
    // nothing), then the present state, whose first call initialises the exposure word on the stream
    HIP_TRY(c, hipSetDevice(c->device));
    BloomState& b = c->frame.bloom;
    const blm::Pyramid p = blm::pyramid_of(c->width, c->height);
    if (int rc = b.d_pyramid.ensure(c, p.off[blm::MAX_LEVELS + 1])) return rc;
    if (int rc = present_state(c)) return rc;
    hipStream_t s = c->stream();
    if (int rc = c->t_bloom.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_bloom(src, c->width, c->height, source, threshold, levels, c->frame.present.d_words, b.d_pyramid, s));
    if (int rc = c->t_bloom.end(c, s)) return rc;
    b.levels = levels;
    return CPT_OK;
}

int cpt_present_bloom(cpt_ctx* c, int source, int tone, float white, int transfer, float intensity, uint8_t* bgra_host) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!prs::args_ok(source, tone, white, transfer) || !blm::amount_ok(intensity))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_present_bloom: source %d, tone %d, white %g (> 0), transfer %d, intensity %g (finite, >= 0)",
                    source, tone, (double)white, transfer, (double)intensity);
    const float4* src = nullptr;
    if (int rc = present_source(c, "cpt_present_bloom", source, &src)) return rc;
    if (int rc = require_full_frame(c, "cpt_present_bloom")) return rc;
    const BloomState& b = c->frame.bloom;
    if (b.levels == 0) return fail(c, CPT_ERR_STATE, "cpt_present_bloom: no pyramid (cpt_bloom first)");
    if (int rc = present_state(c)) return rc;
    PresentState& p = c->frame.present;
    hipStream_t s = c->stream();
    const size_t npix = c->npix();
    if (int rc = c->t_present.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_present_bloom(src, b.d_pyramid, c->width, c->height, source, tone, white, transfer, intensity, p.d_words,
                                         p.d_bgra, s));
    if (int rc = c->t_present.end(c, s)) return rc;
    p.presented = true;
    if (bgra_host && npix) HIP_TRY(c, hipMemcpyAsync(bgra_host, p.d_bgra, npix * 4, hipMemcpyDeviceToHost, s));
    return CPT_OK;
}

int cpt_read_bloom(cpt_ctx* c, int level, float* rgb, size_t capacity_texels) {
    if (!c || !rgb) return CPT_ERR_INVALID_ARG;
    const BloomState& b = c->frame.bloom;
    if (!c->frame.set || b.levels == 0) return fail(c, CPT_ERR_STATE, "cpt_read_bloom: cpt_bloom first");
    if (level < 1 || level > b.levels) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_bloom: level %d (1..%d)", level, b.levels);
    const blm::Pyramid p = blm::pyramid_of(c->width, c->height);
    const size_t n = (size_t)p.w[level] * p.h[level];
    if (capacity_texels < n) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_bloom: %zu < %zu texels", capacity_texels, n);
    if (int rc = sync_checked(c)) return rc;
    std::vector<float4> texels(n);
    if (int rc = read_back(c, texels.data(), b.d_pyramid, n, p.off[level])) return rc;
    for (size_t i = 0; i < n; ++i) {
        rgb[3 * i] = texels[i].x;
        rgb[3 * i + 1] = texels[i].y;
        rgb[3 * i + 2] = texels[i].z;
    }
    return CPT_OK;
}

int cpt_last_bloom_ms(cpt_ctx* c, float* ms) { return last_span_ms(c, &cpt_ctx::t_bloom, ms, "cpt_last_bloom_ms: no cpt_bloom yet"); }

int cpt_bloom_host(int W, int H, int source, const float* src, float exposure, float threshold, int levels, int level, float* rgb) {
    if (W <= 0 || H <= 0 || !src || !rgb || !build_args_ok(source, threshold, levels) || level < 1 || level > levels)
        return CPT_ERR_INVALID_ARG;
    std::vector<float> x;
    std::vector<std::vector<float>> U;
    build_host(W, H, source, src, exposure, threshold, levels, x, U);
    for (size_t i = 0; i < U[level].size(); ++i) rgb[i] = U[level][i];
    return CPT_OK;
}

int cpt_present_bloom_host(int W, int H, int source, const float* src, float exposure, float threshold, int levels, float intensity,
                           int tone, float white, int transfer, uint8_t* bgra) {
    if (W <= 0 || H <= 0 || !src || !bgra || !build_args_ok(source, threshold, levels) || !blm::amount_ok(intensity) ||
        !prs::args_ok(source, tone, white, transfer))
        return CPT_ERR_INVALID_ARG;
    std::vector<float> x;
    std::vector<std::vector<float>> U;
    build_host(W, H, source, src, exposure, threshold, levels, x, U);
    const int w1 = (W + 1) / 2, h1 = (H + 1) / 2;
    const FetchHost glow{U[1].data(), w1};
    for (int y = 0; y < H; ++y)
        for (int xx = 0; xx < W; ++xx) {
            const size_t i = (size_t)y * W + xx;
            const uint32_t w = blm::pixel_word(blm::Rgb{x[3 * i], x[3 * i + 1], x[3 * i + 2]}, blm::up(glow, w1, h1, xx, y), intensity, tone,
                                               white, transfer, srgb_thresholds());
            for (int k = 0; k < 4; ++k) bgra[4 * i + k] = (uint8_t)(w >> (8 * k));
        }
    return CPT_OK;
}

}  // extern "C"
