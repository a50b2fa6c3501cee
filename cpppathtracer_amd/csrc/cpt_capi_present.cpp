// cpt_capi_present.cpp — the C-ABI's presentation of an HDR frame (include/cpt.h):
// the exposure word and its meter, cpt_present and its read-outs, and the host-only hooks on the
// same arithmetic.  The kernels are cpt_present.hip's; the arithmetic is cpt_present.hpp's on both
// sides.
#include <hip/hip_runtime.h>

#include <cstring>
#include <utility>

#include "cpt_context.hpp"
#include "cpt_present.hpp"

using namespace cpt::ctx;
namespace prs = cpt::present;

namespace {

const float SRGB_T[cpt::PRESENT_SRGB_N] = CPT_PRESENT_SRGB_TABLE_INIT;
constexpr size_t EXPOSURE_WORD = prs::HIST_WORDS;

bool meter_args_ok(float key, int permille, float adapt) {
    return cpt::filter::finite(key) && key > 0.f && permille >= 0 && permille <= 1000 && adapt >= 0.f && adapt <= 1.f;
}

}  // namespace

// What every call asks of the context before it writes anything: a frame, no adaptive render
// pending and, for the filtered source, a filter result.  *src: the source plane.
int cpt::ctx::present_source(cpt_ctx* c, const char* who, int source, const float4** src) {
    CPT_REFUSE_PENDING(c, who);
    const Frame& f = c->frame;
    if (!f.set) return fail(c, CPT_ERR_STATE, "%s: no frame (cpt_set_frame first)", who);
    if (source == CPT_PRESENT_FILTERED) {
        if (f.filter.result < 0 || f.filter.d_plane[f.filter.result].capacity() < c->npix())
            return fail(c, CPT_ERR_STATE, "%s: no filter result (cpt_filter_frame or cpt_filter_frame_spatial first)", who);
        if (src) *src = f.filter.d_plane[f.filter.result];
    } else if (src) {
        *src = f.d_accum;
    }
    return CPT_OK;
}

// The present state of the frame, allocated and initialised on the stream at the frame's first
// call: the histogram zero, the exposure 1.
int cpt::ctx::present_state(cpt_ctx* c) {
    HIP_TRY(c, hipSetDevice(c->device));
    PresentState& p = c->frame.present;
    if (int rc = p.d_bgra.ensure(c, c->npix() * 4)) return rc;
    if (p.d_words) return CPT_OK;
    DevBuf<uint32_t> words;
    if (int rc = words.ensure(c, prs::HIST_WORDS + 1)) return rc;
    HIP_TRY(c, hipMemsetAsync(words, 0, prs::HIST_WORDS * sizeof(uint32_t), c->stream()));
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)(words.get() + EXPOSURE_WORD), (int)prs::bits_of(1.0f), 1, c->stream()));
    p.d_words = std::move(words);
    return CPT_OK;
}

extern "C" {

int cpt_set_exposure(cpt_ctx* c, float exposure) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!(cpt::filter::finite(exposure) && exposure > 0.f))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_set_exposure: %g (finite, > 0)", (double)exposure);
    if (int rc = present_source(c, "cpt_set_exposure", CPT_PRESENT_ACCUM, nullptr)) return rc;
    if (int rc = present_state(c)) return rc;
    HIP_TRY(c, hipMemsetD32Async((hipDeviceptr_t)(c->frame.present.d_words.get() + EXPOSURE_WORD), (int)prs::bits_of(exposure), 1,
                                 c->stream()));
    return CPT_OK;
}

int cpt_meter_exposure(cpt_ctx* c, int source, float key, int permille, float adapt) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!prs::source_ok(source) || !meter_args_ok(key, permille, adapt))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_meter_exposure: source %d, key %g (finite, > 0), permille %d (0..1000), adapt %g (0..1)",
                    source, (double)key, permille, (double)adapt);
    const float4* src = nullptr;
    if (int rc = present_source(c, "cpt_meter_exposure", source, &src)) return rc;
    if (int rc = present_state(c)) return rc;
    hipStream_t s = c->stream();
    if (int rc = c->t_present.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_meter(src, c->npix(), source, key, permille, adapt, c->frame.present.d_words, c->grid.cus, s));
    return c->t_present.end(c, s);
}

int cpt_read_exposure(cpt_ctx* c, float* exposure, uint32_t* hist257) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (int rc = present_source(c, "cpt_read_exposure", CPT_PRESENT_ACCUM, nullptr)) return rc;
    if (int rc = present_state(c)) return rc;
    if (int rc = sync_checked(c)) return rc;
    uint32_t words[prs::HIST_WORDS + 1];
    if (int rc = read_back(c, words, c->frame.present.d_words, prs::HIST_WORDS + 1)) return rc;
    if (exposure) *exposure = prs::float_of(words[EXPOSURE_WORD]);
    if (hist257) std::memcpy(hist257, words, prs::HIST_WORDS * sizeof(uint32_t));
    return CPT_OK;
}

int cpt_present(cpt_ctx* c, int source, int tone, float white, int transfer, uint8_t* bgra_host) {
    if (!c) return CPT_ERR_INVALID_ARG;
    if (!prs::args_ok(source, tone, white, transfer))
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_present: source %d, tone %d, white %g (> 0), transfer %d", source, tone, (double)white,
                    transfer);
    const float4* src = nullptr;
    if (int rc = present_source(c, "cpt_present", source, &src)) return rc;
    if (int rc = present_state(c)) return rc;
    PresentState& p = c->frame.present;
    hipStream_t s = c->stream();
    const size_t npix = c->npix();
    if (int rc = c->t_present.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_present(src, npix, source, tone, white, transfer, p.d_words, p.d_bgra, s));
    if (int rc = c->t_present.end(c, s)) return rc;
    p.presented = true;
    if (bgra_host && npix) HIP_TRY(c, hipMemcpyAsync(bgra_host, p.d_bgra, npix * 4, hipMemcpyDeviceToHost, s));
    return CPT_OK;
}

int cpt_read_present(cpt_ctx* c, uint8_t* bgra, size_t capacity) {
    if (!c || !bgra) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.set || !f.present.presented) return fail(c, CPT_ERR_STATE, "cpt_read_present: cpt_present first");
    const size_t bytes = c->npix() * 4;
    if (capacity < bytes) return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_present: %zu < %zu bytes", capacity, bytes);
    if (int rc = sync_checked(c)) return rc;
    return read_back(c, bgra, f.present.d_bgra, bytes);
}

int cpt_copy_present_device(cpt_ctx* c, void* device_dst, size_t bytes, void* caller_stream) {
    if (!c || (!device_dst && bytes)) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.set || !f.present.presented) return fail(c, CPT_ERR_STATE, "cpt_copy_present_device: cpt_present first");
    const size_t have = c->npix() * 4;
    if (bytes > have) return fail(c, CPT_ERR_INVALID_ARG, "cpt_copy_present_device: %zu bytes requested, the frame holds %zu", bytes, have);
    return copy_ordered(c, device_dst, f.present.d_bgra, bytes, (hipStream_t)caller_stream);
}

int cpt_last_present_ms(cpt_ctx* c, float* ms) {
    return last_span_ms(c, &cpt_ctx::t_present, ms, "cpt_last_present_ms: no cpt_meter_exposure or cpt_present yet");
}

int cpt_present_host(size_t npix, int source, const float* src, float exposure, int tone, float white, int transfer, uint8_t* bgra) {
    if ((npix && (!src || !bgra)) || !prs::args_ok(source, tone, white, transfer)) return CPT_ERR_INVALID_ARG;
    for (size_t i = 0; i < npix; ++i) {
        float S[4];
        prs::host_pixel(source, src, i, S);
        const uint32_t w = prs::pixel_word(source, S[0], S[1], S[2], S[3], exposure, tone, white, transfer, SRGB_T);
        bgra[4 * i] = (uint8_t)w;
        bgra[4 * i + 1] = (uint8_t)(w >> 8);
        bgra[4 * i + 2] = (uint8_t)(w >> 16);
        bgra[4 * i + 3] = (uint8_t)(w >> 24);
    }
    return CPT_OK;
}

int cpt_meter_host(size_t npix, int source, const float* src, float key, int permille, float adapt, float* exposure,
                   uint32_t* hist257) {
    if ((npix && !src) || !exposure || !prs::source_ok(source) || !meter_args_ok(key, permille, adapt)) return CPT_ERR_INVALID_ARG;
    uint32_t hist[prs::HIST_WORDS] = {0};
    for (size_t i = 0; i < npix; ++i) {
        float S[4];
        prs::host_pixel(source, src, i, S);
        ++hist[prs::meter_word(source, S[0], S[1], S[2], S[3])];
    }
    *exposure = prs::resolve(hist, *exposure, key, permille, adapt);
    if (hist257) std::memcpy(hist257, hist, sizeof(hist));
    return CPT_OK;
}

int cpt_present_srgb_thresholds_host(float* t256) {
    if (!t256) return CPT_ERR_INVALID_ARG;
    std::memcpy(t256, SRGB_T, sizeof(SRGB_T));
    return CPT_OK;
}

}  // extern "C"
