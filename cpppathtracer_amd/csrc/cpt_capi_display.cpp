// cpt_capi_display.cpp — the C-ABI's display path: the denoise + running-mean kernel on a band
// of output rows, its BGRA8 frame and their readbacks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>

#include "cpt_context.hpp"

using namespace cpt::ctx;

// Display path on output rows [y0, y1) of the 16-aligned launch (path_tracer.cu:177-254).
// The context's frame rows must be one ascending run that covers the band and its 3-row halo
// (clipped to [0, H')): every neighbour the linear-offset stencil reaches.  The running mean
// and the BGRA8 rows belong to the band; a different band starts a fresh mean.
// `history`: the per-pixel Mix (cpt_denoise_mix_history), which has no cur_sample_idx.
static int denoise_band(cpt_ctx* c, uint32_t cur_sample_idx, int y0, int y1, uint8_t* bgra_host, size_t out_rows,
                        bool history = false) {
    Frame& f = c->frame;
    const char* who = history ? "cpt_denoise_mix_history" : "cpt_denoise_mix";   // the call LastError names
    if (!f.set) return fail(c, CPT_ERR_STATE, "%s: cpt_set_frame first", who);
    if (!f.d_normal || !f.d_depth) return fail(c, CPT_ERR_STATE, "%s: render with CPT_RENDER_AUX first", who);
    if (!history && cur_sample_idx == 0) return fail(c, CPT_ERR_INVALID_ARG, "cpt_denoise_mix: cur_sample_idx must be >= 1");
    const int h_eff = 16 * (c->height / 16);
    if (y0 < 0 || y1 > h_eff || y0 >= y1)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_denoise_mix_band: band [%d, %d) outside [0, %d)", y0, y1, h_eff);
    const int row0 = c->rows_h.empty() ? 0 : c->rows_h[0];
    for (int i = 0; i < c->n_rows; ++i)
        if (c->rows_h[i] != row0 + i)
            return fail(c, CPT_ERR_STATE, "%s: the frame rows must be one ascending run", who);
    const int need0 = std::max(0, y0 - 3), need1 = std::min(h_eff, y1 + 3);
    if (row0 > need0 || row0 + c->n_rows < need1)
        return fail(c, CPT_ERR_STATE, "cpt_denoise_mix_band: rows [%d, %d) rendered, band [%d, %d) needs [%d, %d)", row0,
                    row0 + c->n_rows, y0, y1, need0, need1);
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t s = c->stream();
    const size_t cap_rows = std::max<size_t>(out_rows, (size_t)(y1 - y0));
    if (f.display.y0 != y0 || f.display.y1 != y1) {
        // both new buffers first, then the switch: a failure here leaves the previous band, its
        // buffers and band_y0/1, as they were
        const size_t n = cap_rows * c->width;
        DevBuf<float> mix, count;
        DevBuf<uint8_t> bgra;
        if (int rc = ensure_all(c, mix, n * 3, count, n, bgra, n * 4)) return rc;
        HIP_TRY(c, hipMemsetAsync(mix, 0, n * 3 * sizeof(float), s));
        HIP_TRY(c, hipMemsetAsync(count, 0, n * sizeof(float), s));
        HIP_TRY(c, hipMemsetAsync(bgra, 0, n * 4, s));
        f.display.d_mix = std::move(mix);
        f.display.d_count = std::move(count);
        f.display.d_bgra = std::move(bgra);
        f.display.d_mix_next = DevBuf<float>();
        f.display.d_count_next = DevBuf<float>();
        f.display.last_idx = 0;
        f.display.count_stale = false;
        f.display.y0 = y0;
        f.display.y1 = y1;
    }
    // A pinned host frame (hipHostMalloc / hipHostRegister, e.g. torch's pin_memory) is written by
    // the kernel itself through its device alias, so the PCIe transfer overlaps the stencil
    // instead of following it; pageable memory takes the copy after the kernel.
    uint8_t* host_alias = nullptr;
    if (bgra_host && c->width % 16 == 0) {   // (columns past 16*(W/16) are never written by the kernel)
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, bgra_host) == hipSuccess && attr.type == hipMemoryTypeHost &&
            attr.devicePointer != nullptr)
            host_alias = static_cast<uint8_t*>(attr.devicePointer);
        else
            (void)hipGetLastError();   // pageable: not an error
    }
    if (int rc = f.display.d_sink.ensure(c, cpt::DN_SINK_SLOTS)) return rc;
    if (history)
        if (int rc = f.display.fill_count(c)) return rc;
    if (int rc = c->t_display.begin(c, s)) return rc;
    HIP_TRY(c, cpt::launch_denoise_mix(f.d_accum, f.d_normal, f.d_depth, f.display.d_mix, history ? f.display.d_count.get() : nullptr,
                                      f.display.d_bgra, host_alias, f.display.d_sink, c->width, c->height, row0, c->n_rows, y0, y1,
                                      cur_sample_idx, c->grid, s));
    if (int rc = c->t_display.end(c, s)) return rc;
    if (!history) {
        // every pixel of the launch region now has, by definition, cur_sample_idx samples
        f.display.last_idx = cur_sample_idx;
        f.display.count_stale = true;
    }
    if (bgra_host && host_alias) {
        // the kernel writes the band's rows; the rest of the frame is zero, as the copy gives
        const size_t band = (size_t)(y1 - y0) * c->width * 4;
        std::memset(bgra_host + band, 0, cap_rows * c->width * 4 - band);
        HIP_TRY(c, hipStreamSynchronize(s));
    } else if (bgra_host) {
        HIP_TRY(c, hipMemcpyAsync(bgra_host, f.display.d_bgra, cap_rows * c->width * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(c, hipStreamSynchronize(s));
    }
    return CPT_OK;
}

// The count plane as cpt_denoise_mix[_band]'s bookkeeping defines it: the band's launch region
// (its rows x W') filled with the last recorded index; the pixels outside it stay 0.
int DisplayBand::fill_count(cpt_ctx* c) {
    if (!count_stale) return CPT_OK;
    HIP_TRY(c, cpt::launch_fill_count(d_count, c->width, 16 * (c->width / 16), y1 - y0, (float)last_idx, c->stream()));
    count_stale = false;
    return CPT_OK;
}

// What cpt_denoise_mix and cpt_denoise_mix_history (`who`) ask of the frame; *launch: false when
// the launch region is empty (the host frame is zeroed, nothing is launched).
static int full_frame_display(cpt_ctx* c, const char* who, uint8_t* bgra_host, bool* launch) {
    *launch = false;
    if (int rc = require_full_frame(c, who)) return rc;
    if (16 * (c->width / 16) == 0 || 16 * (c->height / 16) == 0) {   // nothing is launched; the frame stays 0
        if (bgra_host) std::memset(bgra_host, 0, (size_t)c->width * c->height * 4);
        return CPT_OK;
    }
    *launch = true;
    return CPT_OK;
}

extern "C" {

int cpt_last_display_ms(cpt_ctx* c, float* ms) {
    return last_span_ms(c, &cpt_ctx::t_display, ms, "cpt_last_display_ms: no display frame yet");
}

int cpt_denoise_mix(cpt_ctx* c, uint32_t cur_sample_idx, uint8_t* bgra_host) {
    if (!c) return CPT_ERR_INVALID_ARG;
    bool launch;
    if (int rc = full_frame_display(c, "cpt_denoise_mix", bgra_host, &launch)) return rc;
    if (!launch) return CPT_OK;
    // the whole frame's rows (those past H' are never written and stay 0)
    return denoise_band(c, cur_sample_idx, 0, 16 * (c->height / 16), bgra_host, (size_t)c->height);
}

int cpt_denoise_mix_history(cpt_ctx* c, uint8_t* bgra_host) {
    if (!c) return CPT_ERR_INVALID_ARG;
    bool launch;
    if (int rc = full_frame_display(c, "cpt_denoise_mix_history", bgra_host, &launch)) return rc;
    if (!launch) return CPT_OK;
    return denoise_band(c, 0, 0, 16 * (c->height / 16), bgra_host, (size_t)c->height, true);
}

int cpt_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return fail(nullptr, CPT_ERR_INVALID_ARG, "cpt_host_register: empty buffer");
    const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterMapped);
    if (e != hipSuccess) return fail(nullptr, CPT_ERR_HIP, "cpt_host_register: %s", hipGetErrorString(e));
    return CPT_OK;
}

int cpt_host_unregister(void* ptr) {
    if (!ptr) return fail(nullptr, CPT_ERR_INVALID_ARG, "cpt_host_unregister: null buffer");
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) return fail(nullptr, CPT_ERR_HIP, "cpt_host_unregister: %s", hipGetErrorString(e));
    return CPT_OK;
}

int cpt_denoise_mix_band(cpt_ctx* c, uint32_t cur_sample_idx, int y0, int y1, uint8_t* bgra_host) {
    if (!c) return CPT_ERR_INVALID_ARG;
    return denoise_band(c, cur_sample_idx, y0, y1, bgra_host, 0);
}

int cpt_copy_bgra_device(cpt_ctx* c, void* device_dst, size_t bytes, void* caller_stream) {
    if (!c || !device_dst) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.display.d_bgra) return fail(c, CPT_ERR_STATE, "cpt_copy_bgra_device: no display frame yet");
    const size_t have = (size_t)(f.display.y1 - f.display.y0) * c->width * 4;
    if (bytes > have) return fail(c, CPT_ERR_INVALID_ARG, "cpt_copy_bgra_device: %zu bytes requested, band holds %zu", bytes, have);
    return copy_ordered(c, device_dst, f.display.d_bgra, bytes, (hipStream_t)caller_stream);
}

int cpt_display_band(const cpt_ctx* c, int* y0, int* y1) {
    if (!c || !y0 || !y1) return CPT_ERR_INVALID_ARG;
    *y0 = c->frame.display.d_mix ? c->frame.display.y0 : 0;
    *y1 = c->frame.display.d_mix ? c->frame.display.y1 : 0;
    return CPT_OK;
}

int cpt_read_mix(cpt_ctx* c, float* rgb, size_t capacity) {
    if (!c || !rgb) return CPT_ERR_INVALID_ARG;
    const Frame& f = c->frame;
    if (!f.display.d_mix) return fail(c, CPT_ERR_STATE, "cpt_read_mix: no display frame yet");
    const size_t rows = (size_t)(f.display.y1 - f.display.y0);
    if (capacity < rows * c->width * 3)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_mix: %zu floats given, the band [%d, %d) holds %zu", capacity,
                    f.display.y0, f.display.y1, rows * c->width * 3);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(rgb, f.display.d_mix, rows * c->width * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream()));
    return sync_checked(c);
}

int cpt_read_display_count(cpt_ctx* c, float* count, size_t capacity) {
    if (!c || !count) return CPT_ERR_INVALID_ARG;
    Frame& f = c->frame;
    if (!f.display.d_mix) return fail(c, CPT_ERR_STATE, "cpt_read_display_count: no display frame yet");
    const size_t rows = (size_t)(f.display.y1 - f.display.y0);
    if (capacity < rows * c->width)
        return fail(c, CPT_ERR_INVALID_ARG, "cpt_read_display_count: %zu floats given, the band [%d, %d) holds %zu", capacity,
                    f.display.y0, f.display.y1, rows * c->width);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = f.display.fill_count(c)) return rc;
    HIP_TRY(c, hipMemcpyAsync(count, f.display.d_count, rows * c->width * sizeof(float), hipMemcpyDeviceToHost, c->stream()));
    return sync_checked(c);
}

int cpt_reset_display(cpt_ctx* c) {
    if (!c) return CPT_ERR_INVALID_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    Frame& f = c->frame;
    if (f.display.d_mix) {
        const int h_eff = 16 * (c->height / 16);
        const size_t rows = f.display.y0 == 0 && f.display.y1 == h_eff ? (size_t)c->height : (size_t)(f.display.y1 - f.display.y0);
        // (a full band set by cpt_denoise_mix_band holds H' rows, not the frame's, and after a
        // cpt_reproject_display the planes are the frame's: never past either plane)
        const size_t n = std::min({rows * c->width, f.display.d_mix.capacity() / 3, f.display.d_count.capacity()});
        HIP_TRY(c, hipMemsetAsync(f.display.d_mix, 0, n * 3 * sizeof(float), c->stream()));
        HIP_TRY(c, hipMemsetAsync(f.display.d_count, 0, n * sizeof(float), c->stream()));
        f.display.last_idx = 0;
        f.display.count_stale = false;
    }
    return CPT_OK;
}

}  // extern "C"
