// cpt_devmem.hpp — the C-ABI's error helpers (fail, HIP_TRY) and the move-only owners of what a
// context holds on the device: DevBuf<T> (a unique_ptr with a capacity; ensure_all for several,
// read_back / write_in for its blocking host copies), HostPinned<T> (pinned host words a stream
// writes), DevEvent, DevStream.
// A default-constructed owner is empty; assigning a fresh one releases what it held.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#include "../../include/cpt.h"

namespace cpt {
namespace ctx {

// Records a formatted message on the context (or, without one, for cpt_last_error(NULL)) and
// returns `code`.
int fail(cpt_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                             \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return fail((ctx), e_ == hipErrorOutOfMemory ? CPT_ERR_OUT_OF_MEMORY : CPT_ERR_HIP,        \
                        "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);           \
    } while (0)

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            cap_ = std::exchange(o.cap_, 0);
        }
        return *this;
    }
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }   // elements
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // Exactly `count` (> 0) elements in place of what the buffer held; empty on failure.
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = hipMalloc((void**)&p_, count * sizeof(T));
        if (e == hipSuccess) cap_ = count;
        else p_ = nullptr;
        return e;
    }
    // Room for `count` elements: the allocation is kept when it is large enough, else replaced
    // by one of exactly `count` (none for 0).  On failure the buffer is empty.
    int ensure(cpt_ctx* c, size_t count) {
        if (p_ && cap_ >= count) return CPT_OK;
        reset();
        if (count == 0) return CPT_OK;
        HIP_TRY(c, alloc(count));
        return CPT_OK;
    }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// Room in several buffers, ensure_all(c, a, count_a, b, count_b, ...): in the written order, and the
// first failure ends it with that failure's status (the buffers before it keep their room).
inline int ensure_all(cpt_ctx*) { return CPT_OK; }
template <typename T, typename... Rest>
int ensure_all(cpt_ctx* c, DevBuf<T>& buf, size_t count, Rest&&... rest) {
    if (int rc = buf.ensure(c, count)) return rc;
    return ensure_all(c, rest...);
}

// The blocking copies between a host array and `count` elements of a buffer (read_back: from
// element `first` on): hipMemcpy, which waits for the copy and for nothing queued on the context's
// stream, so the caller drains first (cpt_context.hpp: drain, sync_checked).  Nothing is issued for
// a count of 0.
template <typename T>
int read_back(cpt_ctx* c, void* host, const DevBuf<T>& buf, size_t count, size_t first = 0) {
    if (count) HIP_TRY(c, hipMemcpy(host, buf.get() + first, count * sizeof(T), hipMemcpyDeviceToHost));
    return CPT_OK;
}
template <typename T>
int write_in(cpt_ctx* c, DevBuf<T>& buf, const void* host, size_t count) {
    if (count) HIP_TRY(c, hipMemcpy(buf.get(), host, count * sizeof(T), hipMemcpyHostToDevice));
    return CPT_OK;
}

// A few page-locked host words a stream copies results into: the copy is then truly asynchronous
// (a read-back into pageable memory makes hipMemcpyAsync wait), and the host reads the words after
// waiting for an event recorded behind it.
template <typename T>
class HostPinned {
public:
    HostPinned() = default;
    HostPinned(const HostPinned&) = delete;
    HostPinned& operator=(const HostPinned&) = delete;
    ~HostPinned() { if (p_) (void)hipHostFree(p_); }
    // `count` (> 0) elements, once; an owner that already holds memory keeps it.
    hipError_t alloc(size_t count) {
        if (p_) return hipSuccess;
        const hipError_t e = hipHostMalloc((void**)&p_, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    // volatile: the device writes the words behind the compiler's back
    volatile T* get() const { return p_; }
    T* raw() const { return p_; }

private:
    T* p_ = nullptr;
};

class DevEvent {
public:
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    DevEvent& operator=(DevEvent&& o) noexcept {
        std::swap(e_, o.e_);
        return *this;
    }
    ~DevEvent() { if (e_) (void)hipEventDestroy(e_); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

class DevStream {
public:
    DevStream() = default;
    DevStream(const DevStream&) = delete;
    DevStream& operator=(const DevStream&) = delete;
    ~DevStream() { if (s_) (void)hipStreamDestroy(s_); }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s_, flags); }
    operator hipStream_t() const { return s_; }

private:
    hipStream_t s_ = nullptr;
};

}  // namespace ctx
}  // namespace cpt
