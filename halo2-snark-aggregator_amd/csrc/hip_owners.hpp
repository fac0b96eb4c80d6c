// Owners of the HIP resources libh2agg.so holds: each releases its handle in its destructor, none knows the context
// (csrc/host.inc has what reports through it: ensure, ensure_pinned, dev_alloc).  All are move-only.  A handle reaches a HIP
// call through the conversion: hipEventRecord(c->ev_ready, c->stream), c->h_pinned + 1024, t.d + 64 * first.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace h2agg {

struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : h(o.h) { o.h = nullptr; }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() {
        if (h) (void)hipEventDestroy(h);
    }
    hipError_t create(unsigned flags) {   // (again: the event it held goes first)
        if (h) (void)hipEventDestroy(h);
        h = nullptr;
        return hipEventCreateWithFlags(&h, flags);
    }
    operator hipEvent_t() const { return h; }
};

struct Stream {
    hipStream_t h = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() {
        if (h) (void)hipStreamDestroy(h);
    }
    hipError_t create(unsigned flags, const int* priority = nullptr) {
        return priority ? hipStreamCreateWithPriority(&h, flags, *priority) : hipStreamCreateWithFlags(&h, flags);
    }
    operator hipStream_t() const { return h; }
};

struct PinnedBuf {   // a grow-only page-locked host block (ensure_pinned, csrc/host.inc)
    uint8_t* p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf&) = delete;
    PinnedBuf& operator=(const PinnedBuf&) = delete;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    operator uint8_t*() const { return p; }
};

struct DevBuf {   // a grow-only device buffer (ensure, csrc/host.inc); freed with its owner
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

// A device allocation of exactly the size asked for: a base table's columns, the work memory of one call.  hipFree waits for
// the device, so nothing queued still uses the memory once its owner has gone.
struct DevMem {
    uint8_t* p = nullptr;
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) {
            reset();
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { reset(); }
    void reset() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    // A failed allocation also leaves HIP's last-error slot set, which the hipGetLastError() behind the next launches would
    // report as that call's failure: taken out here.
    hipError_t alloc(size_t bytes) {
        reset();
        const hipError_t e = hipMalloc((void**)&p, bytes ? bytes : 1);
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
        }
        return e;
    }
    operator uint8_t*() const { return p; }
};

}  // namespace h2agg
