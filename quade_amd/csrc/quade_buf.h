// Who owns device and page-locked memory in the host code: one move-only buffer over five sources.
//
// Buf<Src> gives its memory back in its destructor.  Src says where the memory comes from and nothing else; the growth and ownership
// logic below calls HIP only through Src, so a host-only program can drive it with a source of its own (tests/native/quade_buf_test.cpp).
// How much a growth asks for is the call site's business: need(n, want) takes the bytes to request beside the bytes needed, because the
// pool keys reuse on the size and DESIGN quotes the footprints (quarter() is the rule most sites use).
// Nothing here is on a kernel's path.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>
#include <unistd.h>

#include "quade_pool.h"

extern "C" int qd_pool_trim(void);  // include/quade_hip.h

#pragma GCC visibility push(hidden)  // (header-only: the library exports nothing of it)
namespace qbuf {

// ---- sources: get() sets *cap to what the allocation holds (>= want), put() takes that back -----------------------------------------
struct DriverDev {  // the driver's device memory: long-lived tables, the stand-alone coders' staging
    static hipError_t get(size_t want, void** p, size_t* cap) {
        const hipError_t e = hipMalloc(p, want);
        if (e == hipSuccess) *cap = want;
        return e;
    }
    static void put(void* p, size_t) { (void)hipFree(p); }
};
struct DriverDevTrim : DriverDev {  // out of memory: the pool's idle buffers go back to the driver once (it can hold tens of GB) and the call is repeated
    static hipError_t get(size_t want, void** p, size_t* cap) {
        hipError_t e = DriverDev::get(want, p, cap);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            (void)qd_pool_trim();
            e = DriverDev::get(want, p, cap);
        }
        return e;
    }
};
struct PoolDev {  // quade_pool.h: device memory that a pipeline of this process released earlier; put() drains the device first
    static hipError_t get(size_t want, void** p, size_t* cap) { return qd_pool_get(want, p, cap); }
    static void put(void* p, size_t cap) { qd_pool_put(p, cap); }
    // for need(n, want, keep, st): nothing queued anywhere may still use the old allocation (the inflate launches run on a stream of their own)
    static hipError_t drain() { return hipDeviceSynchronize(); }
    static hipError_t copy(void* dst, const void* src, size_t n, hipStream_t st) {
        const hipError_t e = hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    }
};
struct DriverPin {  // the driver's page-locked host memory
    static hipError_t get(size_t want, void** p, size_t* cap) {
        const hipError_t e = hipHostMalloc(p, want, hipHostMallocDefault);
        if (e == hipSuccess) *cap = want;
        return e;
    }
    static void put(void* p, size_t) { (void)hipHostFree(p); }
};
struct PoolPin {  // quade_pool.h: page-locked host memory from the pool
    static hipError_t get(size_t want, void** p, size_t* cap) { return qd_pool_get_pinned(want, p, cap); }
    static void put(void* p, size_t cap) { qd_pool_put_pinned(p, cap); }
};

// the growth rule of most sites: a quarter more than needed and `pad` on top (in bytes or in elements, as the site counts)
inline size_t quarter(size_t n, size_t pad) { return n + n / 4 + pad; }
// StreamScratch's: twice what the buffer held, at least
inline size_t twice(size_t n, size_t held) { return n > 2 * held ? n : 2 * held; }

// ---- the owner ----------------------------------------------------------------------------------------------------------------------
template <class Src>
struct Buf {
    uint8_t* p = nullptr;
    size_t cap = 0;  // bytes; 0 beside p == nullptr

    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~Buf() { release(); }

    template <class T>
    T* as() const { return reinterpret_cast<T*>(p); }

    void release() {
        if (p) Src::put(p, cap);
        p = nullptr;
        cap = 0;
    }
    // exactly n bytes (the fixed tables); what the buffer held goes back first, and a failure leaves it empty
    hipError_t alloc(size_t n) {
        release();
        void* q = nullptr;
        size_t got = 0;
        const hipError_t e = Src::get(n, &q, &got);
        if (e == hipSuccess) p = static_cast<uint8_t*>(q), cap = q ? got : 0;
        return e;
    }
    // grow-only: room for n bytes; a growth asks the source for `want`
    hipError_t need(size_t n, size_t want) { return n <= cap ? hipSuccess : alloc(want); }
    // the same, and the first `keep` bytes survive the growth (copied on `st`, which is then drained); the new allocation is made before
    // the old one goes back, and a failure leaves the old one in place
    hipError_t need(size_t n, size_t want, size_t keep, hipStream_t st) {
        if (n <= cap) return hipSuccess;
        void* q = nullptr;
        size_t got = 0;
        hipError_t e = Src::get(want, &q, &got);
        if (e != hipSuccess) return e;
        if (p) (void)Src::drain();
        if (p && keep && (e = Src::copy(q, p, keep, st)) != hipSuccess) {
            Src::put(q, got);
            return e;
        }
        release();
        p = static_cast<uint8_t*>(q), cap = got;
        return hipSuccess;
    }
};

// A buffer of T that stands where a T* stood: it converts to the pointer, and sizes are still bytes.
template <class T, class Src>
struct Arr : Buf<Src> {
    operator T*() const { return this->template as<T>(); }
};

// A table that lives on both sides: page-locked host and device memory of one size, counted in elements of T (the stand-alone coders'
// staging).  Both halves or neither: a failed growth leaves the pair empty.
template <class T, class HostSrc = DriverPin, class DevSrc = DriverDev>
struct Pair {
    Arr<T, HostSrc> h;
    Arr<T, DevSrc> d;
    size_t cap() const { return (h.cap < d.cap ? h.cap : d.cap) / sizeof(T); }  // elements
    // room for n elements; a growth asks for `want` elements on each side
    hipError_t need(size_t n, size_t want) {
        if (n <= cap()) return hipSuccess;
        release();
        hipError_t e = h.alloc(want * sizeof(T));
        if (e == hipSuccess) e = d.alloc(want * sizeof(T));
        if (e != hipSuccess) release();
        return e;
    }
    void release() {
        h.release();
        d.release();
    }
};

// Waits for an event without holding a core: hipEventSynchronize spins on this runtime even for events made with hipEventBlockingSync
// (measured: the reader's device lanes burnt 0.95 core-seconds per M pairs waiting for their kernels,
// profiles/r03_e2e_16m_level1_stages_device_inflate.txt).  A few immediate polls (short kernels), then naps of nap_us.
inline hipError_t wait_event_napping(hipEvent_t ev, unsigned nap_us) {
    for (int i = 0; i < 64; ++i) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
    }
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        usleep(nap_us);
    }
}

}  // namespace qbuf
#pragma GCC visibility pop
