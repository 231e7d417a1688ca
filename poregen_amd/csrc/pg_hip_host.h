// pg_hip_host.h -- the host-side HIP scaffolding every handle of libpgmove shares (not installed; host code only, no kernels):
// the error slot, device selection, owning buffers / streams / events, pointer classification.
#pragma once
#include "../../include/pgmove.h"
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstdio>
#include <string>

// ---- the error slot ---------------------------------------------------------------------------------------------------
// A handle type H carries `std::string err`; an error without a handle (a failed create, a null handle) goes to a per-thread string
// of H's own family, which H_last_error(nullptr) returns.
template <class H> std::string &pg_create_error() { static thread_local std::string s; return s; }

template <class H> __attribute__((format(printf, 3, 4))) pg_status pg_fail(H *h, pg_status code, const char *fmt, ...) {
    char buf[1200];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (h) h->err = buf; else pg_create_error<H>() = buf;
    return code;
}
#define PG_HIP_TRY(h, expr) \
    do { hipError_t e_ = (expr); if (e_ != hipSuccess) return pg_fail((h), PG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

// a create that failed behind `new H`: the message moves to the family's create error, the half-built handle goes
template <class H> pg_status pg_create_failed(H *h, pg_status code, void (*destroy)(H *)) {
    pg_create_error<H>() = h->err;
    destroy(h);
    return code;
}

// ---- device selection at create ---------------------------------------------------------------------------------------
template <class H> pg_status pg_select_device(int device) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return pg_fail<H>(nullptr, PG_ERR_NO_DEVICE, "no HIP device available (%s); libpgmove has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device < 0 || device >= ndev) return pg_fail<H>(nullptr, PG_ERR_NO_DEVICE, "device %d out of range (have %d)", device, ndev);
    e = hipSetDevice(device);
    if (e != hipSuccess) return pg_fail<H>(nullptr, PG_ERR_NO_DEVICE, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    return PG_OK;
}

// ---- owning, move-only buffers that only grow -------------------------------------------------------------------------
// The device that owns the memory must be current when a buffer is freed (ensure, release, the destructor).
struct PgDevAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void *p) { return hipFree(p); }
};
struct PgPinnedAlloc {
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t free(void *p) { return hipHostFree(p); }
};
template <class T, class A> struct PgBuf {
    T *p = nullptr;
    size_t cap = 0; // bytes
    PgBuf() = default;
    PgBuf(const PgBuf &) = delete;
    PgBuf &operator=(const PgBuf &) = delete;
    PgBuf(PgBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PgBuf &operator=(PgBuf &&o) noexcept {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~PgBuf() { release(); }
    // Room for `bytes`. A buffer that is too small is freed and allocated anew with `alloc` >= bytes bytes -- the growth policy is the
    // caller's; the contents are not kept, and work that still uses the old allocation has to be waited for by the caller.
    hipError_t ensure(size_t bytes, size_t alloc) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = A::free(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = A::alloc((void **)&p, alloc);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = alloc;
        return hipSuccess;
    }
    hipError_t ensure(size_t bytes) { return ensure(bytes, bytes); } // exact
    void release() { if (p) (void)A::free(p); p = nullptr; cap = 0; }
    template <class U> U *as() const { return reinterpret_cast<U *>(p); }
};
template <class T = void> using PgDev = PgBuf<T, PgDevAlloc>;
template <class T = void> using PgPinned = PgBuf<T, PgPinnedAlloc>; // page-locked host memory

// ---- owning streams and events ----------------------------------------------------------------------------------------
// Declare them in front of a handle's buffers: members go in reverse order, so the buffers are freed first.
template <class T, hipError_t (*Destroy)(T)> struct PgOwned {
    T h = nullptr;
    PgOwned() = default;
    PgOwned(const PgOwned &) = delete;
    PgOwned &operator=(const PgOwned &) = delete;
    ~PgOwned() { if (h) (void)Destroy(h); }
    operator T() const { return h; }
};
using PgStream = PgOwned<hipStream_t, hipStreamDestroy>;
using PgEvent = PgOwned<hipEvent_t, hipEventDestroy>;

// ---- what kind of memory is this pointer? -----------------------------------------------------------------------------
enum PgPtrKind {
    PG_PTR_UNKNOWN, // null, or memory the runtime does not know (pageable host memory)
    PG_PTR_DEVICE,  // device memory of device `device`
    PG_PTR_PINNED,  // page-locked host memory
    PG_PTR_OTHER    // known to the runtime, none of the above (another device's memory, managed memory)
};
// owner (may be null): the device the runtime names for a pointer it knows. Leaves no sticky error behind.
static inline PgPtrKind pg_ptr_kind(const void *p, int device, int *owner = nullptr) {
    hipPointerAttribute_t a{};
    const bool known = p && hipPointerGetAttributes(&a, p) == hipSuccess;
    (void)hipGetLastError();
    if (!known) return PG_PTR_UNKNOWN;
    if (owner) *owner = a.device;
    if (a.type == hipMemoryTypeDevice) return a.device == device ? PG_PTR_DEVICE : PG_PTR_OTHER;
    return a.type == hipMemoryTypeHost ? PG_PTR_PINNED : PG_PTR_OTHER;
}
