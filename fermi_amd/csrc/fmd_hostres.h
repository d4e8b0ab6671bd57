// fmd_hostres.h -- the owning host-side GPU resources of libfmdhip.so (host-only, header-only; included from fmd_internal.h).
// One type per kind of resource; a .hip file defines none of its own.  Plain structs: no copies, a noexcept move where a
// container needs one, a destructor that frees.  Long-lived handles stay C structs with close functions.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

// ---- small shared helpers
static inline hipStream_t S(void *s) { return (hipStream_t)s; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// blocks for n items, t threads each: at most 2^31 threads per launch (the dispatch packet counts work-items in 32
// bits; the kernels loop with a grid stride)
static inline unsigned fmd_nblk(uint64_t n, unsigned t)
{
    const uint64_t b = (n + t - 1) / t, cap = (1ull << 31) / t;
    return (unsigned)(b < cap ? (b ? b : 1) : cap);
}
// one wave (workgroup) per item, at most 2^24 of them: the kernels stride
static inline unsigned fmd_wave_grid(uint64_t n_waves) { return (unsigned)(n_waves < (1u << 24) ? (n_waves ? n_waves : 1) : (1u << 24)); }
// a byte count read as 64 bits (the input of a scan through rocprim::transform_iterator)
struct FmdWiden { __host__ __device__ uint64_t operator()(uint8_t v) const { return (uint64_t)v; } };

// ---- device memory (hipMalloc).  alloc: FMD_OK or FMD_E_NOMEM, the error recorded and the runtime's sticky one cleared; a request
// of 0 bytes gets 16.  need: grow-only (the contents are lost when it grows).  release: the pointer is the caller's from then on.
struct FmdDevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    FmdDevBuf() {}
    FmdDevBuf(const FmdDevBuf &) = delete;
    FmdDevBuf &operator=(const FmdDevBuf &) = delete;
    FmdDevBuf(FmdDevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    FmdDevBuf &operator=(FmdDevBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~FmdDevBuf() { reset(); }
    int alloc(size_t b, const char *what = "hipMalloc")
    {
        reset();
        const hipError_t e = hipMalloc(&p, b ? b : 16);
        if (e != hipSuccess) { p = nullptr; fmd_set_hip_error(e, what); return FMD_E_NOMEM; }
        bytes = b;
        return FMD_OK;
    }
    int need(size_t b) { return b <= bytes ? FMD_OK : alloc(b); }
    void reset() { if (p) hipFree(p); p = nullptr; bytes = 0; }
    void *release() { void *q = p; p = nullptr; bytes = 0; return q; }
    template <class T> T *as() const { return (T *)p; }
};

// ---- pinned host memory (hipHostMalloc), the same shape
struct FmdHostBuf {
    void *p = nullptr;
    size_t bytes = 0;
    FmdHostBuf() {}
    FmdHostBuf(const FmdHostBuf &) = delete;
    FmdHostBuf &operator=(const FmdHostBuf &) = delete;
    FmdHostBuf(FmdHostBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    FmdHostBuf &operator=(FmdHostBuf &&o) noexcept { if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~FmdHostBuf() { reset(); }
    int alloc(size_t b, const char *what = "hipHostMalloc")
    {
        reset();
        const hipError_t e = hipHostMalloc(&p, b ? b : 16, hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; fmd_set_hip_error(e, what); return FMD_E_NOMEM; }
        bytes = b;
        return FMD_OK;
    }
    int need(size_t b) { return b <= bytes ? FMD_OK : alloc(b); }
    void reset() { if (p) hipHostFree(p); p = nullptr; bytes = 0; }
    void *release() { void *q = p; p = nullptr; bytes = 0; return q; }
    template <class T> T *as() const { return (T *)p; }
};

// ---- hipHostRegister for a scope: only arrays of min_bytes and more, never under FMD_NO_PIN, silently skipped when it fails
// (the copies are pageable then)
struct FmdHostPin {
    void *p = nullptr;
    FmdHostPin() {}
    FmdHostPin(void *ptr, size_t bytes, size_t min_bytes) { pin(ptr, bytes, min_bytes); }
    FmdHostPin(const FmdHostPin &) = delete;
    FmdHostPin &operator=(const FmdHostPin &) = delete;
    FmdHostPin(FmdHostPin &&o) noexcept : p(o.p) { o.p = nullptr; }
    ~FmdHostPin() { if (p) hipHostUnregister(p); }
    void pin(void *ptr, size_t bytes, size_t min_bytes)
    {
        if (p || !ptr || bytes < min_bytes || getenv("FMD_NO_PIN")) return;
        if (hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess) p = ptr; else (void)hipGetLastError();
    }
};

// ---- a stream (non-blocking unless asked otherwise), an event (without timing unless asked otherwise)
struct FmdStream {
    hipStream_t s = nullptr;
    FmdStream() {}
    FmdStream(const FmdStream &) = delete;
    FmdStream &operator=(const FmdStream &) = delete;
    ~FmdStream() { reset(); }
    int make(unsigned flags = hipStreamNonBlocking) { return hipStreamCreateWithFlags(&s, flags) == hipSuccess ? FMD_OK : FMD_E_HIP; }
    void reset() { if (s) hipStreamDestroy(s); s = nullptr; }
    operator hipStream_t() const { return s; }
};
struct FmdEvent {
    hipEvent_t e = nullptr;
    FmdEvent() {}
    FmdEvent(const FmdEvent &) = delete;
    FmdEvent &operator=(const FmdEvent &) = delete;
    FmdEvent(FmdEvent &&o) noexcept : e(o.e) { o.e = nullptr; }
    ~FmdEvent() { reset(); }
    int make(unsigned flags = hipEventDisableTiming) { return hipEventCreateWithFlags(&e, flags) == hipSuccess ? FMD_OK : FMD_E_HIP; }
    void reset() { if (e) hipEventDestroy(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

// ---- a second stream with its events, kept in a long-lived handle (fmd_dev): zero bytes are its empty state, it is made on the first
// acquire and goes with destroy().  One caller at a time: acquire is false while another call holds it (that call takes its serial
// path) and when the stream or one of its n_events (<= FMD_OVLP_MAX_PARTS + 1) events cannot be made -- what was made is freed, the
// runtime's last error cleared, and the next acquire tries again.
struct FmdSideStream {
    hipStream_t stream;   // non-blocking: must not synchronise with the null stream
    hipEvent_t ev[FMD_OVLP_MAX_PARTS + 1];
    int ready, busy;      // (busy: atomic)
    bool acquire(int n_events)
    {
        int expect = 0;
        if (!__atomic_compare_exchange_n(&busy, &expect, 1, false, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED)) return false;
        if (!ready) {
            bool ok = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess;
            int made = 0;
            for (; ok && made < n_events; ++made) ok = hipEventCreateWithFlags(&ev[made], hipEventDisableTiming) == hipSuccess;
            if (!ok) {
                for (int i = 0; i < made - 1; ++i) hipEventDestroy(ev[i]);
                if (stream) { hipStreamDestroy(stream); stream = nullptr; }   // or every retry would leak a stream
                (void)hipGetLastError();
                release();
                return false;
            }
            ready = n_events;
        }
        return true;
    }
    void release() { __atomic_store_n(&busy, 0, __ATOMIC_RELEASE); }
    void destroy()
    {
        if (!ready) return;
        hipStreamDestroy(stream);
        for (int i = 0; i < ready; ++i) hipEventDestroy(ev[i]);
        stream = nullptr; ready = 0;
    }
};

// ---- a buffer of the handle's scratch cache (fmd_scratch_acquire) for a scope: the same sizes come back call after call
struct FmdScratch {
    fmd_dev *h = nullptr;
    void *p = nullptr;
    FmdScratch() {}
    FmdScratch(const FmdScratch &) = delete;
    FmdScratch &operator=(const FmdScratch &) = delete;
    ~FmdScratch() { reset(); }
    int alloc(fmd_dev *h_, size_t bytes) { reset(); h = h_; p = fmd_scratch_acquire(h, bytes); return p ? FMD_OK : FMD_E_NOMEM; }
    void reset() { if (p) fmd_scratch_release(h, p); p = nullptr; }
    template <class T> T *as() const { return (T *)p; }
};

// ---- a rocPRIM primitive the two-call way: f(tmp, bytes) with tmp == nullptr sets bytes; then the temporary storage is allocated,
// f runs, the stream is waited for (sync) and the storage goes.  The first failure of the primitive or of the wait is the result.
static inline int fmd_hip_rc(hipError_t e, const char *what)
{
    if (e == hipSuccess) return FMD_OK;
    fmd_set_hip_error(e, what);
    return e == hipErrorOutOfMemory ? FMD_E_NOMEM : FMD_E_HIP;
}
template <class F>
static inline int fmd_with_tmp(hipStream_t st, bool sync, const char *what, F f)
{
    size_t bytes = 0;
    int rc = fmd_hip_rc(f(nullptr, bytes), what);
    if (rc) return rc;
    FmdDevBuf tmp;
    if ((rc = tmp.alloc(bytes, what))) return rc;
    const hipError_t e = f(tmp.p, bytes), e2 = sync ? hipStreamSynchronize(st) : hipSuccess;
    return fmd_hip_rc(e != hipSuccess ? e : e2, what);
}
