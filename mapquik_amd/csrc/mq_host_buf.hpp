// mq_host_buf.hpp -- what the host side owns (part of the one translation unit mq_capi.hip): the thread's error text and HIPCHK, a
// move-only device / page-locked buffer that frees itself, a scoped owner for events, streams and other handles, and the one guard that
// closes every extern "C" entry point.
#pragma once

static thread_local std::string g_err;
static int set_err(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIPCHK(expr)                                                                                              \
    do {                                                                                                          \
        hipError_t _e = (expr);                                                                                   \
        if (_e != hipSuccess) {                                                                                   \
            char _b[512];                                                                                         \
            snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__);  \
            return set_err(_e == hipErrorOutOfMemory ? MQ_ENOMEM : MQ_EHIP, _b);                                  \
        }                                                                                                         \
    } while (0)

// T[cap] in device memory (PINNED: page-locked host memory), freed by its destructor on whichever device is current then: the owner of
// a Buf selects its device before the Buf goes.  ensure() only ever grows; alloc() is for a size that is known (one-off allocations, and
// groups of buffers that share one capacity: their owner resets the whole group first, so that none is left half grown).
template <class T, bool PINNED = false>
struct Buf {
    T *p = nullptr;
    uint64_t cap = 0;  // elements
    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p, o.p);
            std::swap(cap, o.cap);
        }
        return *this;
    }
    ~Buf() { reset(); }
    operator T *() const { return p; }
    void reset() {
        if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    hipError_t try_alloc(uint64_t n) {  // exactly n elements, in place of what it held
        reset();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        else p = nullptr;
        return e;
    }
    int alloc(uint64_t n) {  // the same with the error recorded
        HIPCHK(try_alloc(n));
        return MQ_OK;
    }
    int ensure(uint64_t need) { return need <= cap ? MQ_OK : alloc(need + need / 4 + 64); }
};
template <class T>
using PinnedBuf = Buf<T, true>;
template <class... B>
static void reset_all(B &...b) {  // a group of buffers under one capacity: all of it goes before any of it comes back
    (b.reset(), ...);
}

// One handle (an event, a stream, a block of mq_host_alloc) given back when its owner goes.  Movable, so that a std::vector can hold them.
template <class H, auto Destroy>
struct Scoped {
    H h = nullptr;
    Scoped() = default;
    Scoped(Scoped &&o) noexcept : h(o.h) { o.h = nullptr; }
    Scoped &operator=(const Scoped &) = delete;
    ~Scoped() { reset(); }
    void reset() {
        if (h) (void)Destroy(h);
        h = nullptr;
    }
    operator H() const { return h; }
};
using ScopedEvent = Scoped<hipEvent_t, hipEventDestroy>;
using ScopedStream = Scoped<hipStream_t, hipStreamDestroy>;

// A file descriptor closed when its owner goes; close() for the caller who wants to know how the close went.
struct ScopedFd {
    int fd = -1;
    explicit ScopedFd(int f) : fd(f) {}
    ScopedFd(const ScopedFd &) = delete;
    ScopedFd &operator=(const ScopedFd &) = delete;
    ~ScopedFd() { (void)close(); }
    bool close() {
        const bool ok = fd < 0 || ::close(fd) == 0;
        fd = -1;
        return ok;
    }
    operator int() const { return fd; }
};

// The extern "C" boundary: no exception leaves the library.  R is the entry point's return type: an error code for int / int64_t, nullptr
// for the entry points that return a handle.
template <class F>
static auto guarded(F &&f) -> decltype(f()) {
    using R = decltype(f());
    int rc;
    try {
        return f();
    } catch (const std::bad_alloc &) {
        rc = set_err(MQ_ENOMEM, "out of host memory");
    } catch (const std::exception &e) {
        rc = set_err(MQ_EINVAL, std::string("unexpected exception: ") + e.what());
    }
    if constexpr (std::is_pointer<R>::value) return nullptr;
    else return (R)rc;
}
