// The owner of every device and pinned allocation of the host engines: a pointer with its capacity (in
// elements), move-only, freed by its destructor.  It reads like the pointer it holds, so a use site is
// written as for a raw pointer.  After a failed allocation the buffer is empty (null, capacity 0): the next
// reserve() allocates again.  Host only; no kernel sees it.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <atomic>

namespace mdqt {

// Where a Buf's memory comes from: alloc(void**, bytes, flags), release(void*), and the bytes its Bufs hold now
struct DeviceSpace {
    static inline std::atomic<long long> live{0};   // mdqt_live_bytes(0)
    static hipError_t alloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static hipError_t release(void* p) { return hipFree(p); }
};
struct PinnedSpace {
    static inline std::atomic<long long> live{0};   // mdqt_live_bytes(1)
    static hipError_t alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static hipError_t release(void* p) { return hipHostFree(p); }
};

template <class T, class Space>
class Buf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_; n_ = o.n_;
            o.p_ = nullptr; o.n_ = 0;
        }
        return *this;
    }
    ~Buf() { reset(); }

    operator T*() const { return p_; }
    T* get() const { return p_; }   // where a template or a cast needs the pointer itself
    size_t capacity() const { return n_; }

    void reset() {
        if (!p_) return;
        (void)Space::release(const_cast<void*>(static_cast<const volatile void*>(p_)));
        Space::live -= (long long)(n_ * sizeof(T));
        p_ = nullptr;
        n_ = 0;
    }
    // exactly n elements (n = 0: none), what was held freed first; the contents are not kept
    hipError_t alloc(size_t n, unsigned flags = 0) {
        reset();
        if (!n) return hipSuccess;
        void* q = nullptr;
        const hipError_t r = Space::alloc(&q, n * sizeof(T), flags);
        if (r != hipSuccess) return r;
        p_ = static_cast<T*>(q);
        n_ = n;
        Space::live += (long long)(n * sizeof(T));
        return hipSuccess;
    }
    // at least n elements: nothing where they are there already
    hipError_t reserve(size_t n, unsigned flags = 0) { return n <= n_ ? hipSuccess : alloc(n, flags); }
};

template <class T> using DevBuf = Buf<T, DeviceSpace>;
template <class T> using PinBuf = Buf<T, PinnedSpace>;

}  // namespace mdqt
