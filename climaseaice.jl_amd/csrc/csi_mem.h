// csi_mem.h -- the one owner of memory the library allocates itself: a device allocation (DeviceBuf) or a pinned host allocation
// (PinnedBuf).  Move-only; the destructor frees.  An EMPTY owner never calls HIP -- contexts are built on the stack, on machines
// without a GPU, by the csi_plan_* entry points.  Every failure leaves "empty, size 0", so the next call tries again.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>

namespace csi_host {

template <class T, bool kPinned>
class Buf {
  public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { release(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~Buf() { release(); }

    T* get() const { return p_; }
    size_t size() const { return n_; }          // elements
    explicit operator bool() const { return p_ != nullptr; }

    // Free now.  The CALLER has waited for whatever may still use the array (ensure() below does that itself).
    void release() {
        if (p_) (void)(kPinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; n_ = 0;
    }
    // Replace the allocation by one of n elements (contents undefined).  flags: hipHostMalloc's (pinned) / hipExtMallocWithFlags'
    // (device; 0: plain hipMalloc).  The size is recorded only once the allocation has succeeded.
    hipError_t alloc(size_t n, unsigned flags = 0) {
        release();
        void* p = nullptr;
        const hipError_t e = kPinned ? hipHostMalloc(&p, n * sizeof(T), flags)
                                     : (flags ? hipExtMallocWithFlags(&p, n * sizeof(T), flags) : hipMalloc(&p, n * sizeof(T)));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p); n_ = n;
        return hipSuccess;
    }
    // Exactly n elements.  Unchanged size: NO HIP call (the steady state of every sub-cycle; small grids are host-bound) and the
    // address stays what it was -- neighbouring tiles and a host-channel group hold mappings of some of these arrays.  Otherwise:
    // wait for the streams whose queued work may still read the old array (`also`: a second stream that uses it), free, allocate,
    // optionally zero on `stream`.  *fresh: the array is a new one (its contents are the caller's to provide).
    hipError_t ensure(size_t n, hipStream_t stream, bool zero, hipStream_t also = nullptr, bool* fresh = nullptr) {
        if (fresh) *fresh = n != n_;
        if (n == n_) return hipSuccess;
        hipError_t e;
        if (p_) {
            if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
            if (also && (e = hipStreamSynchronize(also)) != hipSuccess) return e;
        }
        if ((e = alloc(n)) != hipSuccess) return e;
        if (zero && (e = hipMemsetAsync(p_, 0, n * sizeof(T), stream)) != hipSuccess) { release(); return e; }
        return hipSuccess;
    }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T> using DeviceBuf = Buf<T, false>;
template <class T> using PinnedBuf = Buf<T, true>;

}  // namespace csi_host
