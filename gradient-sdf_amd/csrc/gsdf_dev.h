/*
 * gsdf_dev.h -- the owners of the memory libgsdf.so allocates for itself: gsdf_dev<T> (device) and gsdf_pinned<T> (mapped host
 * words).  Move-only; the destructor frees.  Memory handed to the CALLER (gsdf_dev_alloc, gsdf_host_alloc) does not come from here.
 */
#ifndef GSDF_DEV_H_
#define GSDF_DEV_H_

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#ifdef GSDF_EXPERIMENTS
/* gsdf_debug_fail_alloc (test build): owned allocations since its last call, and which of them is to fail (0 = none) */
inline int g_gsdf_alloc_count = 0, g_gsdf_alloc_fail_at = 0;
#endif

template <class T> struct gsdf_elem_size { static constexpr size_t value = sizeof(T); };
template <> struct gsdf_elem_size<void> { static constexpr size_t value = 1; };     /* gsdf_dev<void> counts bytes */

/* `count` elements of device memory.  Reads as a T* wherever one is expected.  An owner released while work is still queued on
 * its buffer is safe: hipFree waits for the device. */
template <class T>
class gsdf_dev {
    T* p_ = nullptr;
    size_t n_ = 0;
public:
    gsdf_dev() = default;
    gsdf_dev(gsdf_dev&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }      /* (move-only: no copies) */
    gsdf_dev& operator=(gsdf_dev&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~gsdf_dev() { reset(); }

    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    T* get() const { return p_; }
    template <class U> U* as() const { return (U*)p_; }
    size_t count() const { return n_; }
    size_t bytes() const { return n_ * gsdf_elem_size<T>::value; }

    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
    /* releases what it holds, then allocates `count` elements (at least one) */
    hipError_t alloc(size_t count) {
        reset();
        if (count == 0) count = 1;
#ifdef GSDF_EXPERIMENTS
        if (++g_gsdf_alloc_count == g_gsdf_alloc_fail_at) { g_gsdf_alloc_fail_at = 0; return hipErrorOutOfMemory; }
#endif
        const hipError_t e = hipMalloc((void**)&p_, count * gsdf_elem_size<T>::value);
        if (e == hipSuccess) n_ = count; else p_ = nullptr;
        return e;
    }
    /* keeps a buffer that is large enough (contents and all); otherwise alloc(count): the old contents are gone */
    hipError_t grow(size_t count) { return p_ && count <= n_ ? hipSuccess : alloc(count); }
};

/* `count` zeroed words of pinned host memory that kernels write through dev(); the host reads them as volatile */
template <class T>
class gsdf_pinned {
    volatile T* p_ = nullptr;
    T* dev_ = nullptr;
public:
    gsdf_pinned() = default;
    gsdf_pinned(const gsdf_pinned&) = delete;
    gsdf_pinned& operator=(const gsdf_pinned&) = delete;
    ~gsdf_pinned() { reset(); }

    operator volatile T*() const { return p_; }
    T* dev() const { return dev_; }

    void reset() {
        if (p_) (void)hipHostFree((void*)p_);
        p_ = nullptr; dev_ = nullptr;
    }
    hipError_t alloc(size_t count) {
        reset();
        void *hp = nullptr, *dp = nullptr;
        hipError_t e = hipHostMalloc(&hp, count * sizeof(T), hipHostMallocMapped);
        if (e != hipSuccess) return e;
        std::memset(hp, 0, count * sizeof(T));
        if ((e = hipHostGetDevicePointer(&dp, hp, 0)) != hipSuccess) { (void)hipHostFree(hp); return e; }
        p_ = (volatile T*)hp; dev_ = (T*)dp;
        return hipSuccess;
    }
};

#endif /* GSDF_DEV_H_ */
