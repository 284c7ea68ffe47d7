/*
 * gsdf_sweep.h -- host side of the entries that sweep the map into buffers of the exact size: the counted pass, the total of a
 * scan, the order of a sweep's keys.  (The rocPRIM scratch idiom, X_need / X, is declared in gsdf_kernels.h.)  Host only.
 */
#ifndef GSDF_SWEEP_H_
#define GSDF_SWEEP_H_

#include "gsdf_ctx.h"

/* c->counter, through which a sweep appends: zeroed on the stream / its 8-byte read enqueued (the caller waits for the stream) */
inline hipError_t gsdf_counter_zero(gsdf_ctx* c) { return hipMemsetAsync(c->counter, 0, sizeof(unsigned long long), c->stream); }
inline hipError_t gsdf_counter_read(gsdf_ctx* c, unsigned long long* n) { return hipMemcpyAsync(n, c->counter, sizeof(*n), hipMemcpyDeviceToHost, c->stream); }
/* the counted pass: `launch` enqueues a sweep that counts (and, given room, appends) through c->counter; *n = its count */
template <class Launch>
hipError_t gsdf_counted(gsdf_ctx* c, Launch&& launch, unsigned long long* n) {
    hipError_t e = gsdf_counter_zero(c);
    if (e != hipSuccess) return e;
    launch();
    if ((e = hipGetLastError()) != hipSuccess || (e = gsdf_counter_read(c, n)) != hipSuccess) return e;
    return hipStreamSynchronize(c->stream);
}

/* enqueues the copies of before[n - 1] and flags[n - 1] (n > 0), `before` the exclusive scan of `flags`: once the caller has
 * waited for the stream, last[0] + last[1] is the total */
inline hipError_t gsdf_scan_total_read(hipStream_t s, const uint32_t* before, const uint32_t* flags, size_t n, uint32_t last[2]) {
    const hipError_t e = hipMemcpyAsync(&last[0], before + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    return e != hipSuccess ? e : hipMemcpyAsync(&last[1], flags + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s);
}

/* The order of n sweep keys: skeys = the keys ascending, order[i] = where the i-th of them stood (stable).  Owns the sort's
 * buffers and scratch; a `need` raised by other X_need calls makes the scratch serve those prims of the caller as well. */
struct gsdf_key_order {
    gsdf_dev<unsigned long long> skeys;
    gsdf_dev<uint32_t> idx, order;
    gsdf_dev<void> tmp;
    hipError_t alloc(size_t n, size_t need = 0) {
        hipError_t e;
        if ((e = skeys.alloc(n)) != hipSuccess || (e = idx.alloc(n)) != hipSuccess || (e = order.alloc(n)) != hipSuccess ||
            (e = gsdf_sort_pairs_u64_need(n, &need)) != hipSuccess) return e;
        return tmp.alloc(need);
    }
    hipError_t run(gsdf_ctx* c, const unsigned long long* keys, size_t n) {
        gsdf_launch_iota(c->stream, idx, n);
        return gsdf_sort_pairs_u64(tmp, keys, skeys, idx, order, n, c->stream);
    }
};

#endif /* GSDF_SWEEP_H_ */
