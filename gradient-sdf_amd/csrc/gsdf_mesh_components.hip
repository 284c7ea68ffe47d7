/*
 * gsdf_mesh_components.hip -- connected components of the indexed iso-surface mesh and the removal of small ones
 * (gsdf_mesh_components, gsdf_extract_mesh_indexed_filtered, include/gsdf.h), on the welded arrays of gsdf_mesh_index.hip while
 * they are on the device.
 *
 *   k_cc_init        parent[v] = v
 *   k_cc_union       one lane per face, union(v0, v1) and union(v1, v2) in ONE lock-free pass: find with path halving, then a
 *                    compare-and-swap that hooks the LARGER root under the smaller.  parent[v] <= v always, only a root is ever
 *                    hooked, so the root of a finished component is its smallest vertex id whatever the order of the lanes
 *   k_cc_roots       (next launch) root[v] = the root of v, flag[v] = (root[v] == v): the full compression, into a second array,
 *                    so the pass reads parent[] and writes nothing it reads
 *   scan             rocPRIM exclusive scan of the flags: a root's count of roots in front of it is its component id -- ascending
 *                    root is ascending smallest vertex
 *   k_cc_vertices    vertex_comp[v] = id of root[v]; vertex count and bounding box of the component
 *   k_cc_faces       face_comp[f] = vertex_comp of its first vertex; face count of the component
 *   k_cc_keep / k_cc_largest   the keep mask from the face counts, and the number kept
 *   k_cc_keep_flags  the mask per vertex and per face; their exclusive scans are the new ids
 *   k_cc_compact_*   kept vertices (position and normal bytes as they are) and kept faces (ids remapped), order preserved
 *
 * No wave waits for another workgroup anywhere: there is no flag to spin on and no barrier across workgroups.  Every loop of
 * k_cc_union ends because the value it follows strictly decreases: find walks parent[x] < x, and a compare-and-swap fails only
 * when another lane has lowered parent[root] below root, which can happen at most `root` times.
 *
 * Visibility (MI355X: eight XCDs with private L2s, an L1 per CU that no other CU's store refreshes): inside k_cc_union every read
 * and write of parent[] is a relaxed atomic at agent scope -- a plain load could return a line cached before another XCD's
 * hook.  Nothing else is exchanged inside a launch; every later step reads what an EARLIER launch wrote.
 *
 * No floating-point sums.  Counts are integer atomicAdd, the box goes through atomicMin / atomicMax on an order-preserving
 * integer image of the float: neither depends on the order of the lanes.
 */
#include "gsdf_kernels.h"

#include <rocprim/device/device_scan.hpp>

#define CC_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

__global__ __launch_bounds__(256) void k_cc_init(uint32_t* __restrict__ parent, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
}

/* the root of x as parent[] stands; on the way every visited node is pointed at its grandparent (fetch_min: a concurrent lane may
 * have pointed it lower already, and it stays there).  x strictly decreases */
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
    uint32_t p = CC_LOAD(parent + x);
    while (p != x) {
        const uint32_t gp = CC_LOAD(parent + p);
        if (gp != p) __hip_atomic_fetch_min(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p; p = gp;
    }
    return x;
}

__device__ __forceinline__ void cc_union(uint32_t* parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        uint32_t expected = a;                                /* a is still a root: hook it under the smaller root b */
        if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        /* another lane hooked a first (parent[a] < a now): look again from where a and b have got to */
    }
}

__global__ __launch_bounds__(256) void k_cc_union(const int32_t* __restrict__ faces, size_t n_faces, uint32_t* parent) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= n_faces) return;
    const uint32_t v0 = (uint32_t)faces[3 * f], v1 = (uint32_t)faces[3 * f + 1], v2 = (uint32_t)faces[3 * f + 2];
    cc_union(parent, v0, v1);
    cc_union(parent, v1, v2);
}

__global__ __launch_bounds__(256) void k_cc_roots(const uint32_t* __restrict__ parent, size_t n, uint32_t* __restrict__ root,
                                                   uint32_t* __restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    root[i] = x;
    flags[i] = x == (uint32_t)i ? 1u : 0u;
}

void gsdf_launch_cc_label(hipStream_t s, const int32_t* faces, size_t n_faces, size_t n_vertices, uint32_t* parent, uint32_t* root,
                          uint32_t* flags) {
    if (!n_vertices) return;
    const dim3 gv((unsigned int)((n_vertices + 255) / 256)), b(256);
    hipLaunchKernelGGL(k_cc_init, gv, b, 0, s, parent, n_vertices);
    if (n_faces) hipLaunchKernelGGL(k_cc_union, dim3((unsigned int)((n_faces + 255) / 256)), b, 0, s, faces, n_faces, parent);
    hipLaunchKernelGGL(k_cc_roots, gv, b, 0, s, parent, n_vertices, root, flags);
}

hipError_t gsdf_scan_u32_need(size_t n, size_t* need) {
    return gsdf_scratch_need(need, [n](size_t& b) { return rocprim::exclusive_scan(nullptr, b, (const uint32_t*)0, (uint32_t*)0, 0u, n, rocprim::plus<uint32_t>(), hipStream_t()); });
}
hipError_t gsdf_scan_u32(const gsdf_dev<void>& tmp, const uint32_t* in, uint32_t* out, size_t n, hipStream_t s) {
    size_t b = tmp.bytes();
    return rocprim::exclusive_scan(tmp.get(), b, in, out, 0u, n, rocprim::plus<uint32_t>(), s);
}

/* a float as an unsigned whose order is the float's (-0 below +0; a NaN sorts beyond the infinity of its sign) */
__device__ __forceinline__ uint32_t cc_ordered(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cc_unordered(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__global__ __launch_bounds__(256) void k_cc_box_init(uint32_t* __restrict__ box, size_t n_comp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_comp * 6) box[i] = (i % 6) < 3 ? 0xFFFFFFFFu : 0u;
}

/* The lanes of a wave that hold one component add to its counters ONCE: faces and vertices come in sweep order, so a wave sees
 * one component, seldom two, and a mesh that is one large component would otherwise send every lane to the same address.  The
 * loop is uniform over the wave (todo is a ballot): each turn takes the component of the first lane left and all lanes equal to
 * it.  Integer sums and minima: grouping changes nothing in the result. */
__device__ __forceinline__ uint32_t cc_wave_min(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}
__device__ __forceinline__ uint32_t cc_wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d));
    return v;
}

__global__ __launch_bounds__(256) void k_cc_vertices(const uint32_t* __restrict__ root, const uint32_t* __restrict__ before,
                                                      const float* __restrict__ vertices, size_t n, int32_t* __restrict__ vcomp,
                                                      int32_t* counts, uint32_t* box) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool act = i < n;
    const uint32_t c = act ? before[root[i]] : 0xFFFFFFFFu;
    uint32_t o[3] = { 0u, 0u, 0u };
    if (act) {
        vcomp[i] = (int32_t)c;
        if (box) { o[0] = cc_ordered(vertices[3 * i]); o[1] = cc_ordered(vertices[3 * i + 1]); o[2] = cc_ordered(vertices[3 * i + 2]); }
    }
    unsigned long long todo = __ballot(act);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t lc = (uint32_t)__shfl((int)c, leader);
        const bool mine = act && c == lc;
        const unsigned long long grp = __ballot(mine);
        if (lane == leader) atomicAdd(counts + 2 * (size_t)lc + 1, (int32_t)__popcll(grp));
        if (box) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t lo = cc_wave_min(mine ? o[k] : 0xFFFFFFFFu), hi = cc_wave_max(mine ? o[k] : 0u);
                if (lane == leader) { atomicMin(box + 6 * (size_t)lc + k, lo); atomicMax(box + 6 * (size_t)lc + 3 + k, hi); }
            }
        }
        todo &= ~grp;
    }
}

__global__ __launch_bounds__(256) void k_cc_faces(const int32_t* __restrict__ faces, const int32_t* __restrict__ vcomp, size_t n,
                                                   int32_t* __restrict__ fcomp, int32_t* counts) {
    const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool act = f < n;
    const int32_t c = act ? vcomp[faces[3 * f]] : -1;
    if (act) fcomp[f] = c;
    unsigned long long todo = __ballot(act);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t lc = __shfl(c, leader);
        const unsigned long long grp = __ballot(act && c == lc);
        if (lane == leader) atomicAdd(counts + 2 * (size_t)lc, (int32_t)__popcll(grp));
        todo &= ~grp;
    }
}

__global__ __launch_bounds__(256) void k_cc_box_decode(const uint32_t* __restrict__ box, size_t n_comp, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_comp * 6) out[i] = cc_unordered(box[i]);
}

void gsdf_launch_cc_tables(hipStream_t s, const int32_t* faces, const float* vertices, const uint32_t* root, const uint32_t* before,
                           size_t n_faces, size_t n_vertices, size_t n_comp, int32_t* vcomp, int32_t* fcomp, int32_t* counts,
                           uint32_t* box_bits, float* box) {
    if (!n_vertices || !n_comp) return;
    const dim3 b(256), gb((unsigned int)((n_comp * 6 + 255) / 256));
    (void)hipMemsetAsync(counts, 0, n_comp * 2 * sizeof(int32_t), s);
    if (box_bits) hipLaunchKernelGGL(k_cc_box_init, gb, b, 0, s, box_bits, n_comp);
    hipLaunchKernelGGL(k_cc_vertices, dim3((unsigned int)((n_vertices + 255) / 256)), b, 0, s, root, before, vertices, n_vertices, vcomp,
                       counts, box_bits);
    if (n_faces) hipLaunchKernelGGL(k_cc_faces, dim3((unsigned int)((n_faces + 255) / 256)), b, 0, s, faces, vcomp, n_faces, fcomp, counts);
    if (box_bits) hipLaunchKernelGGL(k_cc_box_decode, gb, b, 0, s, box_bits, n_comp, box);
}

__global__ __launch_bounds__(256) void k_cc_keep(const int32_t* __restrict__ counts, size_t n_comp, long long min_faces,
                                                  uint32_t* __restrict__ keep, uint32_t* n_kept) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_comp) return;
    const uint32_t k = (long long)counts[2 * i] >= min_faces ? 1u : 0u;
    keep[i] = k;
    if (k) atomicAdd(n_kept, 1u);
}

/* the component with the most faces, the lowest id among equals: ONE workgroup; (faces, id) is a total order, so neither the
 * strided walk nor the tree changes which one wins */
__global__ __launch_bounds__(256) void k_cc_largest(const int32_t* __restrict__ counts, size_t n_comp, uint32_t* __restrict__ keep,
                                                     uint32_t* n_kept) {
    __shared__ int32_t s_cnt[256];
    __shared__ uint32_t s_id[256];
    const auto better = [](int32_t ca, uint32_t ia, int32_t cb, uint32_t ib) { return ca > cb || (ca == cb && ia < ib); };
    int32_t best = -1;
    uint32_t id = 0xFFFFFFFFu;
    for (size_t i = threadIdx.x; i < n_comp; i += 256)
        if (better(counts[2 * i], (uint32_t)i, best, id)) { best = counts[2 * i]; id = (uint32_t)i; }
    s_cnt[threadIdx.x] = best; s_id[threadIdx.x] = id;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w && better(s_cnt[threadIdx.x + w], s_id[threadIdx.x + w], s_cnt[threadIdx.x], s_id[threadIdx.x])) {
            s_cnt[threadIdx.x] = s_cnt[threadIdx.x + w]; s_id[threadIdx.x] = s_id[threadIdx.x + w];
        }
        __syncthreads();
    }
    const uint32_t win = s_id[0];
    for (size_t i = threadIdx.x; i < n_comp; i += 256) keep[i] = (uint32_t)i == win ? 1u : 0u;
    if (threadIdx.x == 0) *n_kept = 1u;
}

void gsdf_launch_cc_keep(hipStream_t s, const int32_t* counts, size_t n_comp, long long min_faces, uint32_t* keep, uint32_t* n_kept) {
    (void)hipMemsetAsync(n_kept, 0, sizeof(uint32_t), s);
    if (!n_comp) return;
    if (min_faces < 0) hipLaunchKernelGGL(k_cc_largest, dim3(1), dim3(256), 0, s, counts, n_comp, keep, n_kept);
    else hipLaunchKernelGGL(k_cc_keep, dim3((unsigned int)((n_comp + 255) / 256)), dim3(256), 0, s, counts, n_comp, min_faces, keep, n_kept);
}

__global__ __launch_bounds__(256) void k_cc_keep_flags(const int32_t* __restrict__ comp, const uint32_t* __restrict__ keep, size_t n,
                                                        uint32_t* __restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) flags[i] = keep[comp[i]];
}
void gsdf_launch_cc_keep_flags(hipStream_t s, const int32_t* comp, const uint32_t* keep, size_t n, uint32_t* flags) {
    if (n) hipLaunchKernelGGL(k_cc_keep_flags, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, comp, keep, n, flags);
}

/* one lane per float of a kept vertex's position (and normal): the bytes as they are */
__global__ __launch_bounds__(256) void k_cc_compact_vertices(const float* __restrict__ v, const float* __restrict__ nrm,
                                                              const uint32_t* __restrict__ flags, const uint32_t* __restrict__ before,
                                                              size_t n, float* __restrict__ v_out, float* __restrict__ n_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 3) return;
    const size_t j = i / 3, k = i - j * 3;
    if (!flags[j]) return;
    const size_t o = 3 * (size_t)before[j] + k;
    v_out[o] = v[i];
    if (n_out) n_out[o] = nrm[i];
}
/* one lane per corner of a kept face: the new id of its vertex (kept with the face: they are in one component) */
__global__ __launch_bounds__(256) void k_cc_compact_faces(const int32_t* __restrict__ faces, const uint32_t* __restrict__ flags,
                                                           const uint32_t* __restrict__ before, const uint32_t* __restrict__ vbefore,
                                                           size_t n, int32_t* __restrict__ f_out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 3) return;
    const size_t j = i / 3, k = i - j * 3;
    if (!flags[j]) return;
    f_out[3 * (size_t)before[j] + k] = (int32_t)vbefore[faces[i]];
}
void gsdf_launch_cc_compact(hipStream_t s, const float* v, const float* nrm, const int32_t* faces, const uint32_t* vflags,
                            const uint32_t* vbefore, const uint32_t* fflags, const uint32_t* fbefore, size_t n_vertices, size_t n_faces,
                            float* v_out, float* n_out, int32_t* f_out) {
    if (n_vertices)
        hipLaunchKernelGGL(k_cc_compact_vertices, dim3((unsigned int)((n_vertices * 3 + 255) / 256)), dim3(256), 0, s, v, nrm, vflags, vbefore,
                           n_vertices, v_out, n_out);
    if (n_faces)
        hipLaunchKernelGGL(k_cc_compact_faces, dim3((unsigned int)((n_faces * 3 + 255) / 256)), dim3(256), 0, s, faces, fflags, fbefore, vbefore,
                           n_faces, f_out);
}
