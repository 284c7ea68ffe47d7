/*
 * gsdf_mesh_index.hip -- the indexed iso-surface mesh (gsdf_extract_mesh_indexed, include/gsdf.h): the triangles of
 * gsdf_extract_mesh with one vertex per crossed grid edge, faces as indices and a normal per vertex from the stored gradients.
 *
 *   k_mesh_corners   k_mesh (gsdf_kernels.hip) once more, unchanged in what it keeps and in what order of operations it
 *                    interpolates; per kept triangle it also writes, for each of the three corners, the key of the grid edge
 *                    the corner lies on and a word holding interpolate's mu and the direction the cube walked that edge in
 *   order            radix sort of (sweep key, triangle) as gsdf_extract_mesh (gsdf_sort.hip): the soup's order
 *   k_corner_keys    the edge keys in that order, with the corner rank 3 face + corner beside them
 *   weld             STABLE radix sort of (edge key, corner rank): a run of equal keys is one vertex and starts with its
 *                    canonical corner (the first in sweep order); k_run_heads flags the run starts, their exclusive scan
 *                    numbers the vertices in ascending key order
 *   k_weld           faces[corner rank] = vertex id; the run start hands its position, edge key and mu word to the vertex
 *   k_vertex_normals one lane per vertex: the two endpoint voxels through gsdf_find, their unit gradients blended with mu
 *
 * No floating-point atomics and no sums whose order depends on the launch: k_mesh_corners appends in any order, the two sorts
 * (keys unique per triangle / ties broken by the rank under a stable sort) remove it again.  rocPRIM's sort and scan are
 * library primitives as in gsdf_sort.hip.
 */
#include "gsdf_kernels.h"
#include "gsdf_math.h"

#include <rocprim/device/device_scan.hpp>

/* KEPT BY HAND: mesh_mu restates the guards and the quotient of mesh_interpolate (gsdf_math.h), k_mesh_corners restates k_mesh
 * (gsdf_kernels.hip) -- corner gather, interpolation, degenerate rule, sweep key.  Change either only together with its original;
 * tests/test_gpu_indexed_mesh.py holds faces and positions to the soup bit for bit. */
/* interpolate's mu as a float (mesh_interpolate, gsdf_math.h: a float quotient held in a double and clamped -- the clamp keeps
 * it a float): 0 where it returns v0 through a 1e-7 guard, 1 where it returns v1 */
__device__ __forceinline__ float mesh_mu(float t0, float t1, float iso) {
    if (fabs((double)(iso - t0)) < 1e-7) return 0.f;
    if (fabs((double)(iso - t1)) < 1e-7) return 1.f;
    if (fabs((double)(t0 - t1)) < 1e-7) return 0.f;
    const float mu = (iso - t0) / (t1 - t0);
    return mu > 1.f ? 1.f : (mu < 0.f ? 0.f : mu);
}

__global__ __launch_bounds__(256) void k_mesh_corners(gsdf_table tab, size_t n_slots, float vs, float iso, const int* __restrict__ mn,
                                                       const signed char* __restrict__ tri_table, float* __restrict__ tris,
                                                       unsigned long long* __restrict__ keys, unsigned long long* __restrict__ ekeys,
                                                       uint32_t* __restrict__ muw, unsigned long long* counter, long long max_tris) {
    /* corner c -> (dx, dy, dz), numbering of computeLutIndex (:599-606); edge e -> its two corners (k_mesh's tables) */
    const int CORNER[8][3] = { { 1, 1, 0 }, { 1, 0, 0 }, { 0, 0, 0 }, { 0, 1, 0 }, { 1, 1, 1 }, { 1, 0, 1 }, { 0, 0, 1 }, { 0, 1, 1 } };
    const int EDGE[12][2] = { { 0, 1 }, { 1, 2 }, { 2, 3 }, { 3, 0 }, { 4, 5 }, { 5, 6 }, { 6, 7 }, { 7, 4 }, { 0, 4 }, { 1, 5 }, { 2, 6 }, { 3, 7 } };
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const int m0 = mn[0], m1 = mn[1], m2 = mn[2];
    const float o0 = -(float)m0 * vs, o1 = -(float)m1 * vs, o2 = -(float)m2 * vs;     /* origin_ (:377) */
    for (; i < n_slots; i += stride) {
        const unsigned long long bk = tab.bkeys[i / GSDF_BLOCK_VOX];
        if (bk == GSDF_KEY_EMPTY) continue;
        const gsdf_payload self = tab.vox[i];
        if (!(self.w > 0.f)) continue;
        int x, y, z;
        gsdf_key_unpack(gsdf_voxel_key(bk, (uint32_t)(i % GSDF_BLOCK_VOX)), &x, &y, &z);
        float d[8];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c == 2) { d[c] = self.s / self.w; continue; }
            const int cx = x + CORNER[c][0], cy = y + CORNER[c][1], cz = z + CORNER[c][2];
            const gsdf_payload* q = gsdf_key_in_range(cx, cy, cz) ? gsdf_find(tab, gsdf_key_pack(cx, cy, cz)) : nullptr;
            float w = 0.f, sd = 0.f;
            if (q) { const float2 ws = *reinterpret_cast<const float2*>(q); w = ws.x; sd = ws.y; }
            if (!(w > 0.f)) ok = false;
            d[c] = ok ? sd / w : 0.f;
        }
        if (!ok) continue;
        int idx = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c) if (d[c] > iso) idx |= 1 << c;
        if (idx == 0 || idx == 255) continue;
        const signed char* t = tri_table + 16 * idx;
        for (int k = 0; k < 15 && t[k] >= 0; k += 3) {
            gsdf_v3 p[3];
            unsigned long long ek[3];
            uint32_t mw[3];
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                const int e = t[k + v], a = EDGE[e][0], b = EDGE[e][1];
                const gsdf_v3 wa = { (float)(x + CORNER[a][0] - m0) * vs - o0, (float)(y + CORNER[a][1] - m1) * vs - o1,
                                     (float)(z + CORNER[a][2] - m2) * vs - o2 };
                const gsdf_v3 wb = { (float)(x + CORNER[b][0] - m0) * vs - o0, (float)(y + CORNER[b][1] - m1) * vs - o1,
                                     (float)(z + CORNER[b][2] - m2) * vs - o2 };
                p[v] = mesh_interpolate(d[a], d[b], wa, wb, iso);
                /* the grid edge: its lower endpoint (z, y, x relative to the bounding-box minimum, 20 bits each, as the sweep
                 * key) and its axis; the two corners of a cube edge differ in exactly one coordinate */
                const int axis = CORNER[a][0] != CORNER[b][0] ? 0 : (CORNER[a][1] != CORNER[b][1] ? 1 : 2);
                const int lx = x + min(CORNER[a][0], CORNER[b][0]) - m0, ly = y + min(CORNER[a][1], CORNER[b][1]) - m1,
                          lz = z + min(CORNER[a][2], CORNER[b][2]) - m2;
                ek[v] = ((((unsigned long long)(uint32_t)lz << 40) | ((unsigned long long)(uint32_t)ly << 20) |
                          (unsigned long long)(uint32_t)lx) << 2) | (unsigned long long)axis;
                /* mu (>= 0: the sign bit is free) | bit 31: the cube walks the edge downwards, a is the upper endpoint */
                mw[v] = __float_as_uint(mesh_mu(d[a], d[b], iso)) | ((uint32_t)CORNER[a][axis] << 31);
            }
            auto same = [](const gsdf_v3& a, const gsdf_v3& b) { return a.x == b.x && a.y == b.y && a.z == b.z; };
            if (same(p[0], p[1]) || same(p[0], p[2]) || same(p[1], p[2])) continue;      /* computeTriangles (:686-712) */
            const unsigned long long o = atomicAdd(counter, 1ull);
            if ((long long)o >= max_tris) continue;
            float* out = tris + 9 * o;
#pragma unroll
            for (int v = 0; v < 3; ++v) {
                out[3 * v] = p[v].x; out[3 * v + 1] = p[v].y; out[3 * v + 2] = p[v].z;
                ekeys[3 * o + v] = ek[v]; muw[3 * o + v] = mw[v];
            }
            keys[o] = ((((unsigned long long)(uint32_t)(z - m2) << 40) | ((unsigned long long)(uint32_t)(y - m1) << 20) |
                        (unsigned long long)(uint32_t)(x - m0)) << 3) | (unsigned long long)(k / 3);
        }
    }
}
void gsdf_launch_mesh_corners(hipStream_t s, gsdf_table tab, size_t n_slots, float vs, float iso, const int* mn_dev,
                              const signed char* tri_table_dev, float* tris_dev, unsigned long long* keys_dev,
                              unsigned long long* ekeys_dev, uint32_t* muw_dev, unsigned long long* counter, long long max_tris) {
    hipLaunchKernelGGL(k_mesh_corners, dim3(2048), dim3(256), 0, s, tab, n_slots, vs, iso, mn_dev, tri_table_dev, tris_dev, keys_dev,
                       ekeys_dev, muw_dev, counter, max_tris);
}

/* corner i = 3 t + v of the soup (t in sweep order): its edge key, and its rank i as the sort's value */
__global__ __launch_bounds__(256) void k_corner_keys(const unsigned long long* __restrict__ ekeys, const uint32_t* __restrict__ order,
                                                      unsigned long long* __restrict__ out, uint32_t* __restrict__ rank, size_t n_tris) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tris * 3) return;
    const size_t t = i / 3, v = i - t * 3;
    out[i] = ekeys[(size_t)order[t] * 3 + v];
    rank[i] = (uint32_t)i;
}
void gsdf_launch_corner_keys(hipStream_t s, const unsigned long long* ekeys, const uint32_t* order, unsigned long long* out,
                             uint32_t* rank, size_t n_tris) {
    if (n_tris) hipLaunchKernelGGL(k_corner_keys, dim3((unsigned int)((n_tris * 3 + 255) / 256)), dim3(256), 0, s, ekeys, order, out, rank, n_tris);
}

__global__ __launch_bounds__(256) void k_run_heads(const unsigned long long* __restrict__ sorted, uint32_t* __restrict__ heads, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) heads[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
}
/* heads[i] = corner i of the sorted list starts a run of equal keys; before[i] = run starts in front of i */
hipError_t gsdf_run_heads_scan_need(size_t n, size_t* need) {
    return gsdf_scratch_need(need, [n](size_t& b) { return rocprim::exclusive_scan(nullptr, b, (uint32_t*)0, (uint32_t*)0, 0u, n, rocprim::plus<uint32_t>(), hipStream_t()); });
}
hipError_t gsdf_run_heads_scan(const gsdf_dev<void>& tmp, const unsigned long long* sorted, uint32_t* heads, uint32_t* before, size_t n,
                               hipStream_t s) {
    if (n) hipLaunchKernelGGL(k_run_heads, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, sorted, heads, n);
    size_t b = tmp.bytes();
    return rocprim::exclusive_scan(tmp.get(), b, heads, before, 0u, n, rocprim::plus<uint32_t>(), s);
}

/* one lane per corner of the sorted list */
__global__ __launch_bounds__(256) void k_weld(const unsigned long long* __restrict__ sorted, const uint32_t* __restrict__ rank,
                                               const uint32_t* __restrict__ heads, const uint32_t* __restrict__ before,
                                               const uint32_t* __restrict__ order, const float* __restrict__ tris,
                                               const uint32_t* __restrict__ muw, size_t n, int32_t* __restrict__ faces,
                                               float* __restrict__ vertices, unsigned long long* __restrict__ vkeys,
                                               uint32_t* __restrict__ vmuw) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t head = heads[i], id = before[i] + head - 1u, r = rank[i];
    faces[r] = (int32_t)id;
    if (!head) return;
    const size_t src = (size_t)order[r / 3] * 3 + r % 3;          /* the canonical corner where k_mesh_corners left it */
    vertices[3 * (size_t)id] = tris[3 * src]; vertices[3 * (size_t)id + 1] = tris[3 * src + 1]; vertices[3 * (size_t)id + 2] = tris[3 * src + 2];
    vkeys[id] = sorted[i];
    vmuw[id] = muw[src];
}
void gsdf_launch_weld(hipStream_t s, const unsigned long long* sorted, const uint32_t* rank, const uint32_t* heads, const uint32_t* before,
                      const uint32_t* order, const float* tris, const uint32_t* muw, size_t n_corners, int32_t* faces, float* vertices,
                      unsigned long long* vkeys, uint32_t* vmuw) {
    if (n_corners)
        hipLaunchKernelGGL(k_weld, dim3((unsigned int)((n_corners + 255) / 256)), dim3(256), 0, s, sorted, rank, heads, before, order, tris, muw,
                           n_corners, faces, vertices, vkeys, vmuw);
}

/* g^ of a voxel: the normalised stored gradient sum, as k_query normalises it; 0 for a voxel that does not exist */
__device__ __forceinline__ gsdf_v3 mesh_unit_gradient(const gsdf_table& tab, int x, int y, int z) {
    const gsdf_payload* q = gsdf_key_in_range(x, y, z) ? gsdf_find(tab, gsdf_key_pack(x, y, z)) : nullptr;
    if (!q || !(q->w > 0.f)) return gsdf_v3{ 0.f, 0.f, 0.f };
    return gsdf_normalized3(gsdf_v3{ q->gx, q->gy, q->gz });
}

/* n = -normalized((1 - mu) g^_a + mu g^_b) over the canonical corner's endpoints a -> b, in float; (0, 0, 0) when the blend
 * has no direction (norm 0 or not finite) */
__global__ __launch_bounds__(256) void k_vertex_normals(gsdf_table tab, const int* __restrict__ mn, const unsigned long long* __restrict__ vkeys,
                                                         const uint32_t* __restrict__ vmuw, size_t n, float* __restrict__ normals) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned long long ek = vkeys[i], q = ek >> 2;
    const int axis = (int)(ek & 3ull);
    const int lx = (int)(q & 0xFFFFFull) + mn[0], ly = (int)((q >> 20) & 0xFFFFFull) + mn[1], lz = (int)(q >> 40) + mn[2];
    const int ux = lx + (axis == 0), uy = ly + (axis == 1), uz = lz + (axis == 2);
    const uint32_t w = vmuw[i];
    const bool down = (w >> 31) != 0u;
    const float mu = __uint_as_float(w & 0x7FFFFFFFu);
    const gsdf_v3 glo = mesh_unit_gradient(tab, lx, ly, lz), gup = mesh_unit_gradient(tab, ux, uy, uz);
    const gsdf_v3 ga = down ? gup : glo, gb = down ? glo : gup;
    const float wa = 1.f - mu;
    const gsdf_v3 b = { wa * ga.x + mu * gb.x, wa * ga.y + mu * gb.y, wa * ga.z + mu * gb.z };
    const float zz = gsdf_sum3(b.x * b.x, b.y * b.y, b.z * b.z);
    gsdf_v3 o = { 0.f, 0.f, 0.f };
    if (zz > 0.f && zz <= 3.4028234e38f) {                         /* (a NaN fails the first test) */
        const float s = sqrtf(zz);
        o = gsdf_v3{ -(b.x / s), -(b.y / s), -(b.z / s) };
    }
    normals[3 * i] = o.x; normals[3 * i + 1] = o.y; normals[3 * i + 2] = o.z;
}
void gsdf_launch_vertex_normals(hipStream_t s, gsdf_table tab, const int* mn_dev, const unsigned long long* vkeys, const uint32_t* vmuw,
                                size_t n_vertices, float* normals) {
    if (n_vertices)
        hipLaunchKernelGGL(k_vertex_normals, dim3((unsigned int)((n_vertices + 255) / 256)), dim3(256), 0, s, tab, mn_dev, vkeys, vmuw,
                           n_vertices, normals);
}
