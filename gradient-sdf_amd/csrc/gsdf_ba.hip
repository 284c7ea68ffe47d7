/*
 * gsdf_ba.hip -- PhotoBA on the GPU: the three voxel sweeps of PhotometricOptimizer
 * (ps_optimizer/PhotometricOptimizer.cpp) over the HBM voxel table.
 *
 *   k_ba_energy  getEnergy   :273-321   sum over voxels (|dist| <= voxel size) of sum_i |A_ij - mean_j|^2
 *   k_ba_pose    solvePose   :499-590   per keyframe b_i (6) and H_i (6x6) of the photoconsistency residual
 *   k_ba_dist    solveDist   :326-388   per-voxel scalar Gauss-Newton step on the distance
 *
 * One lane = one voxel slot; every lane loops over the keyframes it is visible in (vis_ bit-vectors),
 * projects its surface point c - dist * g^ into the keyframe and samples the float BGR image
 * bilinearly.  The work is embarrassingly parallel over voxels; the only reductions are the energy and
 * the 27 numbers per keyframe, reduced per wave (DPP), per workgroup (LDS) and across workgroups in a
 * fixed order by a second small kernel, so results are deterministic.
 */
#include "gsdf_kernels.h"
#include "gsdf_math.h"
#include "gsdf_interp.h"
#include "gsdf_ba_shared.h"
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float ba_dpp_add(float v) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
    return v + __int_as_float(moved);
}
template <int N>
__device__ __forceinline__ void ba_wave_sum_to_lane63(float (&v)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ba_dpp_add<0x111, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ba_dpp_add<0x112, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ba_dpp_add<0x114, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ba_dpp_add<0x118, 0xf>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ba_dpp_add<0x142, 0xa>(v[i]);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = ba_dpp_add<0x143, 0xc>(v[i]);
}

/* ---- getEnergy ---- */
/* block_E: [3][gridDim.x] -- the workgroup's energy, its voxels that took part (|dist| <= vs, seen by >= 1 keyframe) and their
 * observations (voxel x keyframe pairs that project into the image): the counts are the units of the sweep's algorithmic bytes */
template <bool WRITE_MEAN>
__global__ __launch_bounds__(256) void k_ba_energy(ba_args a, double* block_E) {
    __shared__ double red[3][4];
    double E = 0.0;
    unsigned int n_act = 0u, n_obs = 0u;
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t n_items = a.gate_list ? (size_t)*a.gate_count : a.n_slots;
    ba_mean* const mc = WRITE_MEAN ? static_cast<ba_mean*>(a.mean_cache) : nullptr;      /* (WRITE_MEAN: the gate list is in use) */
    for (size_t item = (size_t)blockIdx.x * 256 + threadIdx.x; item < n_items; item += stride) {
        const size_t slot = a.gate_list ? (size_t)a.gate_list[item] : item;
        ba_voxel v;
        bool ok = ba_load_voxel(a, slot, &v);
        ok = ok && !(fabsf(v.dist) > a.vs);                                   /* :285 */
        gsdf_v3 mean = { 0.f, 0.f, 0.f };
        int Nj = 0;
        unsigned long long seen = 0ull;
        if (ok)
            for (int i = 0; i < a.n; ++i) {
                if (!ba_visible(a, slot, i)) continue;
                gsdf_v3 p; float m, n;
                if (!ba_project(a, v, i, &p, &m, &n)) continue;
                const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
                const gsdf_v3 A = ba_interp(n, m, im);
                mean = gsdf_v3{ mean.x + A.x, mean.y + A.y, mean.z + A.z };
                ++Nj;
                seen |= 1ull << (i & 63);
            }
        if (Nj) {
            const float inv = (float)(1. / (double)(float)Nj);
            mean = gsdf_v3{ inv * mean.x, inv * mean.y, inv * mean.z };
        }
        if (WRITE_MEAN) mc[item] = ba_mean{ mean.x, mean.y, mean.z, Nj, seen };
        if (!Nj) continue;
        n_act += 1u; n_obs += (unsigned int)Nj;
        for (int i = 0; i < a.n; ++i) {                                        /* second sweep: same samples */
            if (!((seen >> (i & 63)) & 1ull)) continue;
            gsdf_v3 p; float m, n;
            ba_project(a, v, i, &p, &m, &n);
            const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
            const gsdf_v3 A = ba_interp(n, m, im);
            const gsdf_v3 r = { A.x - mean.x, A.y - mean.y, A.z - mean.z };
            E += (double)gsdf_dot3(r, r);                                      /* :316 */
        }
    }
    double cA = (double)n_act, cO = (double)n_obs;                             /* small integers: exact in any order */
    for (int off = 32; off > 0; off >>= 1) { E += __shfl_down(E, off); cA += __shfl_down(cA, off); cO += __shfl_down(cO, off); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = E; red[1][threadIdx.x >> 6] = cA; red[2][threadIdx.x >> 6] = cO; }
    __syncthreads();
    if (threadIdx.x < 3) block_E[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

/* ---- solveDist ---- */
/* block_cnt (nullable): [2][gridDim.x] -- the workgroup's voxels with at least one observation and their observations */
/* 512 lanes per workgroup: the sweep is a latency chain per lane (a keyframe's projection, then its twelve scattered pixel
 * reads), so it wants every wave the registers allow -- 98 VGPRs = 4 per SIMD = two workgroups of eight waves per CU, where
 * 256-lane workgroups of the same grid left it at two (1.58 ms for C5's 1.42 M voxels) */
#define BA_DIST_THREADS 512
__global__ __launch_bounds__(BA_DIST_THREADS) void k_ba_dist(ba_args a, float damping, double* block_cnt) {
    __shared__ double red[2][BA_DIST_THREADS / 64];
    unsigned int n_act = 0u, n_obs = 0u;
    const size_t stride = (size_t)gridDim.x * BA_DIST_THREADS;
    for (size_t slot = (size_t)blockIdx.x * BA_DIST_THREADS + threadIdx.x; slot < a.n_slots; slot += stride) {
        ba_voxel v;
        if (!ba_load_voxel(a, slot, &v)) continue;
        int Nj = 0;
        gsdf_v3 sA = { 0, 0, 0 }, sD = { 0, 0, 0 }, sAD = { 0, 0, 0 }, sDD = { 0, 0, 0 };
        for (int i = 0; i < a.n; ++i) {
            if (!ba_visible(a, slot, i)) continue;
            gsdf_v3 p; float m, n;
            if (!ba_project(a, v, i, &p, &m, &n)) continue;
            const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
            gsdf_v3 A, g0, g1;
            ba_sample3(n, m, im, &A, &g0, &g1);
            if (ba_truncated(a, A)) continue;                                  /* :364 */
            ++Nj;
            float G[9];
            ba_pi_grad_from(a, p, g0, g1, G);
            const float* Ri = a.R + 9 * i;
            const gsdf_v3 Rtn = { -gsdf_sum3(Ri[0] * v.grad.x, Ri[3] * v.grad.y, Ri[6] * v.grad.z),
                                  -gsdf_sum3(Ri[1] * v.grad.x, Ri[4] * v.grad.y, Ri[7] * v.grad.z),
                                  -gsdf_sum3(Ri[2] * v.grad.x, Ri[5] * v.grad.y, Ri[8] * v.grad.z) };
            const gsdf_v3 Jd = gsdf_matvec(G, Rtn);                            /* :201 */
            sA = gsdf_v3{ sA.x + A.x, sA.y + A.y, sA.z + A.z };
            sD = gsdf_v3{ sD.x + Jd.x, sD.y + Jd.y, sD.z + Jd.z };
            sAD = gsdf_v3{ sAD.x + A.x * Jd.x, sAD.y + A.y * Jd.y, sAD.z + A.z * Jd.z };
            sDD = gsdf_v3{ sDD.x + Jd.x * Jd.x, sDD.y + Jd.y * Jd.y, sDD.z + Jd.z * Jd.z };
        }
        if (!Nj) continue;
        n_act += 1u; n_obs += (unsigned int)Nj;
        const float inv_Nj = (float)(1. / (double)(float)Nj);
        float H_dd = gsdf_sum3(sDD.x, sDD.y, sDD.z) - inv_Nj * gsdf_sum3(sD.x * sD.x, sD.y * sD.y, sD.z * sD.z);
        const float b_d = gsdf_sum3(sAD.x, sAD.y, sAD.z) - inv_Nj * gsdf_sum3(sA.x * sD.x, sA.y * sD.y, sA.z * sD.z);
        H_dd += a.reg_weight * v.w;                                            /* :383 */
        if (H_dd != 0.f) {
            /* updateDist: dist -= delta (:265-268); the table stores s = dist * w */
            gsdf_payload* P = &a.tab.vox[slot];
            P->s = (v.dist - damping * b_d / H_dd) * v.w;
        }
    }
    if (block_cnt) {                                                            /* wave-uniform: a kernel argument */
        double cA = (double)n_act, cO = (double)n_obs;
        for (int off = 32; off > 0; off >>= 1) { cA += __shfl_down(cA, off); cO += __shfl_down(cO, off); }
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = cA; red[1][threadIdx.x >> 6] = cO; }
        __syncthreads();
        if (threadIdx.x < 2) {                                                  /* (small integers: exact in any order) */
            double t = 0.0;
            for (int w = 0; w < BA_DIST_THREADS / 64; ++w) t += red[threadIdx.x][w];
            block_cnt[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
        }
    }
}

/* ---- solvePose: per-workgroup partial (b_i, H_i upper triangle) for every keyframe ---- */
#define BA_NV 27
/* BA_POSE_SLICES workgroups (blockIdx.y) share a set of voxels: each takes every BA_POSE_SLICES-th keyframe of the second loop
 * (the per-keyframe Jacobians and their 27-value wave reduction: 85 % of a wave's instructions).  The gate list holds ~10^5
 * voxels = ~2000 waves: one wave per SIMD and a chain of ~35 k dependent instructions each.  The first loop (the voxel's mean
 * intensity) is repeated by every slice, so more slices soon cost more than they hide: measured on C5 with the per-wave
 * accumulators below, 1 / 2 / 4 / 8 slices = 237 / 232 / 288 / 384 us (308 us with float atomics and no slices). */
#ifndef BA_POSE_SLICES
#define BA_POSE_SLICES 2
#endif
/* CACHED (round 6): the first loop -- the voxel's mean intensity over its keyframes, their number and set -- is what the energy
 * sweep in front of this one computed at the very same state (gsdf_ba_optimize: getEnergy always precedes solvePose; no truncating
 * loss): read from ba_mean instead of being repeated by every slice, which also lifts what kept the slice count at two. */
#ifndef BA_POSE_SLICES_CACHED
#define BA_POSE_SLICES_CACHED 4
#endif
template <bool CACHED, int SLICES>
__global__ __launch_bounds__(256) void k_ba_pose(ba_args a, float* block_part /* [gridDim.x][n][BA_NV] */) {
    const int slice = (int)blockIdx.y;
    /* one accumulator set per WAVE, [4][n][BA_NV]: lane 63 adds its wave's 27 sums of a keyframe with plain LDS read-modify-
     * writes.  (They were float atomics on one set shared by the four waves: ds_add_f32 is lane-serial, ~190 cycles per
     * instruction -- 27 of them per keyframe and wave were two thirds of this kernel.) */
    extern __shared__ float acc[];
    for (int i = threadIdx.x; i < 4 * a.n * BA_NV; i += 256) acc[i] = 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    float* wacc = acc + (size_t)(threadIdx.x >> 6) * a.n * BA_NV;
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t n_items = a.gate_list ? (size_t)*a.gate_count : a.n_slots;
    const size_t n_iter = (n_items + stride - 1) / stride;
    for (size_t it = 0; it < n_iter; ++it) {                                   /* uniform trip count: DPP needs whole waves */
        const size_t item = it * stride + (size_t)blockIdx.x * 256 + threadIdx.x;
        const size_t slot = item < n_items ? (a.gate_list ? (size_t)a.gate_list[item] : item) : a.n_slots;
        ba_voxel v;
        bool ok = slot < a.n_slots && ba_load_voxel(a, slot, &v);
        ok = ok && !(fabsf(v.dist) > a.vs);                                    /* :509 */
        gsdf_v3 mean = { 0.f, 0.f, 0.f };
        int Nj = 0;
        unsigned long long seen = 0ull;                                        /* keyframes (<= 64) this voxel contributes to */
        if (CACHED) {
            if (ok && item < n_items) {
                const ba_mean e = static_cast<const ba_mean*>(a.mean_cache)[item];
                mean = gsdf_v3{ e.mx, e.my, e.mz }; Nj = e.nj; seen = e.seen;     /* (the mean is stored scaled by 1 / Nj) */
            }
        } else if (ok)
            for (int i = 0; i < a.n; ++i) {
                if (!ba_visible(a, slot, i)) continue;
                gsdf_v3 p; float m, n;
                if (!ba_project(a, v, i, &p, &m, &n)) continue;
                const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
                const gsdf_v3 A = ba_interp(n, m, im);
                if (ba_truncated(a, A)) continue;                              /* :542 */
                mean = gsdf_v3{ mean.x + A.x, mean.y + A.y, mean.z + A.z };
                ++Nj;
                seen |= 1ull << (i & 63);
            }
        const float inv_Nj = Nj ? (float)(1. / (double)(float)Nj) : 0.f;
        if (!CACHED) mean = gsdf_v3{ inv_Nj * mean.x, inv_Nj * mean.y, inv_Nj * mean.z };
        for (int i = slice; i < a.n; i += SLICES) {
            const bool mine = ok && Nj && ((seen >> (i & 63)) & 1ull);
            if (!__any(mine)) continue;                                        /* wave-uniform skip */
            float val[BA_NV];
#pragma unroll
            for (int k = 0; k < BA_NV; ++k) val[k] = 0.f;
            if (mine) {
                gsdf_v3 p; float m, n;
                ba_project(a, v, i, &p, &m, &n);
                const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
                gsdf_v3 A, g0, g1;
                ba_sample3(n, m, im, &A, &g0, &g1);
                float G[9], J[18];
                ba_pi_grad_from(a, p, g0, g1, G);
                const float* Ri = a.R + 9 * i;
                const float S[9] = { 0.f, -p.z, p.y, p.z, 0.f, -p.x, -p.y, p.x, 0.f };
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {                              /* computeJc :206-233 */
                        J[6 * r + c] = -gsdf_sum3(G[3 * r] * Ri[3 * c], G[3 * r + 1] * Ri[3 * c + 1], G[3 * r + 2] * Ri[3 * c + 2]);
                        J[6 * r + 3 + c] = gsdf_sum3(G[3 * r] * S[c], G[3 * r + 1] * S[3 + c], G[3 * r + 2] * S[6 + c]);
                    }
                const gsdf_v3 r = { A.x - mean.x, A.y - mean.y, A.z - mean.z };
#pragma unroll
                for (int c = 0; c < 6; ++c) val[c] = gsdf_sum3(r.x * J[c], r.y * J[6 + c], r.z * J[12 + c]);   /* :568 */
                int q = 6;
#pragma unroll
                for (int a1 = 0; a1 < 6; ++a1)
#pragma unroll
                    for (int a2 = a1; a2 < 6; ++a2)
                        val[q++] = (1 - inv_Nj) * gsdf_sum3(J[a1] * J[a2], J[6 + a1] * J[6 + a2], J[12 + a1] * J[12 + a2]);   /* :573 */
            }
            ba_wave_sum_to_lane63(val);
            if (lane == 63) {
#pragma unroll
                for (int k = 0; k < BA_NV; ++k) wacc[i * BA_NV + k] += val[k];
            }
        }
    }
    __syncthreads();
    const int nv = a.n * BA_NV;
    for (int i = threadIdx.x; i < nv; i += 256)
        if ((i / BA_NV) % SLICES == slice)                                                           /* this slice's keyframes */
            block_part[(size_t)blockIdx.x * nv + i] = (acc[i] + acc[nv + i]) + (acc[2 * nv + i] + acc[3 * nv + i]);
}
/* one WAVE per value: lane l adds the partials of workgroups l, l + 64, ... in that order, the 64 lane sums are then added in a
 * fixed tree -- a fixed order, so deterministic like the sequential loop it replaces (one lane per value walking all 512
 * partials: 124 us of dependent strided loads for 1 350 numbers) */
__global__ __launch_bounds__(256) void k_ba_pose_reduce(const float* block_part, int n_blocks, int n_vals, float* out) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (j >= n_vals) return;
    float s = 0.f;
    for (int b = lane; b < n_blocks; b += 64) s += block_part[(size_t)b * n_vals + j];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if (lane == 0) out[j] = s;
}

/* the gate of getEnergy / solvePose as a predicate over slot numbers: the voxel exists and |dist| <= vs (the same s / w division
 * and comparison as the sweeps make) */
struct ba_gate_pred {
    const unsigned long long* bkeys;
    const gsdf_payload* vox;
    float vs;
    __device__ bool operator()(const uint32_t& slot) const {
        if (bkeys[slot / GSDF_BLOCK_VOX] == GSDF_KEY_EMPTY) return false;
        const float2 ws = *reinterpret_cast<const float2*>(vox + slot);        /* w, s */
        if (!(ws.x > 0.f)) return false;
        return !(fabsf(ws.y / ws.x) > vs);
    }
};
hipError_t gsdf_ba_compact_need(const gsdf_ba_dev& d, size_t* need) {
    return gsdf_scratch_need(need, [&d](size_t& b) {
        return rocprim::select(nullptr, b, rocprim::counting_iterator<uint32_t>(0u), (uint32_t*)nullptr, (unsigned long long*)nullptr, d.n_slots,
                               ba_gate_pred{ d.tab.bkeys, d.tab.vox, d.vs }, hipStream_t());
    });
}
hipError_t gsdf_ba_compact(const gsdf_dev<void>& tmp, hipStream_t s, const gsdf_ba_dev& d, uint32_t* list_out, unsigned long long* count_out) {
    const ba_gate_pred pred{ d.tab.bkeys, d.tab.vox, d.vs };
    size_t b = tmp.bytes();
    return rocprim::select(tmp.get(), b, rocprim::counting_iterator<uint32_t>(0u), list_out, count_out, d.n_slots, pred, s);
}

#define BA_BLOCKS 512
void gsdf_launch_ba_energy(hipStream_t s, const gsdf_ba_dev& d, double* block_E, bool write_mean_cache) {
    ba_args a; std::memcpy(&a, &d, sizeof(a));
    if (write_mean_cache && a.gate_list && a.mean_cache) hipLaunchKernelGGL(k_ba_energy<true>, dim3(BA_BLOCKS), dim3(256), 0, s, a, block_E);
    else hipLaunchKernelGGL(k_ba_energy<false>, dim3(BA_BLOCKS), dim3(256), 0, s, a, block_E);
}
void gsdf_launch_ba_dist(hipStream_t s, const gsdf_ba_dev& d, float damping, double* block_cnt) {
    ba_args a; std::memcpy(&a, &d, sizeof(a));
    hipLaunchKernelGGL(k_ba_dist, dim3(BA_BLOCKS), dim3(BA_DIST_THREADS), 0, s, a, damping, block_cnt);
}
void gsdf_launch_ba_pose(hipStream_t s, const gsdf_ba_dev& d, float* block_part, float* out, bool use_mean_cache) {
    ba_args a; std::memcpy(&a, &d, sizeof(a));
    if (use_mean_cache && a.gate_list && a.mean_cache && a.trunc_sq < 0.f)
        hipLaunchKernelGGL((k_ba_pose<true, BA_POSE_SLICES_CACHED>), dim3(BA_BLOCKS, BA_POSE_SLICES_CACHED), dim3(256), (size_t)4 * a.n * BA_NV * sizeof(float), s, a, block_part);
    else
        hipLaunchKernelGGL((k_ba_pose<false, BA_POSE_SLICES>), dim3(BA_BLOCKS, BA_POSE_SLICES), dim3(256), (size_t)4 * a.n * BA_NV * sizeof(float), s, a, block_part);
    const int n_vals = a.n * BA_NV;
    hipLaunchKernelGGL(k_ba_pose_reduce, dim3((n_vals + 3) / 4), dim3(256), 0, s, block_part, BA_BLOCKS, n_vals, out);
}
int gsdf_ba_blocks(void) { return BA_BLOCKS; }
