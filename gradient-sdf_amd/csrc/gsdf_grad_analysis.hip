/*
 * gsdf_grad_analysis.hip -- the gradient-accuracy analysis on the device (gsdf_gradient_angles / gsdf_gradient_stats,
 * include/gsdf.h): the angle between a voxel's gradient and the analytic one of a sphere scene, for the STORED gradient and for
 * central / forward / backward finite differences of the stored distances, and its statistics over |dist| < d
 * (matlab/GradientAnalysisSpheres.m, matlab/phi_statistics.m).
 *
 *   k_grad_bbox        minimum and maximum voxel index of the existing voxels (save_sdf's `voxel min` / `voxel max`)
 *   k_grad_angles      one wave64 per existing block, lane = voxel `local`: the block's 64 records in one coalesced 2 KB read,
 *                      the six face-neighbour blocks through ONE gsdf_block_lookup_n<6, false> (7 block probes per 64 voxels),
 *                      in-block neighbour distances through cross-lane moves, the facing 4 x 4 slabs of the neighbour blocks
 *                      loaded by the 16 lanes on that face only; then the double arithmetic per lane.  Appends (packed key,
 *                      dist, phi[4], threshold bin) in any order
 *   order              radix sort of (packed key, index) (gsdf_sort.hip) and k_grad_gather: the rows in gsdf_export's sorted
 *                      order -- what the host receives, and the FIXED input order of everything below
 *   statistics         per estimator a STABLE radix sort of (phi bits, bin): non-negative floats order like their bit patterns,
 *                      the canonical NaN behind all of them.  k_grad_chunk_stats: per chunk of GRAD_CHUNK sorted elements and
 *                      per threshold k, count / sum / sum of squares of the elements with bin <= k (every bin summed by one
 *                      thread walking the chunk in order, then accumulated over the bins in order).  k_grad_chunk_scan: the
 *                      counts' exclusive scan over the chunks and the sums' totals, chunk after chunk.  k_grad_select: one
 *                      workgroup per (estimator, k) finds the chunk of each of the four order statistics (two each for the 50 %
 *                      and 95 % positions) by binary search in the scanned counts and resolves the rank inside the chunk.
 *
 * No floating-point atomics; every sum has one order, fixed by the sorted arrays: the same map gives the same bytes, run to
 * run and across gsdf_grow.  The table is only read.  rocPRIM's sort is a library primitive as in gsdf_sort.hip.
 */
#include "gsdf_ctx.h"
#include "gsdf_kernels.h"
#include "gsdf_math.h"
#include "gsdf_sweep.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <cmath>
#include <vector>

#define GRAD_CHUNK 2048            /* sorted elements per chunk of the statistics (8 per thread of a 256-thread workgroup) */
#define GRAD_QNAN 0x7FC00000u      /* the NaN every undefined angle is written as: it sorts behind every finite angle */

/* ---- k_grad_bbox ------------------------------------------------------------------------------------------------------ */

/* box[0..2] preset to INT_MAX, box[3..5] to INT_MIN; one wave per block entry */
__global__ __launch_bounds__(256) void k_grad_bbox(gsdf_table tab, size_t n_blocks, int* box) {
    __shared__ int s_box[4][6];
    const uint32_t lane = threadIdx.x & 63u;
    const size_t nw = (size_t)gridDim.x * 4;
    int mn[3] = { 2147483647, 2147483647, 2147483647 }, mx[3] = { -2147483647 - 1, -2147483647 - 1, -2147483647 - 1 };
    for (size_t blk = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < n_blocks; blk += nw) {
        const unsigned long long bk = tab.bkeys[blk];
        if (bk == GSDF_KEY_EMPTY) continue;
        if (!(tab.vox[blk * GSDF_BLOCK_VOX + lane].w > 0.f)) continue;
        int v[3];
        gsdf_key_unpack(gsdf_voxel_key(bk, lane), &v[0], &v[1], &v[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = v[a] < mn[a] ? v[a] : mn[a]; mx[a] = v[a] > mx[a] ? v[a] : mx[a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        int lo = mn[a], hi = mx[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
            lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
        }
        if (lane == 0) { s_box[threadIdx.x >> 6][a] = lo; s_box[threadIdx.x >> 6][3 + a] = hi; }
    }
    __syncthreads();
    /* one update per workgroup and bound: same-address atomics serialise (per wave they cost 220 us on a 2^22-voxel table) */
    if (threadIdx.x < 6) {
        const bool is_max = threadIdx.x >= 3;
        int v = s_box[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < 4; ++w) { const int o = s_box[w][threadIdx.x]; v = is_max ? (o > v ? o : v) : (o < v ? o : v); }
        if (is_max) { if (v != -2147483647 - 1) atomicMax(&box[threadIdx.x], v); }
        else if (v != 2147483647) atomicMin(&box[threadIdx.x], v);
    }
}

/* ---- k_grad_angles ---------------------------------------------------------------------------------------------------- */

/* phi = acosd(min(|v^ . g|, 1)) (GradientAnalysisSpheres.m:162-163) as float32 degrees; v is normalised here, g is unit or NaN.
 * A zero or non-finite v, and a NaN g, give the canonical NaN. */
__device__ __forceinline__ float grad_phi(double vx, double vy, double vz, double gx, double gy, double gz) {
    const double n2 = (vx * vx + vy * vy) + vz * vz;
    if (!(n2 > 0.0) || !(n2 <= 1.7976931348623157e308)) return __uint_as_float(GRAD_QNAN);
    const double n = sqrt(n2);
    double c = fabs(((vx / n) * gx + (vy / n) * gy) + (vz / n) * gz);
    if (!(c == c)) return __uint_as_float(GRAD_QNAN);
    c = c < 1.0 ? c : 1.0;
    const float phi = (float)(acos(c) * (180.0 / 3.14159265358979323846));
    return phi == phi ? phi : __uint_as_float(GRAD_QNAN);
}

/* dist of record `r` as gsdf_export gives it, or T for a voxel that does not exist (D = vs*T*ones(sz), :55) */
__device__ __forceinline__ float grad_dist_or_T(const gsdf_payload* r, float T) {
    const float2 ws = *reinterpret_cast<const float2*>(r);
    return ws.x > 0.f ? ws.y / ws.x : T;
}

struct grad_angles_args {
    gsdf_table tab;
    size_t n_blocks;
    float vs, T;
    const int* box;                    /* [6] min, max */
    const float* spheres;              /* [n_spheres][4] cx cy cz R */
    const float* thr;                  /* [n_thr] ascending */
    int n_spheres, n_thr;
    unsigned long long* keys;          /* outputs, appended through `counter`, at most max_n */
    float* rows;                       /* [5]: dist, phi[4] */
    uint32_t* bin;
    unsigned long long* counter;
    long long max_n;
};

__global__ __launch_bounds__(256) void k_grad_angles(grad_angles_args a) {
    const gsdf_table& tab = a.tab;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t nw = (size_t)gridDim.x * 4;
    const int mn[3] = { a.box[0], a.box[1], a.box[2] }, mx[3] = { a.box[3], a.box[4], a.box[5] };
    const float T = a.T;
    const double vs = (double)a.vs, vs_inv = 1.0 / vs;
    for (size_t blk = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); blk < a.n_blocks; blk += nw) {     /* wave-uniform */
        const unsigned long long bk = tab.bkeys[blk];
        if (bk == GSDF_KEY_EMPTY) continue;
        const gsdf_payload self = tab.vox[blk * GSDF_BLOCK_VOX + lane];
        const bool ex = self.w > 0.f;
        if (!__any(ex)) continue;
        const float dist = self.s / self.w;                                   /* gsdf_export's dist (k_export) */
        const float D0 = ex ? dist : T;
        /* the six face-neighbour blocks: -x +x -y +y -z +z; a block outside the key range is missing */
        const uint32_t bc[3] = { (uint32_t)(bk & 0x7FFFFull), (uint32_t)((bk >> 19) & 0x7FFFFull), (uint32_t)((bk >> 38) & 0x7FFFFull) };
        unsigned long long nbk[6], k0[6];
        uint32_t h[6], pend = 0u;
        int b[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            const int ax = e >> 1;
            const bool in = (e & 1) ? bc[ax] < 0x7FFFFu : bc[ax] > 0u;
            uint32_t q[3] = { bc[0], bc[1], bc[2] };
            q[ax] = (e & 1) ? q[ax] + 1u : q[ax] - 1u;
            nbk[e] = in ? ((unsigned long long)q[0] | ((unsigned long long)q[1] << 19) | ((unsigned long long)q[2] << 38)) : GSDF_KEY_EMPTY;
            h[e] = in ? (gsdf_hash(nbk[e]) & tab.block_mask) : 0u;
            k0[e] = in ? tab.bkeys[h[e]] : GSDF_KEY_EMPTY;
            if (in) pend |= 1u << e;
        }
        gsdf_block_lookup_n<6, false>(tab, nbk, h, k0, pend, b);
        /* neighbour distances: inside the block from the neighbouring lane, across a face from the facing slab */
        float Dm[3], Dp[3];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) {
            const uint32_t sh = 2u * ax, step = 1u << sh, l = (lane >> sh) & 3u;
            float up = __shfl(D0, (int)((lane + step) & 63u)), dn = __shfl(D0, (int)((lane - step) & 63u));
            if (l == 0u) dn = b[2 * ax] >= 0 ? grad_dist_or_T(tab.vox + ((size_t)b[2 * ax] * GSDF_BLOCK_VOX + (lane | (3u << sh))), T) : T;
            if (l == 3u) up = b[2 * ax + 1] >= 0 ? grad_dist_or_T(tab.vox + ((size_t)b[2 * ax + 1] * GSDF_BLOCK_VOX + (lane & ~(3u << sh))), T) : T;
            Dm[ax] = dn; Dp[ax] = up;
        }
        float phi[4] = { 0.f, 0.f, 0.f, 0.f };
        unsigned long long key = 0ull;
        uint32_t bin = 0u;
        if (ex) {
            key = gsdf_voxel_key(bk, lane);
            int v[3];
            gsdf_key_unpack(key, &v[0], &v[1], &v[2]);
            /* ground truth (:96-111): the sphere maximising R - |c - centre|, the first one among equals */
            const double cx = (double)(a.vs * (float)v[0]), cy = (double)(a.vs * (float)v[1]), cz = (double)(a.vs * (float)v[2]);
            double best = 0.0, gx = 0.0, gy = 0.0, gz = 0.0;
            for (int s = 0; s < a.n_spheres; ++s) {
                const double dx = cx - (double)a.spheres[4 * s], dy = cy - (double)a.spheres[4 * s + 1], dz = cz - (double)a.spheres[4 * s + 2];
                const double m = (double)a.spheres[4 * s + 3] - sqrt((dx * dx + dy * dy) + dz * dz);
                if (s == 0 || m > best) { best = m; gx = dx; gy = dy; gz = dz; }
            }
            const double gn2 = (gx * gx + gy * gy) + gz * gz;
            if (gn2 > 0.0) { const double gn = sqrt(gn2); gx /= gn; gy /= gn; gz /= gn; }
            else gx = gy = gz = (double)__uint_as_float(GRAD_QNAN);
            double ce[3], fw[3], bw[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                const double d0 = (double)D0, dm = (double)Dm[ax], dp = (double)Dp[ax];
                const bool lo = v[ax] == mn[ax], hi = v[ax] == mx[ax];
                /* gradient(D, vs) (:81): one-sided on the box's faces, 0 where the box is one voxel thick */
                ce[ax] = (lo && hi) ? 0.0 : (lo ? (dp - d0) / vs : (hi ? (d0 - dm) / vs : (dp - dm) / (2.0 * vs)));
                fw[ax] = hi ? 0.0 : vs_inv * (dp - d0);                       /* :117-124 */
                bw[ax] = lo ? 0.0 : vs_inv * (d0 - dm);                       /* :136-143 */
            }
            phi[0] = grad_phi((double)self.gx, (double)self.gy, (double)self.gz, gx, gy, gz);
            phi[1] = grad_phi(ce[0], ce[1], ce[2], gx, gy, gz);
            phi[2] = grad_phi(fw[0], fw[1], fw[2], gx, gy, gz);
            phi[3] = grad_phi(bw[0], bw[1], bw[2], gx, gy, gz);
            /* the smallest k with |dist| < d[k] (a float compare), or n_thr */
            const float ad = fabsf(dist);
            int lo = 0, hi = a.n_thr;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (ad < a.thr[mid]) hi = mid; else lo = mid + 1; }
            bin = (uint32_t)lo;
        }
        /* one counter update per wave */
        const unsigned long long m = __ballot(ex);
        unsigned long long base = 0ull;
        if (lane == 0u) base = atomicAdd(a.counter, (unsigned long long)__popcll(m));
        base = __shfl(base, 0);
        const unsigned long long o = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (ex && (long long)o < a.max_n) {
            a.keys[o] = key;
            float* r = a.rows + 5 * o;
            r[0] = dist; r[1] = phi[0]; r[2] = phi[1]; r[3] = phi[2]; r[4] = phi[3];
            a.bin[o] = bin;
        }
    }
}

/* ---- order ------------------------------------------------------------------------------------------------------------ */

/* row i of the sorted order <- row order[i]; every output is nullable */
__global__ __launch_bounds__(256) void k_grad_gather(const unsigned long long* __restrict__ skeys, const uint32_t* __restrict__ order,
                                                      const float* __restrict__ urows, const uint32_t* __restrict__ ubin, size_t n,
                                                      int32_t* __restrict__ keys3, float* __restrict__ rows5, uint32_t* __restrict__ phis /* [4][n] */,
                                                      uint32_t* __restrict__ bins) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t j = order[i];
    if (keys3) {
        int x, y, z;
        gsdf_key_unpack(skeys[i], &x, &y, &z);
        keys3[3 * i] = x; keys3[3 * i + 1] = y; keys3[3 * i + 2] = z;
    }
    float r[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = urows[5 * j + k];
    if (rows5) {
#pragma unroll
        for (int k = 0; k < 5; ++k) rows5[5 * i + k] = r[k];
    }
    if (phis) {
#pragma unroll
        for (int e = 0; e < 4; ++e) phis[(size_t)e * n + i] = __float_as_uint(r[1 + e]);
        bins[i] = ubin[j];
    }
}

static hipError_t grad_sort_pairs_u32_need(size_t n, size_t* need) {
    const uint32_t* in = nullptr;
    uint32_t* out = nullptr;
    return gsdf_scratch_need(need, [=](size_t& b) { return rocprim::radix_sort_pairs(nullptr, b, in, out, in, out, n, 0, 32, hipStream_t()); });
}
static hipError_t grad_sort_pairs_u32(const gsdf_dev<void>& tmp, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in,
                                      uint32_t* vals_out, size_t n, hipStream_t s) {
    size_t b = tmp.bytes();
    return rocprim::radix_sort_pairs(tmp.get(), b, keys_in, keys_out, vals_in, vals_out, n, 0, 32, s);
}

/* ---- statistics ------------------------------------------------------------------------------------------------------- */

/* element i of a sorted estimator array takes part at threshold k iff its angle is a number and its bin <= k */
__device__ __forceinline__ uint32_t grad_elem_bin(uint32_t phi_bits, uint32_t bin, uint32_t n_thr) {
    return phi_bits < 0x7F800000u ? bin : n_thr;
}

/* grid (chunks, 4 estimators).  cnt / sum / sq [e][chunk][k]: over the chunk's elements with bin <= k */
__global__ __launch_bounds__(256) void k_grad_chunk_stats(const uint32_t* __restrict__ sphis /* [4][n] */, const uint32_t* __restrict__ sbins /* [4][n] */,
                                                           size_t n, int n_thr, size_t n_chunks, uint32_t* __restrict__ cnt /* [4][n_chunks + 1][n_thr] */,
                                                           double* __restrict__ sum, double* __restrict__ sq /* [4][n_chunks][n_thr] */) {
    __shared__ float s_phi[GRAD_CHUNK];
    __shared__ unsigned short s_bin[GRAD_CHUNK];
    __shared__ uint32_t s_cnt[256];
    __shared__ double s_sum[256], s_sq[256];
    const size_t chunk = blockIdx.x, e = blockIdx.y, first = chunk * GRAD_CHUNK;
    const int m = n - first < GRAD_CHUNK ? (int)(n - first) : GRAD_CHUNK;
    for (int i = threadIdx.x; i < m; i += 256) {
        const uint32_t p = sphis[e * n + first + i];
        s_phi[i] = __uint_as_float(p);
        s_bin[i] = (unsigned short)grad_elem_bin(p, sbins[e * n + first + i], (uint32_t)n_thr);
    }
    __syncthreads();
    /* thread t sums bin t, walking the chunk in order (every thread reads the same LDS word: a broadcast) */
    uint32_t c = 0u;
    double s = 0.0, q = 0.0;
    if ((int)threadIdx.x < n_thr)
        for (int i = 0; i < m; ++i)
            if (s_bin[i] == (unsigned short)threadIdx.x) { const double x = (double)s_phi[i]; ++c; s += x; q += x * x; }
    s_cnt[threadIdx.x] = c; s_sum[threadIdx.x] = s; s_sq[threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t* oc = cnt + (e * (n_chunks + 1) + chunk) * (size_t)n_thr;
        double* os = sum + (e * n_chunks + chunk) * (size_t)n_thr;
        double* oq = sq + (e * n_chunks + chunk) * (size_t)n_thr;
        uint32_t rc = 0u;
        double rs = 0.0, rq = 0.0;
        for (int k = 0; k < n_thr; ++k) { rc += s_cnt[k]; rs += s_sum[k]; rq += s_sq[k]; oc[k] = rc; os[k] = rs; oq[k] = rq; }
    }
}

/* grid (1, 4), thread k: cnt becomes its exclusive scan over the chunks with the total in row n_chunks; tot[e][k] = sum, sum
 * of squares over all chunks, chunk after chunk */
__global__ __launch_bounds__(256) void k_grad_chunk_scan(uint32_t* __restrict__ cnt, const double* __restrict__ sum, const double* __restrict__ sq,
                                                          int n_thr, size_t n_chunks, double* __restrict__ tot /* [4][n_thr][2] */) {
    const int k = (int)threadIdx.x;
    const size_t e = blockIdx.y;
    if (k >= n_thr) return;
    uint32_t run = 0u;
    double s = 0.0, q = 0.0;
    for (size_t ch = 0; ch < n_chunks; ++ch) {
        uint32_t* pc = cnt + (e * (n_chunks + 1) + ch) * (size_t)n_thr + k;
        const uint32_t t = *pc;
        *pc = run; run += t;
        s += sum[(e * n_chunks + ch) * (size_t)n_thr + k];
        q += sq[(e * n_chunks + ch) * (size_t)n_thr + k];
    }
    cnt[(e * (n_chunks + 1) + n_chunks) * (size_t)n_thr + k] = run;
    tot[(e * n_thr + k) * 2] = s; tot[(e * n_thr + k) * 2 + 1] = q;
}

/* grid (n_thr, 4): stats[e][k][5] = count, mean, median, rmse, p95 (phi_statistics.m:69-73; prctile: position n p / 100 + 0.5
 * among the sorted x[1..n], clamped to [1, n], linear in between) */
__global__ __launch_bounds__(256) void k_grad_select(const uint32_t* __restrict__ sphis, const uint32_t* __restrict__ sbins, size_t n, int n_thr,
                                                      size_t n_chunks, const uint32_t* __restrict__ cnt, const double* __restrict__ tot,
                                                      double* __restrict__ stats) {
    __shared__ uint32_t s_c[256];
    __shared__ float s_val[4];
    const uint32_t k = blockIdx.x;
    const size_t e = blockIdx.y;
    const uint32_t* ccol = cnt + e * (n_chunks + 1) * (size_t)n_thr + k;          /* ccol[ch * n_thr] */
    const uint32_t N = ccol[n_chunks * (size_t)n_thr];
    double* out = stats + (e * n_thr + k) * 5;
    if (N == 0u) {
        if (threadIdx.x == 0) {
            const double nan = (double)__uint_as_float(GRAD_QNAN);
            out[0] = 0.0; out[1] = nan; out[2] = nan; out[3] = nan; out[4] = nan;
        }
        return;
    }
    uint32_t rank[4];
    double frac[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        double pos = (double)N * (p == 0 ? 0.5 : 0.95) + 0.5;
        pos = pos < 1.0 ? 1.0 : (pos > (double)N ? (double)N : pos);
        const double fl = floor(pos);
        frac[p] = pos - fl;
        rank[2 * p] = (uint32_t)fl - 1u;
        rank[2 * p + 1] = rank[2 * p] + 1u < N ? rank[2 * p] + 1u : N - 1u;
    }
    for (int j = 0; j < 4; ++j) {
        /* the last chunk whose exclusive count is <= rank holds the element */
        size_t lo = 0, hi = n_chunks - 1;
        while (lo < hi) { const size_t mid = (lo + hi + 1) >> 1; if (ccol[mid * (size_t)n_thr] <= rank[j]) lo = mid; else hi = mid - 1; }
        const uint32_t target = rank[j] - ccol[lo * (size_t)n_thr];
        const size_t i0 = lo * GRAD_CHUNK + (size_t)threadIdx.x * 8;
        uint32_t mine = 0u;
        for (int t = 0; t < 8; ++t) {
            const size_t i = i0 + t;
            if (i < n && grad_elem_bin(sphis[e * n + i], sbins[e * n + i], (uint32_t)n_thr) <= k) ++mine;
        }
        s_c[threadIdx.x] = mine;
        __syncthreads();
        uint32_t before = 0u;
        for (uint32_t t = 0; t < threadIdx.x; ++t) before += s_c[t];
        if (target >= before && target < before + mine) {
            uint32_t seen = before;
            for (int t = 0; t < 8; ++t) {
                const size_t i = i0 + t;
                if (i < n && grad_elem_bin(sphis[e * n + i], sbins[e * n + i], (uint32_t)n_thr) <= k) {
                    if (seen == target) { s_val[j] = __uint_as_float(sphis[e * n + i]); break; }
                    ++seen;
                }
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double x0 = (double)s_val[0], x1 = (double)s_val[1], y0 = (double)s_val[2], y1 = (double)s_val[3];
        out[0] = (double)N;
        out[1] = tot[(e * n_thr + k) * 2] / (double)N;
        out[2] = x0 + frac[0] * (x1 - x0);
        out[3] = sqrt(tot[(e * n_thr + k) * 2 + 1] / (double)N);
        out[4] = y0 + frac[1] * (y1 - y0);
    }
}

/* ---- host: gsdf_gradient_angles / gsdf_gradient_stats ------------------------------------------------------------------ */

static int gfail(int code, const std::string& msg) { return gsdf_fail(code, msg); }

static bool grad_spheres_ok(const float* sp, int n_spheres) {
    for (int i = 0; i < 4 * n_spheres; ++i)
        if (!std::isfinite(sp[i])) return false;
    for (int i = 0; i < n_spheres; ++i)
        if (!(sp[4 * i + 3] > 0.f)) return false;
    return true;
}

/* what both entries share: the rows of all existing voxels on the device and the order that sorts them by packed key */
struct grad_rows {
    size_t n = 0;
    gsdf_dev<unsigned long long> ukeys;
    gsdf_dev<uint32_t> ubin;
    gsdf_dev<float> urows;
    gsdf_key_order ord;
};

static int grad_count(gsdf_ctx* c, size_t* n) {
    int64_t h = 0;
    if (int rc = gsdf_count(c, &h)) return rc;
    if (h > 2147483647ll) return gfail(GSDF_ERR_INVALID, "gradient analysis: more than 2^31 - 1 voxels (row indices are 32-bit)");
    *n = (size_t)h;
    return GSDF_OK;
}

/* R.n = the voxel count from grad_count, > 0.  Everything is queued on the context's stream; nothing is waited for. */
static int grad_compute_rows(gsdf_ctx* c, const float* spheres4_host, int n_spheres, const float* thresholds, int n_thr, grad_rows& R) {
    const size_t n = R.n;
    gsdf_dev<int> d_box;
    gsdf_dev<float> d_par;                                  /* spheres [64][4], then thresholds [256] */
    HIP_TRY(d_box.alloc(6));
    HIP_TRY(d_par.alloc(256 + 256));
    HIP_TRY(R.ukeys.alloc(n));
    HIP_TRY(R.ubin.alloc(n));
    HIP_TRY(R.urows.alloc(n * 5));
    HIP_TRY(R.ord.alloc(n));
    float par[512] = { 0.f };
    std::copy(spheres4_host, spheres4_host + 4 * n_spheres, par);
    if (n_thr) std::copy(thresholds, thresholds + n_thr, par + 256);
    const int box[6] = { 2147483647, 2147483647, 2147483647, -2147483647 - 1, -2147483647 - 1, -2147483647 - 1 };
    HIP_TRY(hipMemcpyAsync(d_box, box, sizeof(box), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_par, par, sizeof(par), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(gsdf_counter_zero(c));
    const size_t n_blocks = (size_t)c->tab.block_mask + 1;
    const unsigned int grid = (unsigned int)std::min<size_t>((n_blocks + 3) / 4, 4096);
    hipLaunchKernelGGL(k_grad_bbox, dim3(std::min(grid, 1024u)), dim3(256), 0, c->stream, c->tab, n_blocks, d_box.get());
    grad_angles_args a;
    a.tab = c->tab; a.n_blocks = n_blocks; a.vs = c->voxel_size; a.T = c->T; a.box = d_box; a.spheres = d_par; a.thr = d_par + 256;
    a.n_spheres = n_spheres; a.n_thr = n_thr; a.keys = R.ukeys; a.rows = R.urows; a.bin = R.ubin; a.counter = c->counter;
    a.max_n = (long long)n;
    hipLaunchKernelGGL(k_grad_angles, dim3(grid), dim3(256), 0, c->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(R.ord.run(c, R.ukeys, n));
    /* d_box and d_par are released on return: hipFree waits for the kernels that read them (gsdf_dev.h) */
    return GSDF_OK;
}

int gsdf_gradient_angles(gsdf_ctx* c, const float* spheres4_host, int n_spheres, int32_t* keys, float* rows5, int64_t max_n, int64_t* n) {
    if (!c) return gfail(GSDF_ERR_INVALID, "null context");
    if (int rc = gsdf_flush_pending(c)) return rc;
    if (!spheres4_host || !n || max_n < 0 || (max_n > 0 && !keys && !rows5)) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_angles: null argument");
    if (n_spheres < 1 || n_spheres > 64) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_angles: 1..64 spheres");
    if (!grad_spheres_ok(spheres4_host, n_spheres)) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_angles: a sphere row is not finite or has R <= 0");
    HIP_TRY(hipSetDevice(c->device));
    grad_rows R;
    if (int rc = grad_count(c, &R.n)) return rc;
    *n = (int64_t)R.n;
    if (R.n == 0 || max_n == 0) return GSDF_OK;                                /* an empty map; the sizing call */
    if ((int64_t)R.n > max_n) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_angles: max_n too small (*n holds the need)");
    if (int rc = grad_compute_rows(c, spheres4_host, n_spheres, nullptr, 0, R)) return rc;
    gsdf_dev<int32_t> d_keys3;
    gsdf_dev<float> d_rows;
    if (keys) HIP_TRY(d_keys3.alloc(R.n * 3));
    if (rows5) HIP_TRY(d_rows.alloc(R.n * 5));
    hipLaunchKernelGGL(k_grad_gather, dim3((unsigned int)((R.n + 255) / 256)), dim3(256), 0, c->stream, R.ord.skeys.get(), R.ord.order.get(),
                       R.urows.get(), R.ubin.get(), R.n, keys ? d_keys3.get() : nullptr, rows5 ? d_rows.get() : nullptr, (uint32_t*)nullptr,
                       (uint32_t*)nullptr);
    HIP_TRY(hipGetLastError());
    /* into buffers of the library first: the caller's are written only once everything has succeeded */
    std::vector<int32_t> hk(keys ? R.n * 3 : 0);
    std::vector<float> hr(rows5 ? R.n * 5 : 0);
    if (keys) HIP_TRY(hipMemcpyAsync(hk.data(), d_keys3, hk.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (rows5) HIP_TRY(hipMemcpyAsync(hr.data(), d_rows, hr.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    unsigned long long n2 = 0;
    HIP_TRY(gsdf_counter_read(c, &n2));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n2 != R.n) return gfail(GSDF_ERR_HIP, "gsdf_gradient_angles: the map changed between the counting and the angle pass");
    if (keys) std::copy(hk.begin(), hk.end(), keys);
    if (rows5) std::copy(hr.begin(), hr.end(), rows5);
    return GSDF_OK;
}

int gsdf_gradient_stats(gsdf_ctx* c, const float* spheres4_host, int n_spheres, const float* thresholds, int n_thr, double* stats) {
    if (!c) return gfail(GSDF_ERR_INVALID, "null context");
    if (int rc = gsdf_flush_pending(c)) return rc;
    if (!spheres4_host || !thresholds || !stats) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_stats: null argument");
    if (n_spheres < 1 || n_spheres > 64) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_stats: 1..64 spheres");
    if (n_thr < 1 || n_thr > 256) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_stats: 1..256 thresholds");
    if (!grad_spheres_ok(spheres4_host, n_spheres)) return gfail(GSDF_ERR_INVALID, "gsdf_gradient_stats: a sphere row is not finite or has R <= 0");
    for (int k = 0; k < n_thr; ++k)
        if (!std::isfinite(thresholds[k]) || !(thresholds[k] > 0.f) || (k > 0 && !(thresholds[k] > thresholds[k - 1])))
            return gfail(GSDF_ERR_INVALID, "gsdf_gradient_stats: thresholds must be finite, positive and strictly ascending");
    HIP_TRY(hipSetDevice(c->device));
    grad_rows R;
    if (int rc = grad_count(c, &R.n)) return rc;
    const size_t n = R.n, n_out = (size_t)4 * n_thr * 5;
    std::vector<double> hs(n_out);
    if (n == 0) {
        for (size_t i = 0; i < n_out; ++i) hs[i] = i % 5 == 0 ? 0.0 : (double)NAN;
        std::copy(hs.begin(), hs.end(), stats);
        return GSDF_OK;
    }
    if (int rc = grad_compute_rows(c, spheres4_host, n_spheres, thresholds, n_thr, R)) return rc;
    const size_t n_chunks = (n + GRAD_CHUNK - 1) / GRAD_CHUNK;
    gsdf_dev<uint32_t> d_phis, d_bins, d_sphis, d_sbins, d_cnt;
    gsdf_dev<double> d_sum, d_sq, d_tot, d_stats;
    gsdf_dev<void> d_tmp;
    HIP_TRY(d_phis.alloc(4 * n));
    HIP_TRY(d_bins.alloc(n));
    HIP_TRY(d_sphis.alloc(4 * n));
    HIP_TRY(d_sbins.alloc(4 * n));
    HIP_TRY(d_cnt.alloc(4 * (n_chunks + 1) * n_thr));
    HIP_TRY(d_sum.alloc(4 * n_chunks * n_thr));
    HIP_TRY(d_sq.alloc(4 * n_chunks * n_thr));
    HIP_TRY(d_tot.alloc((size_t)4 * n_thr * 2));
    HIP_TRY(d_stats.alloc(n_out));
    size_t need = 0;
    HIP_TRY(grad_sort_pairs_u32_need(n, &need));
    HIP_TRY(d_tmp.alloc(need));
    hipLaunchKernelGGL(k_grad_gather, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, c->stream, R.ord.skeys.get(), R.ord.order.get(),
                       R.urows.get(), R.ubin.get(), n, (int32_t*)nullptr, (float*)nullptr, d_phis.get(), d_bins.get());
    for (size_t e = 0; e < 4; ++e)
        HIP_TRY(grad_sort_pairs_u32(d_tmp, d_phis + e * n, d_sphis + e * n, d_bins, d_sbins + e * n, n, c->stream));
    hipLaunchKernelGGL(k_grad_chunk_stats, dim3((unsigned int)n_chunks, 4), dim3(256), 0, c->stream, d_sphis.get(), d_sbins.get(), n, n_thr,
                       n_chunks, d_cnt.get(), d_sum.get(), d_sq.get());
    hipLaunchKernelGGL(k_grad_chunk_scan, dim3(1, 4), dim3(256), 0, c->stream, d_cnt.get(), d_sum.get(), d_sq.get(), n_thr, n_chunks, d_tot.get());
    hipLaunchKernelGGL(k_grad_select, dim3((unsigned int)n_thr, 4), dim3(256), 0, c->stream, d_sphis.get(), d_sbins.get(), n, n_thr, n_chunks,
                       d_cnt.get(), d_tot.get(), d_stats.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hs.data(), d_stats, n_out * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    unsigned long long n2 = 0;
    HIP_TRY(gsdf_counter_read(c, &n2));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n2 != n) return gfail(GSDF_ERR_HIP, "gsdf_gradient_stats: the map changed between the counting and the angle pass");
    std::copy(hs.begin(), hs.end(), stats);
    return GSDF_OK;
}
