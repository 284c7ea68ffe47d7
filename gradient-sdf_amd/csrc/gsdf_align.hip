/*
 * gsdf_align.hip -- registration of a point set against the map, and the map's own surface cloud (gfx950).
 *
 *   k_align_pass / k_align_head   RigidPointOptimizer::optimize_sampled, :70-95, over n given points   RigidPointOptimizer.cpp:51-96
 *   k_align_pass_multi / k_align_head_multi   the same two bodies for a batch of starting poses, one run each, side by side
 *   k_align_pass_robust / k_align_head_robust (and _multi_robust)   the same bodies with a robust loss's weight on every term
 *   k_align_residuals   the distance and the voxel weight each point meets under a pose: what a pass sees, per point
 *   k_surface_flag / k_surface_rows   MapGradPixelSdf::extract_pc's rows, in memory                    MapGradPixelSdf.cpp:177-195
 *
 * The reference's tracker turns the depth image into points (:62-69) and never looks at the image again (:70-82); the pass
 * below is that loop over points the caller brings.  Per point it evaluates gsdf_grad_sample (gsdf_sample.h), the body of
 * k_query, so a pass sees bit for bit what gsdf_query returns for the transformed point.
 *
 * Sums (E, g[6], H upper triangle[21], count): every float term is widened to double and added
 *   - per lane in the order of the grid-stride loop (point i, i + stride, ...),
 *   - over the 64 lanes of a wave by a fixed xor butterfly (32, 16, 8, 4, 2, 1),
 *   - over the waves of a workgroup in wave order (one LDS row per wave),
 *   - over the workgroups in index order, by the head kernel,
 * and each of the 29 double totals is rounded to float once.  The order is a function of n and of the launch geometry, which is
 * a function of n alone: the same call gives the same bytes.  No floating-point atomics; the kernel boundary between a pass and
 * its head is the only grid barrier, there is no hand-off between workgroups inside a launch.
 * The _multi kernels run the same two bodies for several starting poses in one launch pair: workgroup (x, y) of the pass is
 * workgroup x of run live[y], workgroup y of the head is that run's head, each run on its own state, partial rows and trace rows.
 * Per run the order above holds unchanged, so a run's bytes are those of a single call from its start.
 *
 * Both kernels are gathers over a table that is cache-resident at the project's map sizes; nothing here is MFMA-shaped.
 * Wave = 64 lanes.
 */
#include "gsdf_kernels.h"
#include "gsdf_align_loss.h"
#include "gsdf_math.h"
#include "gsdf_sample.h"

#include <hip/hip_runtime.h>

#define ALIGN_WAVES (GSDF_ALIGN_BLOCK / 64)
/* the sums of a pass: the 29 of GSDF_TRACK_NSUM, and for a robust pass the weight sum (slot 29) and the inlier count (slot 30) */
#define ALIGN_NSUM(ROBUST) ((ROBUST) ? GSDF_ALIGN_NSUM_ROBUST : GSDF_TRACK_NSUM)
/* floats of a trace row: 36, and for a robust pass 38 ([36] = the weight sum, [37] = the inlier count) */
#define ALIGN_TRACE(ROBUST) ((ROBUST) ? 38 : 36)

int gsdf_align_grid(long long n) {
    const long long b = (n + GSDF_ALIGN_BLOCK - 1) / GSDF_ALIGN_BLOCK;
    return (int)(b < 1 ? 1 : (b > GSDF_ALIGN_MAXBLK ? GSDF_ALIGN_MAXBLK : b));
}

/* One pass over the points for one run: part[workgroup][32] = this workgroup's 29 sums (slots 29..31 zero).  The body of
 * k_align_pass and of k_align_pass_multi: blockIdx.x / gridDim.x are the workgroup's index and count within the run.
 * ROBUST (k_align_pass_robust, k_align_pass_multi_robust): every term carries the weight rw = gsdf_align_weight(loss, scale, phi)
 * of its point -- wphi = rw phi and wJ = rw J, then wphi phi, wphi J[a], wJ[a] J[b], one float operation each -- and the row
 * has 31 sums: slot 29 the sum of the weights, slot 30 the number of points with rw > 0.  With loss = L2, rw = 1 and every
 * product with it is exact: slots 0..28 are the plain pass's bit for bit. */
template <bool ROBUST>
__device__ __forceinline__ void align_pass_body(gsdf_table tab, float vs, float inv_vs, const float* __restrict__ pts, long long n,
                                                const gsdf_align_state* __restrict__ st, double* __restrict__ part,
                                                double (&rows)[ALIGN_WAVES][GSDF_ALIGN_ROW], int loss = 0, float scale = 0.f) {
    constexpr int NSUM = ALIGN_NSUM(ROBUST);
    float R[9];
    gsdf_quat_to_R(st->pose7 + 3, R);                                      /* :53 */
    const gsdf_v3 t = { st->pose7[0], st->pose7[1], st->pose7[2] };        /* :54 */
    double acc[NSUM];
#pragma unroll
    for (int v = 0; v < NSUM; ++v) acc[v] = 0.0;
    const long long stride = (long long)gridDim.x * GSDF_ALIGN_BLOCK;
    for (long long i = (long long)blockIdx.x * GSDF_ALIGN_BLOCK + threadIdx.x; i < n; i += stride) {
        const gsdf_v3 x = { pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] };
        const gsdf_v3 p = gsdf_rigid_apply(R, t, x);                       /* :70 */
        /* a point that is not finite never reaches the float -> int conversion of float2vox (the reference would convert it) */
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
        float w0, phi;
        gsdf_v3 g;
        gsdf_grad_sample(tab, vs, inv_vs, p, w0, phi, g);                  /* :72, :75 */
        if (w0 > 0.f) {
            const gsdf_v3 pxg = gsdf_cross3(p, g);
            const float J[6] = { g.x, g.y, g.z, pxg.x, pxg.y, pxg.z };     /* :77-78 */
            if constexpr (ROBUST) {
                const float rw = gsdf_align_weight(loss, scale, phi);
                const float wphi = rw * phi;
                float wJ[6];
#pragma unroll
                for (int a = 0; a < 6; ++a) wJ[a] = rw * J[a];
                acc[0] += (double)(wphi * phi);
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[1 + a] += (double)(wphi * J[a]);
                int q = 7;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b) acc[q++] += (double)(wJ[a] * J[b]);
                acc[28] += 1.0;
                acc[29] += (double)rw;
                if (rw > 0.f) acc[30] += 1.0;
            } else {
                acc[0] += (double)(phi * phi);                             /* :76 */
#pragma unroll
                for (int a = 0; a < 6; ++a) acc[1 + a] += (double)(phi * J[a]);   /* :79 */
                int q = 7;
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b) acc[q++] += (double)(J[a] * J[b]);   /* :80 */
                acc[28] += 1.0;                                            /* :81 */
            }
        }
    }
    /* the butterfly: afterwards every lane holds the wave's sums (a + b is commutative, so all lanes hold the same bits) */
#pragma unroll
    for (int v = 0; v < NSUM; ++v) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc[v] += __shfl_xor(acc[v], m, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int v = 0; v < NSUM; ++v) rows[wave][v] = acc[v];
    }
    __syncthreads();
    if (threadIdx.x < GSDF_ALIGN_ROW) {
        double s = 0.0;
        if (threadIdx.x < NSUM) {
            s = rows[0][threadIdx.x];
#pragma unroll
            for (int wv = 1; wv < ALIGN_WAVES; ++wv) s += rows[wv][threadIdx.x];
        }
        part[(size_t)blockIdx.x * GSDF_ALIGN_ROW + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(GSDF_ALIGN_BLOCK) void k_align_pass(gsdf_table tab, float vs, float inv_vs, const float* __restrict__ pts,
                                                                 long long n, const gsdf_align_state* __restrict__ st,
                                                                 double* __restrict__ part) {
    if (st->done) return;                                                  /* queued beyond the end of the run */
    __shared__ double rows[ALIGN_WAVES][GSDF_ALIGN_ROW];
    align_pass_body<false>(tab, vs, inv_vs, pts, n, st, part, rows);
}

/* The same pass for the live runs of a batch of starts: workgroup (x, y) is workgroup x of run live[y].  st[m], part[m][gridDim.x][32]. */
__global__ __launch_bounds__(GSDF_ALIGN_BLOCK) void k_align_pass_multi(gsdf_table tab, float vs, float inv_vs, const float* __restrict__ pts,
                                                                       long long n, const gsdf_align_state* __restrict__ st,
                                                                       double* __restrict__ part, const int* __restrict__ live) {
    const int h = live[blockIdx.y];
    if (st[h].done) return;                                                /* ended inside this batch */
    __shared__ double rows[ALIGN_WAVES][GSDF_ALIGN_ROW];
    align_pass_body<false>(tab, vs, inv_vs, pts, n, st + h, part + (size_t)h * gridDim.x * GSDF_ALIGN_ROW, rows);
}

/* the two passes with the loss's weights: the same body, 31 sums per row */
__global__ __launch_bounds__(GSDF_ALIGN_BLOCK) void k_align_pass_robust(gsdf_table tab, float vs, float inv_vs, const float* __restrict__ pts,
                                                                        long long n, const gsdf_align_state* __restrict__ st,
                                                                        double* __restrict__ part, int loss, float scale) {
    if (st->done) return;
    __shared__ double rows[ALIGN_WAVES][GSDF_ALIGN_ROW];
    align_pass_body<true>(tab, vs, inv_vs, pts, n, st, part, rows, loss, scale);
}
__global__ __launch_bounds__(GSDF_ALIGN_BLOCK) void k_align_pass_multi_robust(gsdf_table tab, float vs, float inv_vs,
                                                                              const float* __restrict__ pts, long long n,
                                                                              const gsdf_align_state* __restrict__ st,
                                                                              double* __restrict__ part, const int* __restrict__ live,
                                                                              int loss, float scale) {
    const int h = live[blockIdx.y];
    if (st[h].done) return;
    __shared__ double rows[ALIGN_WAVES][GSDF_ALIGN_ROW];
    align_pass_body<true>(tab, vs, inv_vs, pts, n, st + h, part + (size_t)h * gridDim.x * GSDF_ALIGN_ROW, rows, loss, scale);
}

/* The head of one pass (:86-95): totals, solve, stop test, pose update, trace row.  The partial rows are staged through LDS
 * ALIGN_HEAD_ROWS at a time by the whole workgroup (a lane that loads its value row by row waits for a round trip per row:
 * measured with 190 rows, a 25-pass call took 1.51 ms that way and takes 0.65 ms this way); lane v < 29 then adds value v of
 * the staged rows in index order. */
#define ALIGN_HEAD_THREADS 256
#define ALIGN_HEAD_ROWS 64
/* the body of k_align_head and of k_align_head_multi; `last` (nullable, 36 floats) receives every executed pass's row in turn.
 * ROBUST: 31 totals, and rows of 38 floats whose [36] and [37] are the weight sum and the inlier count; the rest is the same. */
template <bool ROBUST>
__device__ __forceinline__ void align_head_body(gsdf_align_state* __restrict__ st, const double* __restrict__ part, int grid, float conv_sq,
                                                float damping, int max_passes, float* __restrict__ trace, float* __restrict__ last,
                                                double (&stage)[ALIGN_HEAD_ROWS * GSDF_ALIGN_ROW], float (&tot)[GSDF_ALIGN_ROW]) {
    constexpr int NSUM = ALIGN_NSUM(ROBUST), TRACE = ALIGN_TRACE(ROBUST);
    double s = 0.0;
    for (int b0 = 0; b0 < grid; b0 += ALIGN_HEAD_ROWS) {
        const int nrow = min(ALIGN_HEAD_ROWS, grid - b0);
        for (int e = threadIdx.x; e < nrow * GSDF_ALIGN_ROW; e += ALIGN_HEAD_THREADS) stage[e] = part[(size_t)b0 * GSDF_ALIGN_ROW + e];
        __syncthreads();
        if (threadIdx.x < NSUM)
            for (int r = 0; r < nrow; ++r) s += stage[r * GSDF_ALIGN_ROW + threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < NSUM) tot[threadIdx.x] = (float)s;        /* the one rounding of each sum */
    __syncthreads();
    if (threadIdx.x != 0) return;
    float gvec[6], Hm[36];
#pragma unroll
    for (int i = 0; i < 6; ++i) gvec[i] = tot[1 + i];
    int q = 7;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) { Hm[6 * i + j] = tot[q]; Hm[6 * j + i] = tot[q]; ++q; }
    /* the EXACT forms of gsdf_math.h (correctly rounded roots and divisions, full-range sinf / cosf), not the tracker's <= 1-ulp
     * ones: this head runs a handful of times per call, not 10 000 times a second */
    float xi[6];
    gsdf_llt_solve6(Hm, gvec, xi);                                         /* :86 */
#pragma unroll
    for (int i = 0; i < 6; ++i) xi[i] = damping * xi[i];
    const float nrm = gsdf_sum3(xi[0] * xi[0], xi[1] * xi[1], xi[2] * xi[2]) +
                      gsdf_sum3(xi[3] * xi[3], xi[4] * xi[4], xi[5] * xi[5]);
    const int k = st->passes;
    if (trace) {
        float* tr = trace + (size_t)TRACE * k;
#pragma unroll
        for (int i = 0; i < GSDF_TRACK_NSUM; ++i) tr[i] = tot[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) tr[29 + i] = xi[i];
        tr[35] = nrm;
        if constexpr (ROBUST) { tr[36] = tot[29]; tr[37] = tot[30]; }
    }
    if (last) {
#pragma unroll
        for (int i = 0; i < GSDF_TRACK_NSUM; ++i) last[i] = tot[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) last[29 + i] = xi[i];
        last[35] = nrm;
        if constexpr (ROBUST) { last[36] = tot[29]; last[37] = tot[30]; }
    }
    st->passes = k + 1;
    if (nrm < conv_sq) {                                                   /* :88-91: xi is NOT applied */
        st->converged = 1;
        st->done = 1;
        return;
    }
    bool nan = false;
#pragma unroll
    for (int i = 0; i < 6; ++i) nan = nan || isnan(xi[i]);
    if (!nan) {                                                            /* :94-95 */
        float mxi[6], pose[7];
#pragma unroll
        for (int i = 0; i < 6; ++i) mxi[i] = -xi[i];
#pragma unroll
        for (int i = 0; i < 7; ++i) pose[i] = st->pose7[i];
        gsdf_se3_exp_mul(mxi, pose);
#pragma unroll
        for (int i = 0; i < 7; ++i) st->pose7[i] = pose[i];
    }
    if (k + 1 >= max_passes) st->done = 1;                                 /* :98 return false */
}

__global__ __launch_bounds__(ALIGN_HEAD_THREADS) void k_align_head(gsdf_align_state* __restrict__ st, const double* __restrict__ part,
                                                                   int grid, float conv_sq, float damping, int max_passes,
                                                                   float* __restrict__ trace) {
    if (st->done) return;
    __shared__ double stage[ALIGN_HEAD_ROWS * GSDF_ALIGN_ROW];
    __shared__ float tot[GSDF_ALIGN_ROW];
    align_head_body<false>(st, part, grid, conv_sq, damping, max_passes, trace, nullptr, stage, tot);
}

/* The heads of the live runs side by side: workgroup y is the head of run live[y] on its rows part[h][grid][32], its state, its
 * trace rows trace[h][max_passes][36] (nullable) and its last row last[h][36] (nullable). */
__global__ __launch_bounds__(ALIGN_HEAD_THREADS) void k_align_head_multi(gsdf_align_state* __restrict__ st, const double* __restrict__ part,
                                                                         int grid, float conv_sq, float damping, int max_passes,
                                                                         float* __restrict__ trace, float* __restrict__ last,
                                                                         const int* __restrict__ live) {
    const int h = live[blockIdx.x];
    if (st[h].done) return;
    __shared__ double stage[ALIGN_HEAD_ROWS * GSDF_ALIGN_ROW];
    __shared__ float tot[GSDF_ALIGN_ROW];
    align_head_body<false>(st + h, part + (size_t)h * grid * GSDF_ALIGN_ROW, grid, conv_sq, damping, max_passes,
                           trace ? trace + (size_t)h * max_passes * 36 : nullptr, last ? last + (size_t)h * 36 : nullptr, stage, tot);
}

/* the two heads over 31 totals, with rows of 38 floats */
__global__ __launch_bounds__(ALIGN_HEAD_THREADS) void k_align_head_robust(gsdf_align_state* __restrict__ st, const double* __restrict__ part,
                                                                          int grid, float conv_sq, float damping, int max_passes,
                                                                          float* __restrict__ trace) {
    if (st->done) return;
    __shared__ double stage[ALIGN_HEAD_ROWS * GSDF_ALIGN_ROW];
    __shared__ float tot[GSDF_ALIGN_ROW];
    align_head_body<true>(st, part, grid, conv_sq, damping, max_passes, trace, nullptr, stage, tot);
}
__global__ __launch_bounds__(ALIGN_HEAD_THREADS) void k_align_head_multi_robust(gsdf_align_state* __restrict__ st,
                                                                                const double* __restrict__ part, int grid, float conv_sq,
                                                                                float damping, int max_passes, float* __restrict__ trace,
                                                                                float* __restrict__ last, const int* __restrict__ live) {
    const int h = live[blockIdx.x];
    if (st[h].done) return;
    __shared__ double stage[ALIGN_HEAD_ROWS * GSDF_ALIGN_ROW];
    __shared__ float tot[GSDF_ALIGN_ROW];
    align_head_body<true>(st + h, part + (size_t)h * grid * GSDF_ALIGN_ROW, grid, conv_sq, damping, max_passes,
                          trace ? trace + (size_t)h * max_passes * 38 : nullptr, last ? last + (size_t)h * 38 : nullptr, stage, tot);
}

void gsdf_launch_align_pass(hipStream_t s, gsdf_table tab, float vs, float inv_vs, const float* pts, long long n,
                            gsdf_align_state* st, double* part, float conv_sq, float damping, int max_passes, float* trace,
                            int loss, float scale) {
    const int grid = gsdf_align_grid(n);
    if (loss >= 0) {
        hipLaunchKernelGGL(k_align_pass_robust, dim3(grid), dim3(GSDF_ALIGN_BLOCK), 0, s, tab, vs, inv_vs, pts, n, st, part, loss, scale);
        hipLaunchKernelGGL(k_align_head_robust, dim3(1), dim3(ALIGN_HEAD_THREADS), 0, s, st, part, grid, conv_sq, damping, max_passes, trace);
        return;
    }
    hipLaunchKernelGGL(k_align_pass, dim3(grid), dim3(GSDF_ALIGN_BLOCK), 0, s, tab, vs, inv_vs, pts, n, st, part);
    hipLaunchKernelGGL(k_align_head, dim3(1), dim3(ALIGN_HEAD_THREADS), 0, s, st, part, grid, conv_sq, damping, max_passes, trace);
}

void gsdf_launch_align_pass_multi(hipStream_t s, gsdf_table tab, float vs, float inv_vs, const float* pts, long long n,
                                  gsdf_align_state* st, double* part, const int* live, int n_live, float conv_sq, float damping,
                                  int max_passes, float* trace, float* last, int loss, float scale) {
    if (n_live < 1) return;
    const int grid = gsdf_align_grid(n);
    if (loss >= 0) {
        hipLaunchKernelGGL(k_align_pass_multi_robust, dim3(grid, n_live), dim3(GSDF_ALIGN_BLOCK), 0, s, tab, vs, inv_vs, pts, n, st, part,
                           live, loss, scale);
        hipLaunchKernelGGL(k_align_head_multi_robust, dim3(n_live), dim3(ALIGN_HEAD_THREADS), 0, s, st, part, grid, conv_sq, damping,
                           max_passes, trace, last, live);
        return;
    }
    hipLaunchKernelGGL(k_align_pass_multi, dim3(grid, n_live), dim3(GSDF_ALIGN_BLOCK), 0, s, tab, vs, inv_vs, pts, n, st, part, live);
    hipLaunchKernelGGL(k_align_head_multi, dim3(n_live), dim3(ALIGN_HEAD_THREADS), 0, s, st, part, grid, conv_sq, damping, max_passes,
                       trace, last, live);
}

/* ------------------------------------------------------------------------------------------------
 * residuals under a pose
 * ---------------------------------------------------------------------------------------------- */
struct align_pose7 { float v[7]; };
/* What a pass from `pose` sees per point: p = R x + t as align_pass_body forms it, then gsdf_grad_sample.  w[i] = the voxel's
 * weight, 0 for a missing voxel or a point that is not finite after the transform; phi[i] = the distance, 0 where w[i] == 0.
 * One lane per point (grid-stride behind the grid cap), no reductions. */
__global__ __launch_bounds__(256) void k_align_residuals(gsdf_table tab, float vs, float inv_vs, const float* __restrict__ pts, long long n,
                                                         align_pose7 pose, float* __restrict__ phi_out, float* __restrict__ w_out) {
    float R[9];
    gsdf_quat_to_R(pose.v + 3, R);
    const gsdf_v3 t = { pose.v[0], pose.v[1], pose.v[2] };
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const gsdf_v3 x = { pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] };
        const gsdf_v3 p = gsdf_rigid_apply(R, t, x);
        float w0 = 0.f, phi = 0.f;
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            gsdf_v3 g;
            gsdf_grad_sample(tab, vs, inv_vs, p, w0, phi, g);
        }
        phi_out[i] = phi;
        w_out[i] = w0;
    }
}

void gsdf_launch_align_residuals(hipStream_t s, gsdf_table tab, float vs, float inv_vs, const float* pts, long long n,
                                 const float pose7[7], float* phi_out, float* w_out) {
    if (n <= 0) return;
    align_pose7 pose;
    for (int i = 0; i < 7; ++i) pose.v[i] = pose7[i];
    const long long b = (n + 255) / 256;
    hipLaunchKernelGGL(k_align_residuals, dim3((unsigned int)(b > 65536 ? 65536 : b)), dim3(256), 0, s, tab, vs, inv_vs, pts, n, pose,
                       phi_out, w_out);
}

/* ------------------------------------------------------------------------------------------------
 * surface cloud
 * ---------------------------------------------------------------------------------------------- */
/* one row of extract_pc (:184-192) from a stored voxel; false = the voxel gives none */
__device__ __forceinline__ bool surface_row(const gsdf_payload& sl, float vs, float vs_2, int x, int y, int z, float (&r)[6]) {
    if (!(sl.w > 0.f) || sl.w < 5) return false;                           /* the voxel exists; :184-185 */
    const gsdf_v3 gn = gsdf_normalized3(gsdf_v3{ sl.gx, sl.gy, sl.gz });
    const gsdf_v3 g = { 1.2f * gn.x, 1.2f * gn.y, 1.2f * gn.z };           /* :186 */
    const float dist = sl.s / sl.w;
    const gsdf_v3 d = { dist * g.x, dist * g.y, dist * g.z };              /* :187 */
    if (!(fabsf(d.x) < vs_2 && fabsf(d.y) < vs_2 && fabsf(d.z) < vs_2)) return false;   /* :188 */
    r[0] = vs * (float)x - d.x; r[1] = vs * (float)y - d.y; r[2] = vs * (float)z - d.z; /* :191 */
    r[3] = -g.x; r[4] = -g.y; r[5] = -g.z;                                 /* :192 */
    return true;
}

/* the slots that pass the gates: packed key and slot appended through `counter` (keys == nullptr: count only) */
__global__ __launch_bounds__(256) void k_surface_flag(gsdf_table tab, size_t n_slots, float vs, float vs_2, unsigned long long* __restrict__ keys,
                                                      uint32_t* __restrict__ slots, unsigned long long* counter, long long max_n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n_slots; i += stride) {
        const unsigned long long bk = tab.bkeys[i / GSDF_BLOCK_VOX];      /* one block per wavefront */
        if (bk == GSDF_KEY_EMPTY) continue;
        const gsdf_payload sl = tab.vox[i];
        const unsigned long long key = gsdf_voxel_key(bk, (uint32_t)(i % GSDF_BLOCK_VOX));
        int x, y, z;
        gsdf_key_unpack(key, &x, &y, &z);
        float r[6];
        if (!surface_row(sl, vs, vs_2, x, y, z, r)) continue;
        const unsigned long long o = atomicAdd(counter, 1ull);
        if (!keys || (long long)o >= max_n) continue;
        keys[o] = key; slots[o] = (uint32_t)i;
    }
}
/* row i of the cloud from the i-th slot in key order */
__global__ __launch_bounds__(256) void k_surface_rows(gsdf_table tab, float vs, float vs_2, const unsigned long long* __restrict__ skeys,
                                                      const uint32_t* __restrict__ sslots, size_t n, float* __restrict__ rows6) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int x, y, z;
    gsdf_key_unpack(skeys[i], &x, &y, &z);
    float r[6];
    (void)surface_row(tab.vox[sslots[i]], vs, vs_2, x, y, z, r);           /* passed in k_surface_flag */
#pragma unroll
    for (int k = 0; k < 6; ++k) rows6[6 * i + k] = r[k];
}

void gsdf_launch_surface_flag(hipStream_t s, gsdf_table tab, size_t n_slots, float vs, unsigned long long* keys, uint32_t* slots,
                              unsigned long long* counter, long long max_n) {
    const float vs_2 = (float)(.5 * vs);                                   /* :179 */
    hipLaunchKernelGGL(k_surface_flag, dim3(2048), dim3(256), 0, s, tab, n_slots, vs, vs_2, keys, slots, counter, max_n);
}
void gsdf_launch_surface_rows(hipStream_t s, gsdf_table tab, float vs, const unsigned long long* skeys, const uint32_t* sslots, size_t n,
                              float* rows6) {
    if (n == 0) return;
    const float vs_2 = (float)(.5 * vs);
    hipLaunchKernelGGL(k_surface_rows, dim3((unsigned int)((n + 255) / 256)), dim3(256), 0, s, tab, vs, vs_2, skeys, sslots, n, rows6);
}
