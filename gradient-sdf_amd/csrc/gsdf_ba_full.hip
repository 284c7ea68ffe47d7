/*
 * gsdf_ba_full.hip -- PhotoBA's coupled pose step, PhotometricOptimizer::solvePoseFull
 * (ps_optimizer/PhotometricOptimizer.cpp:392-496): the off-diagonal 6x6 blocks of the 6n x 6n normal matrix.
 *
 * Every gated voxel j (|dist| <= vs, :406) that counts the keyframes i1 < i2 adds -inv_Nj * J_i1j^T J_i2j to block (i1, i2)
 * (:475-479).  With one row per (voxel, colour channel) -- the 6n-wide row a_jc that holds J_ij[c, :] at columns 6i.. for the
 * keyframes the voxel counts and zeros elsewhere -- all those blocks together are the dense symmetric contraction
 *
 *     S = sum_j inv_Nj * sum_c a_jc^T a_jc,        H[i1, i2] = -S[i1, i2]  (i1 != i2)
 *
 * which is what this file computes, on the exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32: an f32 FMA chain in k order,
 * nothing wider inside).  The diagonal blocks and the right-hand side are the decoupled step's sums (k_ba_pose, gsdf_ba.hip).
 *
 *   k_ba_full         a workgroup streams slabs of 16 gated voxels: one lane per (voxel, keyframe) pair computes J_ij exactly as
 *                     k_ba_pose does and stores its three rows in LDS; the eight waves then run the 32x32x2 products over the
 *                     32x32 tiles of the upper triangle, each wave keeping its tiles' accumulators in registers for the whole
 *                     stream, and write them to a per-workgroup partial at the end
 *   k_ba_full_reduce  adds the partials in workgroup order (a fixed order: the same bytes from run to run) and writes -S into
 *                     the off-diagonal blocks of H, both triangles from the one upper value (H is bit-symmetric)
 *
 * No float atomics anywhere.  The first loop of solvePoseFull (which keyframes a voxel counts, and their number Nj) is one
 * predicate per (voxel, keyframe) pair here -- visible, projects into the image, not truncated -- so the kernel has one route
 * and does not read the mean cache: the mean itself is only needed by the right-hand side.
 */
#include "gsdf_ba_shared.h"
#include <cstring>

#define BAF_THREADS 512
#define BAF_WAVES (BAF_THREADS / 64)
#define BAF_VOX 16                       /* voxels per slab */
#define BAF_ROWS (3 * BAF_VOX)           /* one row per voxel and colour channel */
#define BAF_MAX_NT 12                    /* 32-column tiles of 6 * 64 = 384 columns */
#define BAF_LD (32 * BAF_MAX_NT + 4)     /* row stride in floats: + 4 spreads the (voxel, keyframe) lanes' stores over the banks */
#define BAF_MAX_TILES (BAF_MAX_NT * (BAF_MAX_NT + 1) / 2)
#define BAF_SLOTS ((BAF_MAX_TILES + BAF_WAVES - 1) / BAF_WAVES)   /* tiles per wave: 10 x 16 accumulator registers */
#define BAF_BLOCKS 256                   /* one workgroup per CU (74 KB of LDS, 2 waves per SIMD); the partials are
                                          * BAF_BLOCKS x tiles x 4 KB = 80 MB at n = 64, 0.8 MB at n = 6 */

typedef float baf_acc __attribute__((ext_vector_type(16)));

/* tile t of the upper triangle, row-major: (0,0) (0,1) .. (0,nt-1) (1,1) .. */
__device__ __forceinline__ void baf_tile(int t, int nt, int* ti, int* tj) {
    int r = 0;
    while (t >= nt - r) { t -= nt - r; ++r; }
    *ti = r; *tj = r + t;
}
/* the keyframes with a column inside tile column c (columns 32c .. 32c + 31 of 6 per keyframe) */
__device__ __forceinline__ unsigned long long baf_tile_keyframes(int c) {
    const int lo = (32 * c) / 6, hi = min((32 * c + 31) / 6, 63);
    const unsigned long long upto_hi = hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull);
    return upto_hi & ~((1ull << lo) - 1ull);
}

__global__ __launch_bounds__(BAF_THREADS) void k_ba_full(ba_args a, int nt, float* part /* [gridDim.x][tiles][16][64] */) {
    __shared__ float X[BAF_ROWS * BAF_LD];
    __shared__ ba_voxel sv[BAF_VOX];
    __shared__ uint32_t sslot[BAF_VOX];
    __shared__ int sok[BAF_VOX];
    __shared__ unsigned long long sseen[BAF_VOX];
    __shared__ float sinv[BAF_ROWS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_up = nt * (nt + 1) / 2;
    for (int i = tid; i < BAF_ROWS * BAF_LD; i += BAF_THREADS) X[i] = 0.f;     /* the padding columns stay zero */
    baf_acc acc[BAF_SLOTS];
    int col_i[BAF_SLOTS], col_j[BAF_SLOTS];                                    /* wave-uniform */
    /* A[i = lane & 31][k = lane >> 5] and B[k = lane >> 5][j = lane & 31] of a 32x32x2 product: row k, column 32 * tile + .. */
    const float* const Xl = X + (lane >> 5) * BAF_LD + (lane & 31);
#pragma unroll
    for (int s = 0; s < BAF_SLOTS; ++s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
        int ti = 0, tj = 0;
        if (wave + BAF_WAVES * s < n_up) baf_tile(wave + BAF_WAVES * s, nt, &ti, &tj);
        col_i[s] = ti; col_j[s] = tj;
    }
    const size_t n_items = a.gate_list ? (size_t)*a.gate_count : a.n_slots;
    const size_t n_slabs = (n_items + BAF_VOX - 1) / BAF_VOX;
    for (size_t slab = blockIdx.x; slab < n_slabs; slab += gridDim.x) {
        if (tid < BAF_VOX) {
            const size_t item = slab * BAF_VOX + tid;
            bool ok = false;
            uint32_t slot = 0u;
            ba_voxel v;
            if (item < n_items) {
                slot = a.gate_list ? a.gate_list[item] : (uint32_t)item;
                ok = ba_load_voxel(a, slot, &v) && !(fabsf(v.dist) > a.vs);    /* :406 */
            }
            if (ok) sv[tid] = v;
            sslot[tid] = slot; sok[tid] = ok ? 1 : 0; sseen[tid] = 0ull;
        }
        __syncthreads();                                   /* (also: every wave is through the last slab's products) */
        for (int p = tid; p < BAF_VOX * a.n; p += BAF_THREADS) {
            const int vx = p & (BAF_VOX - 1), i = p / BAF_VOX;
            float J[18];
#pragma unroll
            for (int k = 0; k < 18; ++k) J[k] = 0.f;
            if (sok[vx] && ba_visible(a, sslot[vx], i)) {
                const ba_voxel v = sv[vx];
                gsdf_v3 pt; float m, n;
                const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
                /* the first loop's rule for counting keyframe i (k_ba_pose): it projects into the image and TRUNC_L2 keeps it */
                if (ba_project(a, v, i, &pt, &m, &n) && !(a.trunc_sq >= 0.f && ba_truncated(a, ba_interp(n, m, im)))) {
                    gsdf_v3 A, g0, g1;
                    ba_sample3(n, m, im, &A, &g0, &g1);
                    float G[9];
                    ba_pi_grad_from(a, pt, g0, g1, G);
                    const float* Ri = a.R + 9 * i;
                    const float S[9] = { 0.f, -pt.z, pt.y, pt.z, 0.f, -pt.x, -pt.y, pt.x, 0.f };
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) {                          /* computeJc :206-233, as in k_ba_pose */
                            J[6 * r + c] = -gsdf_sum3(G[3 * r] * Ri[3 * c], G[3 * r + 1] * Ri[3 * c + 1], G[3 * r + 2] * Ri[3 * c + 2]);
                            J[6 * r + 3 + c] = gsdf_sum3(G[3 * r] * S[c], G[3 * r + 1] * S[3 + c], G[3 * r + 2] * S[6 + c]);
                        }
                    atomicOr(&sseen[vx], 1ull << (i & 63));                    /* (an integer OR: the order does not matter) */
                }
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) {                                      /* zeros where the voxel does not count keyframe i */
                float2* row = reinterpret_cast<float2*>(X + (3 * vx + r) * BAF_LD + 6 * i);
                row[0] = make_float2(J[6 * r], J[6 * r + 1]);
                row[1] = make_float2(J[6 * r + 2], J[6 * r + 3]);
                row[2] = make_float2(J[6 * r + 4], J[6 * r + 5]);
            }
        }
        __syncthreads();
        if (tid < BAF_ROWS) {
            const int Nj = __popcll(sseen[tid / 3]);
            sinv[tid] = Nj ? (float)(1. / (double)(float)Nj) : 0.f;            /* inv_Nj, as the decoupled step has it */
        }
        __syncthreads();
        unsigned long long any = 0ull;                                         /* keyframes some voxel of the slab counts */
#pragma unroll
        for (int k = 0; k < BAF_VOX; ++k) any |= sseen[k];
        const float* const inv = sinv + (lane >> 5);                          /* the row's inv_Nj scales the B operand on the read */
#pragma unroll
        for (int s = 0; s < BAF_SLOTS; ++s) {
            if (wave + BAF_WAVES * s >= n_up) continue;                        /* wave-uniform */
            /* a tile column none of the slab's voxels has a keyframe in is all zeros: its products change nothing */
            if (!(any & baf_tile_keyframes(col_i[s])) || !(any & baf_tile_keyframes(col_j[s]))) continue;
            const float* pa = Xl + 32 * col_i[s];
            const float* pb = Xl + 32 * col_j[s];
#pragma unroll
            for (int k = 0; k < BAF_ROWS / 2; ++k)                             /* rows 2k, 2k + 1: the k of one 32x32x2 product */
                acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * k * BAF_LD], inv[2 * k] * pb[2 * k * BAF_LD], acc[s], 0, 0, 0);
        }
    }
#pragma unroll
    for (int s = 0; s < BAF_SLOTS; ++s) {
        const int t = wave + BAF_WAVES * s;
        if (t >= n_up) continue;
        float* out = part + ((size_t)blockIdx.x * n_up + t) * 1024 + lane;
#pragma unroll
        for (int r = 0; r < 16; ++r) out[64 * r] = acc[s][r];
    }
}

/* one lane per element of an upper-triangle tile: the partials of workgroups 0, 1, .. in that order; -S goes to H[gi, gj] and
 * H[gj, gi] of every off-diagonal 6x6 block (the diagonal blocks are the pose sweep's) */
__global__ __launch_bounds__(256) void k_ba_full_reduce(const float* part, int n_blocks, int nt, int n, float* H /* (6n)^2 */) {
    const int n_up = nt * (nt + 1) / 2;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_up * 1024) return;
    int ti, tj;
    baf_tile(e >> 10, nt, &ti, &tj);
    const int reg = (e >> 6) & 15, lane = e & 63;
    const int gi = 32 * ti + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), gj = 32 * tj + (lane & 31);   /* the C / D map */
    const int N = 6 * n;
    if (gi >= N || gj >= N || gi / 6 >= gj / 6) return;
    float s = 0.f;
    for (int b = 0; b < n_blocks; ++b) s += part[(size_t)b * n_up * 1024 + e];
    const float h = 0.f - s;                                                   /* (an empty block is +0, not -0) */
    H[(size_t)gi * N + gj] = h;
    H[(size_t)gj * N + gi] = h;
}

static int baf_tiles(int n) { const int nt = (6 * n + 31) / 32; return nt * (nt + 1) / 2; }
size_t gsdf_ba_full_part_floats(int n) { return (size_t)BAF_BLOCKS * baf_tiles(n) * 1024; }
void gsdf_launch_ba_full(hipStream_t s, const gsdf_ba_dev& d, float* part, float* H) {
    ba_args a; std::memcpy(&a, &d, sizeof(a));
    const int nt = (6 * a.n + 31) / 32;
    hipLaunchKernelGGL(k_ba_full, dim3(BAF_BLOCKS), dim3(BAF_THREADS), 0, s, a, nt, part);
    hipLaunchKernelGGL(k_ba_full_reduce, dim3((baf_tiles(a.n) * 1024 + 255) / 256), dim3(256), 0, s, part, BAF_BLOCKS, nt, a.n, H);
}
