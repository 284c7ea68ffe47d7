/*
 * gsdf_ba_shared.h -- the device helpers the PhotoBA sweeps share (gsdf_ba.hip: energy, decoupled pose step, distance step;
 * gsdf_ba_full.hip: the coupled pose system): the kernels' argument block, the voxel load, the vis_ test, the projection and
 * the image sampling of PhotometricOptimizer.cpp, operation for operation.
 */
#ifndef GSDF_BA_SHARED_H_
#define GSDF_BA_SHARED_H_
#include "gsdf_kernels.h"
#include "gsdf_math.h"
#include "gsdf_interp.h"

#include <hip/hip_runtime.h>

/* computeImageGradient(m = row, n = col, direction) -- :80-140 */
__device__ __forceinline__ gsdf_v3 ba_grad(float m, float n, const ba_img& im, int direction) {
    const int x = (int)floorf(m), y = (int)floorf(n);
    const float w01 = m - x, w11 = n - y;
    const float w00 = (float)(1.0 - w01), w10 = (float)(1.0 - w11);
    float v0[3] = { 0.f, 0.f, 0.f }, v1[3] = { 0.f, 0.f, 0.f };
    float a = 1.f, b = 0.f;
#define BA_DIFF(o, r1, c1, r0, c0) { const float *p1 = ba_px(im, r1, c1), *p0 = ba_px(im, r0, c0); o[0] = p1[0] - p0[0]; o[1] = p1[1] - p0[1]; o[2] = p1[2] - p0[2]; }
    if (direction == 0) {
        if ((x + 1) < im.H && (y + 1) < im.W) { BA_DIFF(v0, x, y + 1, x, y); BA_DIFF(v1, x + 1, y + 1, x + 1, y); a = w00; b = w01; }
        else if ((x + 1) >= im.H) { if ((y + 1) < im.W) { BA_DIFF(v0, x, y + 1, x, y); } else { BA_DIFF(v0, x, y, x, y - 1); } }
        else { BA_DIFF(v0, x, y, x, y - 1); BA_DIFF(v1, x + 1, y, x + 1, y - 1); a = w00; b = w01; }
    } else {
        if ((x + 1) < im.H && (y + 1) < im.W) { BA_DIFF(v0, x + 1, y, x, y); BA_DIFF(v1, x + 1, y + 1, x, y + 1); a = w10; b = w11; }
        else if ((x + 1) >= im.H && (y + 1) < im.W) { BA_DIFF(v0, x, y, x - 1, y); BA_DIFF(v1, x, y + 1, x - 1, y + 1); a = w10; b = w11; }
        else { if ((x + 1) < im.H) { BA_DIFF(v0, x + 1, y, x, y); } else { BA_DIFF(v0, x, y, x - 1, y); } }
    }
#undef BA_DIFF
    return gsdf_v3{ a * v0[2] + b * v1[2], a * v0[1] + b * v1[1], a * v0[0] + b * v1[0] };
}

struct ba_args {
    gsdf_table tab;
    size_t n_slots;
    const uint32_t* vis;
    int vis_words;
    int n, W, H;
    const float* images;      /* n x H x W x 3 BGR */
    const float* R;           /* n x 9 */
    const float* t;           /* n x 3 */
    const int* frame_idx;
    float fx, fy, cx, cy, vs, reg_weight;
    float trunc_sq;
    const uint32_t* gate_list;      /* nullable: slots of the voxels with |dist| <= vs, in slot order (gsdf_ba_compact) */
    const unsigned long long* gate_count;
    void* mean_cache;               /* nullable: ba_mean per entry of gate_list (see gsdf_ba_dev) */
};
/* what the first loop of getEnergy / solvePose finds for a voxel: the mean intensity over the keyframes it is seen in (already
 * scaled by 1 / Nj), their number and their set */
struct __attribute__((aligned(8))) ba_mean { float mx, my, mz; int nj; unsigned long long seen; };
static_assert(sizeof(ba_args) == sizeof(gsdf_ba_dev), "ba_args mirrors gsdf_ba_dev (the launchers memcpy one into the other)");

struct ba_voxel { float dist, w; gsdf_v3 grad, gn, c; };

__device__ __forceinline__ bool ba_load_voxel(const ba_args& a, size_t slot, ba_voxel* v) {
    const unsigned long long bk = a.tab.bkeys[slot / GSDF_BLOCK_VOX];
    if (bk == GSDF_KEY_EMPTY) return false;
    const gsdf_payload p = a.tab.vox[slot];
    if (!(p.w > 0.f)) return false;                    /* the voxel exists iff w > 0 */
    int x, y, z;
    gsdf_key_unpack(gsdf_voxel_key(bk, (uint32_t)(slot % GSDF_BLOCK_VOX)), &x, &y, &z);
    v->w = p.w; v->dist = p.s / p.w;
    v->grad = gsdf_v3{ p.gx, p.gy, p.gz };
    v->gn = gsdf_normalized3(v->grad);
    v->c = gsdf_v3{ a.vs * (float)x, a.vs * (float)y, a.vs * (float)z };
    return true;
}
__device__ __forceinline__ bool ba_visible(const ba_args& a, size_t slot, int i) {
    const int f = a.frame_idx[i];
    if (f >= 32 * a.vis_words) return false;
    return (a.vis[slot * a.vis_words + (f >> 5)] >> (f & 31)) & 1u;
}
/* LossFunction::TRUNC_L2 (loss.h:45): a keyframe whose intensity residual is too large is left out of the voxel's sums
 * (solveDist :364, solvePose :542); every other loss value behaves like L2 in the reference's code */
__device__ __forceinline__ bool ba_truncated(const ba_args& a, const gsdf_v3& A) {
    return a.trunc_sq >= 0.f && fmaxf(A.x * A.x, fmaxf(A.y * A.y, A.z * A.z)) > a.trunc_sq;
}

/* projection shared by getIntensity / computeJc / computeJdOneFrame (:165-177) */
__device__ __forceinline__ bool ba_project(const ba_args& a, const ba_voxel& v, int i, gsdf_v3* point, float* m, float* n) {
    const float* Ri = a.R + 9 * i;
    const float* ti = a.t + 3 * i;
    const gsdf_v3 d = { v.c.x - v.dist * v.gn.x - ti[0], v.c.y - v.dist * v.gn.y - ti[1], v.c.z - v.dist * v.gn.z - ti[2] };
    const gsdf_v3 p = { gsdf_sum3(Ri[0] * d.x, Ri[3] * d.y, Ri[6] * d.z), gsdf_sum3(Ri[1] * d.x, Ri[4] * d.y, Ri[7] * d.z),
                        gsdf_sum3(Ri[2] * d.x, Ri[5] * d.y, Ri[8] * d.z) };
    const float z_inv = (float)(1. / (double)p.z);
    *m = a.fx * p.x * z_inv + a.cx;
    *n = a.fy * p.y * z_inv + a.cy;
    *point = p;
    return !(*m < 0 || *m >= a.W || *n < 0 || *n >= a.H);
}
/* interpolateImage + both computeImageGradient directions at one position (row m, column n).  Away from the image border all
 * three read the SAME four pixels -- (x, y), (x+1, y), (x, y+1), (x+1, y+1) -- so they are read once (4 scattered 12-byte loads
 * instead of 12: the distance and pose sweeps are bound by the rate at which the texture-address path takes scattered
 * addresses, ~0.4 T per second at 37 M observations per millisecond); the arithmetic per output is that of ba_interp / ba_grad,
 * operation for operation.  At the border the three functions are called as they are. */
__device__ __forceinline__ void ba_sample3(float m, float n, const ba_img& im, gsdf_v3* A, gsdf_v3* g0, gsdf_v3* g1) {
    const int x = (int)floorf(m), y = (int)floorf(n);
    if (__builtin_expect(!((x + 1) < im.H && (y + 1) < im.W), 0)) {
        *A = ba_interp(m, n, im); *g0 = ba_grad(m, n, im, 0); *g1 = ba_grad(m, n, im, 1);
        return;
    }
    const float *pa = ba_px(im, x + 1, y), *pb = ba_px(im, x, y);              /* (x+1, y+1) and (x, y+1) follow them in memory */
    float a[3], b[3], c[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { a[k] = pa[k]; c[k] = pa[3 + k]; b[k] = pb[k]; d[k] = pb[3 + k]; }
    const double w1 = (y + 1.0 - n) * (m - x), w2 = (y + 1.0 - n) * (x + 1.0 - m), w3 = (n - y) * (m - x), w4 = (n - y) * (x + 1.0 - m);
    float t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        t[k] = (((float)(w1 * (double)a[k]) + (float)(w2 * (double)b[k])) + (float)(w3 * (double)c[k])) + (float)(w4 * (double)d[k]);
    *A = gsdf_v3{ t[2], t[1], t[0] };
    const float w01 = m - x, w11 = n - y;
    const float w00 = (float)(1.0 - w01), w10 = (float)(1.0 - w11);
    float u0[3], u1[3], v0[3], v1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { u0[k] = d[k] - b[k]; u1[k] = c[k] - a[k]; v0[k] = a[k] - b[k]; v1[k] = c[k] - d[k]; }
    *g0 = gsdf_v3{ w00 * u0[2] + w01 * u1[2], w00 * u0[1] + w01 * u1[1], w00 * u0[0] + w01 * u1[0] };
    *g1 = gsdf_v3{ w10 * v0[2] + w11 * v1[2], w10 * v0[1] + w11 * v1[1], w10 * v0[0] + w11 * v1[0] };
}
/* G from already sampled gradients (ba_sample3) */
__device__ __forceinline__ void ba_pi_grad_from(const ba_args& a, const gsdf_v3& p, const gsdf_v3& g0, const gsdf_v3& g1, float* G) {
    const float z_inv = (float)(1. / (double)p.z), z_inv_sq = z_inv * z_inv;
    const float pg[6] = { a.fx * z_inv, 0.f, -a.fx * p.x * z_inv_sq, 0.f, a.fy * z_inv, -a.fy * p.y * z_inv_sq };
    const float ig[6] = { g0.x, g1.x, g0.y, g1.y, g0.z, g1.z };
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[3 * r + c] = ig[2 * r] * pg[c] + ig[2 * r + 1] * pg[3 + c];
}
__device__ __forceinline__ void ba_image_pi_grad(const ba_args& a, const gsdf_v3& p, float m, float n, int i, float* G) {
    const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
    const float z_inv = (float)(1. / (double)p.z), z_inv_sq = z_inv * z_inv;
    const gsdf_v3 g0 = ba_grad(n, m, im, 0), g1 = ba_grad(n, m, im, 1);
    const float pg[6] = { a.fx * z_inv, 0.f, -a.fx * p.x * z_inv_sq, 0.f, a.fy * z_inv, -a.fy * p.y * z_inv_sq };
    const float ig[6] = { g0.x, g1.x, g0.y, g1.y, g0.z, g1.z };
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) G[3 * r + c] = ig[2 * r] * pg[c] + ig[2 * r + 1] * pg[3 + c];
}

#endif /* GSDF_BA_SHARED_H_ */
