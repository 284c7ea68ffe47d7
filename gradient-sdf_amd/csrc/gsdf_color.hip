/*
 * gsdf_color.hip -- ColorUpsampler (ps_optimizer/ColorUpsampler.h/.cpp) over the HBM voxel table: sub-voxel albedo from the
 * keyframe images and the coloured point cloud (extractCloud), behind gsdf_color_compute / _export / _cloud (include/gsdf.h).
 *
 *   selection   init :143-146         voxels with |dist| < (float)(sqrt(3) vs): rocPRIM select over the slots (as gsdf_ba_compact)
 *   order       --                    packed (z, y, x) keys of the selection, radix-sorted with their slots (gsdf_sort.hip)
 *   k_color     computeColor :334-377 8 lanes per Hr voxel (SdfVoxelHr, SdfVoxel.h:83-101), one per sub-voxel
 *   k_cloud_*   extractCloud :251-330 per-voxel predicate and count, exclusive scan, compaction into 9-float rows
 *   k_hr_mesh   extractMesh :240-249  HrLayeredMarchingCubes::computeIsoSurface (mesh/HrLayeredMarchingCubes.cpp:359-822): 8 lanes
 *                                     per Hr voxel, one fine cube each; neighbours by binary search in the sorted keys
 *
 * The result is a snapshot, like the reference's SdfHrMap copy: it lives in buffers of its own, sorted by key, and later
 * fusion, BA steps or table growth leave it as it is until the next gsdf_color_compute.  The table is only read.
 */
#include "gsdf_ctx.h"
#include "gsdf_interp.h"
#include "gsdf_kernels.h"
#include "gsdf_math.h"
#include "gsdf_sweep.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>
#include <climits>
#include <cmath>
#include <vector>

#include "../../include/gsdf_mc_tables.h"

#define GSDF_COLOR_ROW 37            /* dist, weight, grad[3], d[8], r[8], g[8], b[8] */

/* ---- device ---------------------------------------------------------------------------------------------------------- */

/* init :143-146: the voxel exists (w > 0, as ba_load_voxel) and fabsf(dist) < (float)(sqrt(3.) * vs), strict, in float */
struct color_sel_pred {
    const unsigned long long* bkeys;
    const gsdf_payload* vox;
    float gate;
    __device__ bool operator()(const uint32_t& slot) const {
        if (bkeys[slot / GSDF_BLOCK_VOX] == GSDF_KEY_EMPTY) return false;
        const float2 ws = *reinterpret_cast<const float2*>(vox + slot);        /* w, s */
        if (!(ws.x > 0.f)) return false;
        return fabsf(ws.y / ws.x) < gate;
    }
};

__global__ __launch_bounds__(256) void k_color_keys(const uint32_t* __restrict__ list, const unsigned long long* __restrict__ bkeys,
                                                     unsigned long long* __restrict__ keys, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t slot = list[i];
    keys[i] = gsdf_voxel_key(bkeys[slot / GSDF_BLOCK_VOX], slot % GSDF_BLOCK_VOX);
}

/* getSubvoxelFloat :208-212, one coordinate: vs * (0.25f * (+-1) + idx) */
__device__ __forceinline__ float color_centre(float vs, int hi, int idx) { return vs * ((hi ? 0.25f : -0.25f) + (float)idx); }

struct color_args {
    gsdf_table tab;
    const uint32_t* slots;            /* the selected slots in (z, y, x) key order */
    long long n_vox;
    const uint32_t* vis;
    int vis_words;
    int n, W, H;
    const float* images;              /* n x H x W x 3 BGR */
    const float* R;                   /* n x 9, row-major */
    const float* t;                   /* n x 3 */
    const int* frame_idx;
    float fx, fy, cx, cy, vs;
    float* rows;                      /* n_vox x GSDF_COLOR_ROW */
    unsigned long long* obs;          /* device word: voxel x keyframe observations (added to) */
};

/* 8 lanes per Hr voxel, lane (i & 7) = sub-voxel i (x from bit 0, y from bit 1, z from bit 2): 8 voxels per wave64.  The keyframe
 * loop is uniform over the wave: a keyframe counts for a voxel only if all 8 of its sub-voxels project into the image
 * (getIntensity :181-197), and that is an 8-bit field of one __ballot.  The 8 sub-voxels of a voxel lie a quarter voxel apart,
 * so their bilinear taps fall on neighbouring pixels and mostly hit the same cache lines. */
__global__ __launch_bounds__(256) void k_color(color_args a) {
    const int lane = threadIdx.x & 63, sub = lane & 7, gbase = lane & ~7;
    const long long item = ((long long)blockIdx.x * 256 + threadIdx.x) >> 3;
    const bool live = item < a.n_vox;
    size_t slot = 0;
    float w = 0.f, dist = 0.f;
    gsdf_v3 g = { 0.f, 0.f, 0.f };
    int x = 0, y = 0, z = 0;
    uint32_t myword = 0u;
    if (live) {
        slot = a.slots[item];
        const unsigned long long bk = a.tab.bkeys[slot / GSDF_BLOCK_VOX];
        const gsdf_payload p = a.tab.vox[slot];
        w = p.w; dist = p.s / p.w;                                             /* as ba_load_voxel */
        g = gsdf_v3{ p.gx, p.gy, p.gz };
        gsdf_key_unpack(gsdf_voxel_key(bk, (uint32_t)(slot % GSDF_BLOCK_VOX)), &x, &y, &z);
        if (sub < a.vis_words) myword = a.vis[slot * a.vis_words + sub];     /* the voxel's vis_ words, once per group */
    }
    /* SdfVoxelHr(voxel, vs) -- SdfVoxel.h:83-101: grad normalised, d[i] = dist + vs4 * (+-g0 +- g1 +- g2) evaluated left to right
     * (a - b is a + (-b) exactly, so every sign pattern of :92-99 is (s0 + s1) + s2) */
    const gsdf_v3 gn = gsdf_normalized3(g);
    const float vs4 = 0.25f * a.vs;
    const float s0 = (sub & 1) ? gn.x : -gn.x, s1 = (sub & 2) ? gn.y : -gn.y, s2 = (sub & 4) ? gn.z : -gn.z;
    const float d = dist + vs4 * ((s0 + s1) + s2);
    /* getSubvoxelFloat :208-212: vs * (0.25f * corner + idx) */
    const gsdf_v3 c = { color_centre(a.vs, sub & 1, x), color_centre(a.vs, sub & 2, y), color_centre(a.vs, sub & 4, z) };
    const gsdf_v3 q = { c.x - gn.x * d, c.y - gn.y * d, c.z - gn.z * d };     /* centre_i - grad d[i] */
    const float Wf = (float)a.W, Hf = (float)a.H;
    gsdf_v3 sum = { 0.f, 0.f, 0.f };
    int count = 0;
    for (int i = 0; i < a.n; ++i) {                                            /* computeColor :346-365 */
        const int f = a.frame_idx[i];                                          /* wave-uniform */
        const int wi = f >> 5;
        uint32_t word = 0u;
        if (wi < a.vis_words) {                                                /* ba_visible's rule: bits past the vectors are unset */
            if (wi < 8) word = (uint32_t)__shfl((int)myword, gbase + wi);
            else if (live) word = a.vis[slot * a.vis_words + wi];
        }
        const bool seen = live && ((word >> (f & 31)) & 1u);
        if (!__any(seen)) continue;                                            /* wave-uniform skip */
        const float* Ri = a.R + 9 * i;
        const float* ti = a.t + 3 * i;
        /* getIntensity :175: R^T ((centre_i - grad d[i]) - t), summed as ba_project */
        const gsdf_v3 e = { q.x - ti[0], q.y - ti[1], q.z - ti[2] };
        const gsdf_v3 p = { gsdf_sum3(Ri[0] * e.x, Ri[3] * e.y, Ri[6] * e.z), gsdf_sum3(Ri[1] * e.x, Ri[4] * e.y, Ri[7] * e.z),
                            gsdf_sum3(Ri[2] * e.x, Ri[5] * e.y, Ri[8] * e.z) };
        const float m = (a.fx * p.x) / p.z + a.cx;                             /* :177-178, a true division */
        const float n = (a.fy * p.y) / p.z + a.cy;
        /* :181-197: the keyframe is dropped if any m or n is NaN or any sub-voxel falls outside [0,W) x [0,H) -- a NaN fails
         * every comparison below, so both rules are this one predicate */
        const bool inside = m >= 0.f && m < Wf && n >= 0.f && n < Hf;
        const unsigned long long b = __ballot(seen && inside);
        if (((b >> gbase) & 0xffull) != 0xffull) continue;
        const ba_img im = { a.W, a.H, a.images + (size_t)i * a.W * a.H * 3 };
        const gsdf_v3 A = ba_interp(n, m, im);                                 /* interpolateImage(n(i), m(i), img) */
        sum = gsdf_v3{ sum.x + A.x, sum.y + A.y, sum.z + A.z };
        ++count;
    }
    /* :369-373 and setAlbedo :217-235: (1.f / (float)count) * sum, then std::max(c, 0) and std::min(c, 1) -- a NaN (count 0)
     * passes both as NaN */
    const float inv = 1.f / (float)count;
    float col[3] = { inv * sum.x, inv * sum.y, inv * sum.z };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        col[k] = (col[k] < 0.f) ? 0.f : col[k];
        col[k] = (1.f < col[k]) ? 1.f : col[k];
    }
    if (live) {
        float* row = a.rows + (size_t)item * GSDF_COLOR_ROW;
        if (sub < 5) row[sub] = sub == 0 ? dist : sub == 1 ? w : sub == 2 ? gn.x : sub == 3 ? gn.y : gn.z;
        row[5 + sub] = d;
        row[13 + sub] = col[0];
        row[21 + sub] = col[1];
        row[29 + sub] = col[2];
    }
    /* observations (voxel x keyframe pairs that counted): one atomic per wave */
    unsigned int o = (live && sub == 0) ? (unsigned int)count : 0u;
    for (int off = 32; off > 0; off >>= 1) o += (unsigned int)__shfl_xor((int)o, off);
    if (lane == 0 && o) atomicAdd(a.obs, (unsigned long long)o);
}

/* extractCloud :259-300 for one Hr voxel of the snapshot: the bit mask of the sub-voxels that are emitted.  The reference's
 * "seen by at least one keyframe" test (:264-271) is implied by a colour that is not NaN: a voxel no keyframe counted has
 * count 0 and NaN albedo, and a keyframe counts only where its vis_ bit is set. */
__device__ __forceinline__ unsigned int color_cloud_mask(const float* row, float vs4, gsdf_v3* nrm) {
    const gsdf_v3 gg = gsdf_normalized3(gsdf_v3{ row[2], row[3], row[4] });  /* -v.grad.normalized(): normalised a second time */
    *nrm = gsdf_v3{ -gg.x, -gg.y, -gg.z };
    if (row[1] < 5) return 0u;                                                 /* :275 */
    unsigned int mask = 0u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float d = row[5 + i];
        const float dx = nrm->x * d, dy = nrm->y * d, dz = nrm->z * d;         /* voxel_normal * v.d.asDiagonal() */
        if (fabsf(dx) < vs4 && fabsf(dy) < vs4 && fabsf(dz) < vs4 && !isnan(row[13 + i]) && !isnan(row[21 + i]) && !isnan(row[29 + i]))
            mask |= 1u << i;
    }
    return mask;
}
__global__ __launch_bounds__(256) void k_cloud_count(const float* __restrict__ rows, size_t n, float vs4, uint32_t* __restrict__ counts) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    gsdf_v3 nrm;
    counts[v] = (uint32_t)__popc(color_cloud_mask(rows + v * GSDF_COLOR_ROW, vs4, &nrm));
}
/* rows9: point centre_i + dvec, normal, colour -- in the snapshot's voxel order, then by sub-voxel index */
__global__ __launch_bounds__(256) void k_cloud_emit(const unsigned long long* __restrict__ keys, const float* __restrict__ rows, size_t n,
                                                    float vs, float vs4, const uint32_t* __restrict__ offsets, float* __restrict__ out) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const float* row = rows + v * GSDF_COLOR_ROW;
    gsdf_v3 nrm;
    const unsigned int mask = color_cloud_mask(row, vs4, &nrm);
    if (!mask) return;
    int x, y, z;
    gsdf_key_unpack(keys[v], &x, &y, &z);
    float* o = out + (size_t)offsets[v] * 9;
    for (int i = 0; i < 8; ++i) {
        if (!((mask >> i) & 1u)) continue;
        const float d = row[5 + i];
        const float cx = color_centre(vs, i & 1, x), cy = color_centre(vs, i & 2, y), cz = color_centre(vs, i & 4, z);
        o[0] = cx + nrm.x * d; o[1] = cy + nrm.y * d; o[2] = cz + nrm.z * d;
        o[3] = nrm.x; o[4] = nrm.y; o[5] = nrm.z;
        o[6] = row[13 + i]; o[7] = row[21 + i]; o[8] = row[29 + i];
        o += 9;
    }
}

/* ---- host: gsdf_color_* --------------------------------------------------------------------------------------------------- */

static int cfail(int code, const std::string& msg) { return gsdf_fail(code, msg); }

/* the selection (rocPRIM select over the slot numbers) and the cloud's prefix sum, as the X_need / X pairs of gsdf_kernels.h */
static hipError_t color_select_need(const color_sel_pred& pred, size_t n_slots, size_t* need) {
    return gsdf_scratch_need(need, [&](size_t& b) {
        return rocprim::select(nullptr, b, rocprim::counting_iterator<uint32_t>(0u), (uint32_t*)nullptr, (unsigned long long*)nullptr, n_slots, pred, hipStream_t());
    });
}
static hipError_t color_select(const gsdf_dev<void>& tmp, const color_sel_pred& pred, uint32_t* list, unsigned long long* count, size_t n_slots,
                               hipStream_t s) {
    size_t b = tmp.bytes();
    return rocprim::select(tmp.get(), b, rocprim::counting_iterator<uint32_t>(0u), list, count, n_slots, pred, s);
}
static hipError_t color_scan_need(size_t n, size_t* need) {
    return gsdf_scratch_need(need, [n](size_t& b) { return rocprim::exclusive_scan(nullptr, b, (uint32_t*)0, (uint32_t*)0, 0u, n, rocprim::plus<uint32_t>(), hipStream_t()); });
}
static hipError_t color_scan(const gsdf_dev<void>& tmp, uint32_t* counts, uint32_t* offsets, size_t n, hipStream_t s) {
    size_t b = tmp.bytes();
    return rocprim::exclusive_scan(tmp.get(), b, counts, offsets, 0u, n, rocprim::plus<uint32_t>(), s);
}

int gsdf_color_compute(gsdf_ctx* c, int n, const float* images_bgr_host, const float* poses16_host, const int* frame_idx,
                       int64_t* n_voxels) {
    if (!c) return cfail(GSDF_ERR_INVALID, "null context");
    if (int rc = gsdf_flush_pending(c)) return rc;
    if (!c->frame.planes) return cfail(GSDF_ERR_INVALID, "gsdf_normals_init must be called first (image size and intrinsics)");
    if (c->map_type != GSDF_MAP_GRAD) return cfail(GSDF_ERR_INVALID, "ColorUpsampler needs the Gradient-SDF map (a base-sdf context has no gradient)");
    if (!c->map.vis) return cfail(GSDF_ERR_INVALID, "ColorUpsampler needs the vis_ bit-vectors: call gsdf_enable_vis before fusing");
    if (n < 1 || n > 64) return cfail(GSDF_ERR_INVALID, "bad argument (1..64 keyframes)");
    const bool from_ba = !images_bgr_host || !poses16_host || !frame_idx;
    if (from_ba && !c->ba_n) return cfail(GSDF_ERR_INVALID, "NULL images, poses or frame_idx name PhotoBA's: gsdf_ba_setup was not called");
    if (from_ba && n != c->ba_n) return cfail(GSDF_ERR_INVALID, "NULL images, poses or frame_idx name PhotoBA's: n must equal its keyframe count");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* poses and keyframe ids on the host first: the ids are checked, the poses split into R (row-major) and t */
    std::vector<int> fid((size_t)n);
    if (frame_idx) std::copy(frame_idx, frame_idx + n, fid.begin());
    else HIP_TRY(hipMemcpy(fid.data(), c->ba.frame_idx, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    for (int v : fid)
        if (v < 0) return cfail(GSDF_ERR_INVALID, "frame_idx: keyframe ids must be >= 0");
    std::vector<float> Rt((size_t)n * 12);
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k)
                Rt[9 * (size_t)i + 3 * r + k] = poses16_host ? poses16_host[16 * (size_t)i + 4 * r + k] : c->ba_R[9 * (size_t)i + 3 * r + k];
            Rt[9 * (size_t)n + 3 * (size_t)i + r] = poses16_host ? poses16_host[16 * (size_t)i + 4 * r + 3] : c->ba_t[3 * (size_t)i + r];
        }
    gsdf_color_state* S = &c->color;
    S->valid = false; S->cloud_n = -1;
    HIP_TRY(S->Rt.grow(Rt.size()));
    HIP_TRY(S->fidx.grow((size_t)n));
    HIP_TRY(S->words.grow(2));
    HIP_TRY(S->list.grow(c->n_slots));
    HIP_TRY(hipMemcpyAsync(S->Rt, Rt.data(), Rt.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(S->fidx, fid.data(), fid.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const float* images = c->ba.images;                                          /* NULL: gsdf_ba_setup's, no second upload */
    if (images_bgr_host) {
        const size_t cnt = (size_t)n * c->W * c->H * 3;
        HIP_TRY(S->images.grow(cnt));
        HIP_TRY(hipMemcpyAsync(S->images, images_bgr_host, cnt * sizeof(float), hipMemcpyHostToDevice, c->stream));
        images = S->images;
    }
    HIP_TRY(hipMemsetAsync(S->words, 0, 2 * sizeof(unsigned long long), c->stream));
    /* selection: the slots of the kept voxels, in slot order */
    const float gate = (float)(std::sqrt(3.) * c->voxel_size);                   /* init :143 */
    const color_sel_pred pred{ c->tab.bkeys, c->tab.vox, gate };
    size_t need = 0;
    HIP_TRY(color_select_need(pred, c->n_slots, &need));
    HIP_TRY(S->tmp.grow(need));
    HIP_TRY(color_select(S->tmp, pred, S->list, S->words, c->n_slots, c->stream));
    unsigned long long N = 0;
    HIP_TRY(hipMemcpyAsync(&N, S->words, sizeof(N), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* order: (z, y, x) keys of the selection sorted together with their slots */
    HIP_TRY(S->keys_in.grow((size_t)N));
    HIP_TRY(S->keys.grow((size_t)N));
    HIP_TRY(S->slots.grow((size_t)N));
    HIP_TRY(S->rows.grow((size_t)N * GSDF_COLOR_ROW));
    if (N) {
        hipLaunchKernelGGL(k_color_keys, dim3((unsigned int)((N + 255) / 256)), dim3(256), 0, c->stream, S->list, c->tab.bkeys, S->keys_in, (size_t)N);
        need = 0;
        HIP_TRY(gsdf_sort_pairs_u64_need((size_t)N, &need));
        HIP_TRY(S->tmp.grow(need));
        HIP_TRY(gsdf_sort_pairs_u64(S->tmp, S->keys_in, S->keys, S->list, S->slots, (size_t)N, c->stream));
        color_args a;
        a.tab = c->tab; a.slots = S->slots; a.n_vox = (long long)N;
        a.vis = c->map.vis; a.vis_words = c->vis_words;
        a.n = n; a.W = c->W; a.H = c->H;
        a.images = images; a.R = S->Rt; a.t = S->Rt + 9 * (size_t)n; a.frame_idx = S->fidx;
        a.fx = c->K[0]; a.fy = c->K[4]; a.cx = c->K[2]; a.cy = c->K[5]; a.vs = c->voxel_size;
        a.rows = S->rows; a.obs = S->words + 1;
        hipLaunchKernelGGL(k_color, dim3((unsigned int)((8 * N + 255) / 256)), dim3(256), 0, c->stream, a);
        HIP_TRY(hipGetLastError());
    }
    unsigned long long obs = 0;
    HIP_TRY(hipMemcpyAsync(&obs, S->words + 1, sizeof(obs), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    S->n = (long long)N; S->obs = (long long)obs; S->vs = c->voxel_size;
    S->valid = true;
    if (n_voxels) *n_voxels = (int64_t)N;
    return GSDF_OK;
}

int gsdf_color_counters(gsdf_ctx* c, int64_t* voxels, int64_t* observations) {
    if (!c || !voxels || !observations) return cfail(GSDF_ERR_INVALID, "null argument");
    if (!c->color.valid) return cfail(GSDF_ERR_INVALID, "gsdf_color_compute was not called (or the map was reset)");
    *voxels = c->color.n; *observations = c->color.obs;
    return GSDF_OK;
}

int gsdf_color_export(gsdf_ctx* c, int32_t* keys, float* rows, int64_t max_n, int64_t* n) {
    if (!c) return cfail(GSDF_ERR_INVALID, "null context");
    if (!c->color.valid) return cfail(GSDF_ERR_INVALID, "gsdf_color_compute was not called (or the map was reset)");
    const gsdf_color_state* S = &c->color;
    if (n) *n = S->n;
    if (S->n == 0 || max_n <= 0 || (!keys && !rows)) return GSDF_OK;
    if (max_n < S->n) return cfail(GSDF_ERR_INVALID, "export buffer too small");
    HIP_TRY(hipSetDevice(c->device));
    if (rows) HIP_TRY(hipMemcpy(rows, S->rows, (size_t)S->n * GSDF_COLOR_ROW * sizeof(float), hipMemcpyDeviceToHost));
    if (keys) {
        std::vector<unsigned long long> hk((size_t)S->n);
        HIP_TRY(hipMemcpy(hk.data(), S->keys, hk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < hk.size(); ++i) {
            int x, y, z;
            gsdf_key_unpack(hk[i], &x, &y, &z);
            keys[3 * i] = x; keys[3 * i + 1] = y; keys[3 * i + 2] = z;
        }
    }
    return GSDF_OK;
}

int gsdf_color_cloud(gsdf_ctx* c, float* rows9, int64_t max_n, int64_t* n) {
    if (!c) return cfail(GSDF_ERR_INVALID, "null context");
    if (!c->color.valid) return cfail(GSDF_ERR_INVALID, "gsdf_color_compute was not called (or the map was reset)");
    gsdf_color_state* S = &c->color;
    HIP_TRY(hipSetDevice(c->device));
    if (S->cloud_n < 0) {                                                      /* predicate, prefix sum, compaction */
        const size_t N = (size_t)S->n;
        const float vs4 = (float)(.25 * S->vs);                                /* extractCloud :254 */
        unsigned long long total = 0;
        if (N) {
            HIP_TRY(S->counts.grow(N));
            HIP_TRY(S->offsets.grow(N));
            const dim3 grid((unsigned int)((N + 255) / 256));
            hipLaunchKernelGGL(k_cloud_count, grid, dim3(256), 0, c->stream, S->rows, N, vs4, S->counts);
            size_t need = 0;
            HIP_TRY(color_scan_need(N, &need));
            HIP_TRY(S->tmp.grow(need));
            HIP_TRY(color_scan(S->tmp, S->counts, S->offsets, N, c->stream));
            uint32_t last[2] = { 0u, 0u };
            HIP_TRY(gsdf_scan_total_read(c->stream, S->offsets, S->counts, N, last));
            HIP_TRY(hipStreamSynchronize(c->stream));
            total = (unsigned long long)last[0] + last[1];
            HIP_TRY(S->cloud.grow((size_t)total * 9));
            hipLaunchKernelGGL(k_cloud_emit, grid, dim3(256), 0, c->stream, S->keys, S->rows, N, S->vs, vs4, S->offsets, S->cloud);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
        S->cloud_n = (long long)total;
    }
    if (n) *n = S->cloud_n;
    if (S->cloud_n == 0 || max_n <= 0 || !rows9) return GSDF_OK;
    if (max_n < S->cloud_n) return cfail(GSDF_ERR_INVALID, "cloud buffer too small");
    HIP_TRY(hipMemcpy(rows9, S->cloud, (size_t)S->cloud_n * 9 * sizeof(float), hipMemcpyDeviceToHost));
    return GSDF_OK;
}

/* ---- extractMesh: HrLayeredMarchingCubes::computeIsoSurface (mesh/HrLayeredMarchingCubes.cpp:359-822) over the snapshot -------- */

#define GSDF_HR_KEY_BITS 20          /* bits per fine coordinate of the sweep key: 3 x 20 + 3 for the triangle number */

/* bounding box over ALL snapshot keys (:374-381): box[0..2] = minimum (preset to INT_MAX), box[3..5] = maximum (INT_MIN) */
__global__ __launch_bounds__(256) void k_hr_bbox(const unsigned long long* __restrict__ keys, size_t n, int* box) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    int m[6] = { INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN };
    for (; i < n; i += stride) {
        int p[3];
        gsdf_key_unpack(keys[i], &p[0], &p[1], &p[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) { m[a] = p[a] < m[a] ? p[a] : m[a]; m[3 + a] = p[a] > m[3 + a] ? p[a] : m[3 + a]; }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        int v = m[a];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(v, o); v = (a < 3 ? other < v : other > v) ? other : v; }
        if ((threadIdx.x & 63) == 0) { if (a < 3) atomicMin(&box[a], v); else atomicMax(&box[a], v); }
    }
}

/* corner c of a cube -> dx | dy << 1 | dz << 2, the numbering of computeLutIndex (:680-687) -- k_mesh's CORNER table:
 * (1,1,0) (1,0,0) (0,0,0) (0,1,0), then the same with dz = 1 */
__device__ __forceinline__ int hr_corner_bits(int c) { return ((0x2013 >> (4 * (c & 3))) & 3) | ((c >> 2) << 2); }
/* setVoxel :666-668 and getColor :771: static_cast<unsigned char>(float); a NaN (a voxel no keyframe counted) is undefined
 * behaviour in the reference and 0 here */
__device__ __forceinline__ unsigned int hr_byte(float v) { return isnan(v) ? 0u : ((unsigned int)(int)v & 0xffu); }

struct hr_mesh_args {
    const unsigned long long* keys;   /* the snapshot: packed keys in (z, y, x) order ... */
    const float* rows;                /* ... and their GSDF_COLOR_ROW floats */
    long long n;
    int mn[3], mx[3];                 /* bounding box of the keys */
    float vs, iso;
    const signed char* tri_table;
    float* tris;                      /* 9 floats per triangle */
    uint32_t* cols;                   /* 3 words per triangle: r | g << 8 | b << 16 per vertex */
    unsigned long long* skeys;        /* sweep key per triangle */
    unsigned long long* counter;
    long long max_tris;
};

/* 8 lanes per Hr voxel as in k_color: lane (i & 7) anchors the fine cube whose (0,0,0) corner is sub-voxel i, i.e. fine cell
 * 2 (X - min) + bit per axis (copyCube :638-653).  The cube's other corners lie in this voxel and in up to 7 coarse neighbours
 * (+x, +y, +z): lane j of the group looks for neighbour (j & 1, j >> 1 & 1, j >> 2) by binary search in the sorted keys -- all of
 * them sort after the voxel itself -- and leaves its row index in LDS for the group.  A missing neighbour is zeroWeights
 * (:611-628).  The sweep (:410-417) stops at dim - 2 = 2 extent - 2 per axis: no cube is anchored in a voxel of the box's maximal
 * coarse layer.  Triangles are appended with the sweep key (fine z, y, x, triangle number); the host sorts them. */
__global__ __launch_bounds__(256) void k_hr_mesh(hr_mesh_args a) {
    __shared__ int s_nb[256];                                                  /* per group: row index of neighbour j, -1 = missing */
    __shared__ int s_row[8][256];                                              /* per lane: row index of cube corner c ... */
    __shared__ float s_d[8][256];                                              /* ... and its distance */
    const int tid = threadIdx.x, sub = tid & 7, g0 = tid & ~7;
    const long long item = ((long long)blockIdx.x * 256 + tid) >> 3;
    const bool live = item < a.n;
    int x = 0, y = 0, z = 0, nb = -1;
    if (live) {
        gsdf_key_unpack(a.keys[item], &x, &y, &z);
        const int nx = x + (sub & 1), ny = y + ((sub >> 1) & 1), nz = z + (sub >> 2);
        if (sub == 0) nb = (int)item;
        else if (gsdf_key_in_range(nx, ny, nz)) {
            const unsigned long long want = gsdf_key_pack(nx, ny, nz);
            long long lo = item + 1, hi = a.n;
            while (lo < hi) {
                const long long mid = lo + ((hi - lo) >> 1);
                if (a.keys[mid] < want) lo = mid + 1; else hi = mid;
            }
            if (lo < a.n && a.keys[lo] == want) nb = (int)lo;
        }
    }
    s_nb[tid] = nb;
    __syncthreads();
    if (!live || x >= a.mx[0] || y >= a.mx[1] || z >= a.mx[2]) return;         /* the sweep's dim - 2 bounds (:410-417) */
    /* computeLutIndex :675-720 */
    bool ok = true;
    int idx = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int cb = hr_corner_bits(c);
        const int r = s_nb[g0 + (sub & cb)];                                   /* the coarse voxel steps where bit and offset are both 1 */
        float w = 0.f, d = 0.f;
        if (r >= 0) { const float* row = a.rows + (size_t)r * GSDF_COLOR_ROW; w = row[1]; d = row[5 + (sub ^ cb)]; }
        if (w == 0.0f) ok = false;
        if (d > a.iso) idx |= 1 << c;
        s_row[c][tid] = r;
        s_d[c][tid] = d;
    }
    if (!ok || idx == 0 || idx == 255) return;
    const int f0 = 2 * (x - a.mn[0]) + (sub & 1), f1 = 2 * (y - a.mn[1]) + ((sub >> 1) & 1), f2 = 2 * (z - a.mn[2]) + (sub >> 2);
    const float o0 = -(float)a.mn[0] * a.vs, o1 = -(float)a.mn[1] * a.vs, o2 = -(float)a.mn[2] * a.vs;     /* origin_ :384 */
    const signed char* t = a.tri_table + 16 * idx;
    for (int k = 0; k < 15 && t[k] >= 0; k += 3) {
        gsdf_v3 p[3];
        uint32_t col[3];
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            /* edge e -> its corners in getVertex order (:422-576): k_mesh's EDGE table */
            const int e = t[k + v];
            const int ca = e < 8 ? e : e - 8, cb = e < 8 ? (e & 4) | ((e + 1) & 3) : e - 4;
            /* voxelToWorld :817-821: 0.5f * ((float)i * vs) - origin */
            const int ba = hr_corner_bits(ca), bb = hr_corner_bits(cb);
            const gsdf_v3 wa = { 0.5f * ((float)(f0 + (ba & 1)) * a.vs) - o0, 0.5f * ((float)(f1 + ((ba >> 1) & 1)) * a.vs) - o1,
                                 0.5f * ((float)(f2 + (ba >> 2)) * a.vs) - o2 };
            const gsdf_v3 wb = { 0.5f * ((float)(f0 + (bb & 1)) * a.vs) - o0, 0.5f * ((float)(f1 + ((bb >> 1) & 1)) * a.vs) - o1,
                                 0.5f * ((float)(f2 + (bb >> 2)) * a.vs) - o2 };
            p[v] = mesh_interpolate(s_d[ca][tid], s_d[cb][tid], wa, wb, a.iso);
            /* getColor :756-773 with the endpoints in the order of ITS calls: reversed for edges 2, 3, 6, 7 (:458, :471, :510,
             * :523).  Red, green and blue are read at the cell's own index (the reference reads green at idx + 1 and blue at
             * idx + 2, other cells of its layer window: not a function of the map). */
            const bool rev = e < 8 && (e & 2);
            const int c1 = rev ? cb : ca, c2 = rev ? ca : cb;
            const float* r1 = a.rows + (size_t)s_row[c1][tid] * GSDF_COLOR_ROW + 13 + (sub ^ hr_corner_bits(c1));
            const float* r2 = a.rows + (size_t)s_row[c2][tid] * GSDF_COLOR_ROW + 13 + (sub ^ hr_corner_bits(c2));
            const gsdf_v3 q1 = { (float)hr_byte(r1[0] * 255.f) / 255.f, (float)hr_byte(r1[8] * 255.f) / 255.f, (float)hr_byte(r1[16] * 255.f) / 255.f };
            const gsdf_v3 q2 = { (float)hr_byte(r2[0] * 255.f) / 255.f, (float)hr_byte(r2[8] * 255.f) / 255.f, (float)hr_byte(r2[16] * 255.f) / 255.f };
            const gsdf_v3 cv = mesh_interpolate(s_d[c1][tid], s_d[c2][tid], q1, q2, a.iso);
            col[v] = hr_byte(cv.x * 255.f) | (hr_byte(cv.y * 255.f) << 8) | (hr_byte(cv.z * 255.f) << 16);
        }
        auto same = [](const gsdf_v3& u, const gsdf_v3& w) { return u.x == w.x && u.y == w.y && u.z == w.z; };
        if (same(p[0], p[1]) || same(p[0], p[2]) || same(p[1], p[2])) continue;          /* computeTriangles :789 */
        const unsigned long long o = atomicAdd(a.counter, 1ull);
        if ((long long)o >= a.max_tris) continue;
        float* out = a.tris + 9 * o;
#pragma unroll
        for (int v = 0; v < 3; ++v) { out[3 * v] = p[v].x; out[3 * v + 1] = p[v].y; out[3 * v + 2] = p[v].z; a.cols[3 * o + v] = col[v]; }
        a.skeys[o] = ((((unsigned long long)(uint32_t)f2 << (2 * GSDF_HR_KEY_BITS)) | ((unsigned long long)(uint32_t)f1 << GSDF_HR_KEY_BITS) |
                       (unsigned long long)(uint32_t)f0) << 3) | (unsigned long long)(k / 3);
    }
}

/* out[9 t + 3 v + ch] = byte ch of cols[3 order[t] + v]: one lane per byte */
__global__ __launch_bounds__(256) void k_hr_gather_cols(const uint32_t* __restrict__ cols, const uint32_t* __restrict__ order,
                                                         uint8_t* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * 9) return;
    const size_t t = i / 9, k = i - t * 9;
    out[i] = (uint8_t)(cols[(size_t)order[t] * 3 + k / 3] >> (8 * (k % 3)));
}

int gsdf_color_mesh(gsdf_ctx* c, float iso, float* triangles_out, uint8_t* colors_out, int64_t max_tris, int64_t* n_tris) {
    if (!c) return cfail(GSDF_ERR_INVALID, "null context");
    if (!c->color.valid) return cfail(GSDF_ERR_INVALID, "gsdf_color_compute was not called (or the map was reset)");
    if (!n_tris || (max_tris > 0 && !triangles_out)) return cfail(GSDF_ERR_INVALID, "null argument");
    const gsdf_color_state* S = &c->color;
    *n_tris = 0;
    if (S->n == 0) return GSDF_OK;
    if (S->n > (long long)INT_MAX) return cfail(GSDF_ERR_INVALID, "gsdf_color_mesh: more than 2^31 - 1 Hr voxels");
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)S->n;
    const long long cap = max_tris > 0 ? (long long)max_tris : 0;
    gsdf_dev<int> d_box;
    HIP_TRY(d_box.alloc(6));
    int box[6] = { INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN };
    HIP_TRY(hipMemcpyAsync(d_box, box, sizeof(box), hipMemcpyHostToDevice, c->stream));
    /* few workgroups: every wave ends in 6 atomics on the same words (1024 workgroups: 220 us on 2 x 10^5 keys) */
    hipLaunchKernelGGL(k_hr_bbox, dim3((unsigned int)std::min<size_t>((N + 255) / 256, 64)), dim3(256), 0, c->stream, S->keys.get(), N, d_box.get());
    HIP_TRY(hipMemcpyAsync(box, d_box, sizeof(box), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int a = 0; a < 3; ++a)                                                 /* fine cells 0 .. 2 extent - 1 must fit the sweep key */
        if (2ll * ((long long)box[3 + a] - box[a] + 1) > (1ll << GSDF_HR_KEY_BITS))
            return cfail(GSDF_ERR_INVALID, "gsdf_color_mesh: the snapshot's bounding box spans more than 2^19 voxels on an axis (the sweep key holds 20 bits per fine coordinate)");
    gsdf_dev<signed char> d_tab;
    gsdf_dev<float> d_tris;
    gsdf_dev<uint32_t> d_cols;
    gsdf_dev<unsigned long long> d_keys;
    HIP_TRY(d_tab.alloc(256 * 16));
    if (cap) HIP_TRY(d_tris.alloc((size_t)cap * 9));
    if (cap) HIP_TRY(d_cols.alloc((size_t)cap * 3));
    if (cap) HIP_TRY(d_keys.alloc((size_t)cap));
    HIP_TRY(hipMemcpyAsync(d_tab, GSDF_MC_TRI_TABLE, 256 * 16, hipMemcpyHostToDevice, c->stream));   /* the Hr triTable (:96-352) is the classic one */
    hr_mesh_args a;
    a.keys = S->keys; a.rows = S->rows; a.n = S->n;
    for (int k = 0; k < 3; ++k) { a.mn[k] = box[k]; a.mx[k] = box[3 + k]; }
    a.vs = S->vs; a.iso = iso; a.tri_table = d_tab;
    a.tris = d_tris; a.cols = d_cols; a.skeys = d_keys; a.counter = c->counter; a.max_tris = cap;
    unsigned long long n = 0;
    HIP_TRY(gsdf_counted(c, [&] { hipLaunchKernelGGL(k_hr_mesh, dim3((unsigned int)((8 * N + 255) / 256)), dim3(256), 0, c->stream, a); }, &n));
    /* the reference's order (fine z-y-x sweep, triangles of a cube in table order) = ascending sweep key, as gsdf_extract_mesh */
    if (n && n <= (unsigned long long)cap) {
        const size_t got = (size_t)n;
        gsdf_key_order ord;
        gsdf_dev<float> d_sorted;
        gsdf_dev<uint8_t> d_bytes;
        HIP_TRY(ord.alloc(got));
        HIP_TRY(d_sorted.alloc(got * 9));
        HIP_TRY(ord.run(c, d_keys, got));
        gsdf_launch_gather_tris(c->stream, d_tris, ord.order, d_sorted, got);
        HIP_TRY(hipMemcpyAsync(triangles_out, d_sorted, got * 9 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        if (colors_out) {
            HIP_TRY(d_bytes.alloc(got * 9));
            hipLaunchKernelGGL(k_hr_gather_cols, dim3((unsigned int)((got * 9 + 255) / 256)), dim3(256), 0, c->stream, d_cols.get(), ord.order.get(),
                               d_bytes.get(), got);
            HIP_TRY(hipMemcpyAsync(colors_out, d_bytes, got * 9, hipMemcpyDeviceToHost, c->stream));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *n_tris = (int64_t)n;                                                      /* total found, also when it exceeds max_tris */
    if (n > (unsigned long long)cap && cap) return cfail(GSDF_ERR_INVALID, "gsdf_color_mesh: max_tris too small (n_tris holds the need)");
    return GSDF_OK;
}
