/*
 * gsdf_select.hip -- removing voxels from the map (gfx950): the selection, its consumers, gsdf_erase_selected, gsdf_compact.
 * The definitions are in include/gsdf.h.
 *
 * The selection S is one 64-bit word per block entry of the present table (bit = gsdf_block_local); a second bitmap of the
 * same size behind it receives the predicate set P of the running call, and four device words behind that the counts.
 *
 *   k_sel_box       one thread per block entry: the 64 bits follow from the block key, no voxel record is read
 *   k_sel_weight    one wave per block entry, one lane per record: a ballot is the word
 *   k_sel_points    one wave per point, lanes over the blocks of the point's candidate cube: the exact predicate on the block's
 *                   64 centres, then ONE lookup per block that holds a member and one integer atomic OR
 *   k_sel_combine   one wave per block entry: S := op(S, P), and the members with w > 0 / their blocks counted
 *   k_sel_export    the members with w > 0 appended through a counter (packed keys for the host, int32 triples for the device)
 *   k_sel_erase     one wave per block entry: member records and their vis_ words zeroed; block keys stay
 *   k_sel_live      blocks that hold a voxel, for gsdf_compact's room rule (the rebuild itself is gsdf_merge.hip's)
 *
 * Every kernel is a sweep over a table that is cache-resident at the project's map sizes or a gather around given points;
 * nothing here is MFMA-shaped.  No floating-point atomics, no spin waits, every loop bounded.  Wave = 64 lanes.
 */
#include "gsdf_ctx.h"
#include "gsdf_math.h"
#include "gsdf_sweep.h"

#include <cmath>
#include <cstring>
#include <numeric>

namespace {

enum { SW_VOXELS = 0, SW_BLOCKS, SW_AUX, SW_COUNT_ = 4 };       /* the device words behind the two bitmaps */
enum { OP_INVERT = 4, OP_KEEP = 5 };                             /* beside GSDF_SEL_*: S := ~S on existing blocks / count only */

struct sel_f3 { float v[3]; };
struct sel_pose { float R[9]; float t[3]; int on; };

/* the three 4-bit masks of a block's voxel indices per axis -> its 64-bit word, bit = x | y << 2 | z << 4 */
__device__ __forceinline__ unsigned long long sel_word_of_masks(uint32_t mx, uint32_t my, uint32_t mz) {
    uint32_t xy = 0u;
#pragma unroll
    for (int y = 0; y < 4; ++y) if ((my >> y) & 1u) xy |= mx << (4 * y);
    unsigned long long w = 0ull;
#pragma unroll
    for (int z = 0; z < 4; ++z) if ((mz >> z) & 1u) w |= (unsigned long long)xy << (16 * z);
    return w;
}

/* voxel index of in-block coordinate a (0..3) of the biased block coordinate B (a field of a block key) */
__device__ __forceinline__ int sel_index(uint32_t B, int a) { return (int)((B << 2) | (uint32_t)a) - GSDF_KEY_OFF; }

__global__ __launch_bounds__(256) void k_sel_box(const unsigned long long* __restrict__ bkeys, size_t n_blocks, float vs, sel_f3 lo, sel_f3 hi,
                                                 unsigned long long* __restrict__ P) {
    const size_t b = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (b >= n_blocks) return;
    const unsigned long long bk = bkeys[b];
    if (bk == GSDF_KEY_EMPTY) { P[b] = 0ull; return; }
    const uint32_t B[3] = { (uint32_t)(bk & 0x7FFFFull), (uint32_t)((bk >> 19) & 0x7FFFFull), (uint32_t)((bk >> 38) & 0x7FFFFull) };
    uint32_t m[3] = { 0u, 0u, 0u };
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float c = vs * (float)sel_index(B[a], e);                 /* the voxel centre */
            if (lo.v[a] <= c && c <= hi.v[a]) m[a] |= 1u << e;
        }
    P[b] = sel_word_of_masks(m[0], m[1], m[2]);
}

__global__ __launch_bounds__(256) void k_sel_weight(gsdf_table tab, size_t n_blocks, float w_min, float w_max, unsigned long long* __restrict__ P) {
    const size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long bk = tab.bkeys[b];
    bool in = false;
    if (bk != GSDF_KEY_EMPTY) {
        const float w = tab.vox[b * GSDF_BLOCK_VOX + lane].w;
        in = w_min <= w && w < w_max;
    }
    const unsigned long long word = __ballot(in);
    if (lane == 0) P[b] = word;
}

/* One wave per point (grid-stride).  P was zeroed by the caller.  The candidate cube is taken per axis in double, one index
 * wider on each side than exact arithmetic needs; its blocks are dealt to the lanes, 64 at a time.  A lane evaluates the exact
 * float predicate on the 64 voxel centres of its block (whole blocks: more candidates than the cube, which the predicate
 * rejects) and only a block that holds a member is looked up.  At most 10^3 blocks per point (radius <= 16 voxels). */
__global__ __launch_bounds__(256) void k_sel_points(gsdf_table tab, float vs, const float* __restrict__ pts, long long n, sel_pose pose,
                                                    float radius, unsigned long long* P) {
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 4;
    const float r2 = radius * radius;
    const gsdf_v3 t = { pose.t[0], pose.t[1], pose.t[2] };
    for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < n; i += stride) {          /* uniform in the wave */
        const gsdf_v3 x = { pts[3 * i], pts[3 * i + 1], pts[3 * i + 2] };
        const gsdf_v3 p = pose.on ? gsdf_rigid_apply(pose.R, t, x) : x;
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
        const float pc[3] = { p.x, p.y, p.z };
        int blo[3], bn[3];
        bool none = false;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double l = ((double)pc[a] - (double)radius) / (double)vs, h = ((double)pc[a] + (double)radius) / (double)vs;
            if (!(l > -2097152.0 && h < 2097152.0)) { none = true; continue; }     /* beyond 2^21 voxels: nothing packable near it */
            const int lo = (int)ceil(l) - 1, hi = (int)floor(h) + 1;
            /* biased block coordinates; those outside [0, 2^19) lie beyond the packable range and are left out before any packing */
            int b0 = (lo + GSDF_KEY_OFF) >> 2, b1 = (hi + GSDF_KEY_OFF) >> 2;
            b0 = b0 < 0 ? 0 : b0;
            b1 = b1 > 0x7FFFF ? 0x7FFFF : b1;
            blo[a] = b0; bn[a] = b1 - b0 + 1;
            if (bn[a] <= 0) none = true;
        }
        if (none) continue;
        const int total = bn[0] * bn[1] * bn[2];                           /* <= 10^3 */
        for (int base = 0; base < total; base += 64) {
            const int idx = base + lane;
            unsigned long long word = 0ull, bk = 0ull;
            if (idx < total) {
                const uint32_t B[3] = { (uint32_t)(blo[0] + idx % bn[0]), (uint32_t)(blo[1] + (idx / bn[0]) % bn[1]),
                                        (uint32_t)(blo[2] + idx / (bn[0] * bn[1])) };
                float dd[3][4];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float c = vs * (float)sel_index(B[a], e);
                        const float d = c - pc[a];
                        dd[a][e] = d * d;
                    }
#pragma unroll
                for (int l = 0; l < 64; ++l)
                    if (dd[0][l & 3] + (dd[1][(l >> 2) & 3] + dd[2][l >> 4]) <= r2) word |= 1ull << l;
                bk = (unsigned long long)B[0] | ((unsigned long long)B[1] << 19) | ((unsigned long long)B[2] << 38);
            }
            /* the lookup runs with the whole wave converged (it votes across the wave) */
            const uint32_t pend = word ? 1u : 0u;
            const unsigned long long bks[1] = { bk };
            uint32_t hs[1] = { gsdf_hash(bk) & tab.block_mask };
            unsigned long long ks[1] = { pend ? tab.bkeys[hs[0]] : GSDF_KEY_EMPTY };
            int bs[1];
            gsdf_block_lookup_n<1, false>(tab, bks, hs, ks, pend, bs);
            if (pend && bs[0] >= 0) atomicOr(&P[bs[0]], word);
        }
    }
}

__device__ __forceinline__ unsigned long long sel_apply(int op, unsigned long long s, unsigned long long p) {
    switch (op) {
    case GSDF_SEL_REPLACE:   return p;
    case GSDF_SEL_ADD:       return s | p;
    case GSDF_SEL_INTERSECT: return s & p;
    case GSDF_SEL_SUBTRACT:  return s & ~p;
    case OP_INVERT:          return ~s;
    default:                 return s;
    }
}

/* S := op(S, P) (s_none: S counts as empty, whatever the buffer holds); entries without a block get 0.  words[SW_VOXELS] +=
 * members with w > 0, words[SW_BLOCKS] += blocks that hold one. */
__global__ __launch_bounds__(256) void k_sel_combine(gsdf_table tab, size_t n_blocks, unsigned long long* S, const unsigned long long* P, int op,
                                                     int s_none, unsigned long long* words) {
    const size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    const unsigned long long bk = tab.bkeys[b];
    unsigned long long s = s_none ? 0ull : S[b];
    if (op != OP_KEEP) {
        const unsigned long long p = (op == OP_INVERT) ? 0ull : P[b];
        s = bk == GSDF_KEY_EMPTY ? 0ull : sel_apply(op, s, p);
        if (lane == 0) S[b] = s;
    }
    bool live = false;
    if (bk != GSDF_KEY_EMPTY && ((s >> lane) & 1ull)) live = tab.vox[b * GSDF_BLOCK_VOX + lane].w > 0.f;
    const unsigned long long m = __ballot(live);
    if (lane == 0 && m) {
        atomicAdd(&words[SW_VOXELS], (unsigned long long)__popcll(m));
        atomicAdd(&words[SW_BLOCKS], 1ull);
    }
}

/* the members with w > 0, appended through `counter`: packed keys (keys64) or int32 triples (keys32); raw sums or (dist, g, w) */
__global__ __launch_bounds__(256) void k_sel_export(gsdf_table tab, size_t n_slots, const unsigned long long* __restrict__ S,
                                                    unsigned long long* keys64, int32_t* keys32, float* payload_out,
                                                    unsigned long long* counter, long long max_n, int raw) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_slots; i += stride) {
        const size_t b = i / GSDF_BLOCK_VOX;
        const uint32_t local = (uint32_t)(i % GSDF_BLOCK_VOX);
        const unsigned long long bk = tab.bkeys[b];
        if (bk == GSDF_KEY_EMPTY || !((S[b] >> local) & 1ull)) continue;
        const gsdf_payload sl = tab.vox[i];
        if (!(sl.w > 0.f)) continue;
        const unsigned long long o = atomicAdd(counter, 1ull);
        if ((long long)o >= max_n) continue;
        const unsigned long long key = gsdf_voxel_key(bk, local);
        if (keys64) keys64[o] = key;
        if (keys32) {
            int x, y, z;
            gsdf_key_unpack(key, &x, &y, &z);
            keys32[3 * o] = x; keys32[3 * o + 1] = y; keys32[3 * o + 2] = z;
        }
        if (payload_out) {
            float* p = payload_out + 5 * o;
            p[0] = raw ? sl.s : sl.s / sl.w; p[1] = sl.gx; p[2] = sl.gy; p[3] = sl.gz; p[4] = sl.w;
        }
    }
}

/* member records := 0 (32 bytes, and the vis_ words): what the table clear leaves.  Block keys stay.  words[SW_VOXELS] += members
 * that existed, words[SW_BLOCKS] += blocks that lost a voxel and hold none afterwards. */
__global__ __launch_bounds__(256) void k_sel_erase(gsdf_table tab, size_t n_blocks, const unsigned long long* __restrict__ S, uint32_t* vis, int vw,
                                                   unsigned long long* words) {
    const size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    if (tab.bkeys[b] == GSDF_KEY_EMPTY) return;
    const unsigned long long s = S[b];
    if (!s) return;
    const size_t slot = b * GSDF_BLOCK_VOX + lane;
    const bool member = (s >> lane) & 1ull;
    const bool exists = tab.vox[slot].w > 0.f;
    const unsigned long long had = __ballot(exists), gone = __ballot(exists && member);
    if (member) {
        uint4* p = reinterpret_cast<uint4*>(tab.vox + slot);
        p[0] = make_uint4(0u, 0u, 0u, 0u); p[1] = make_uint4(0u, 0u, 0u, 0u);
        for (int w = 0; w < vw; ++w) vis[slot * vw + w] = 0u;
    }
    if (lane == 0 && gone) {
        atomicAdd(&words[SW_VOXELS], (unsigned long long)__popcll(gone));
        if (!(had & ~gone)) atomicAdd(&words[SW_BLOCKS], 1ull);
    }
}

/* blocks that hold a voxel with w > 0, added to *out */
__global__ __launch_bounds__(256) void k_sel_live(gsdf_table tab, size_t n_blocks, unsigned long long* out) {
    const size_t b = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    if (tab.bkeys[b] == GSDF_KEY_EMPTY) return;
    const unsigned long long m = __ballot(tab.vox[b * GSDF_BLOCK_VOX + lane].w > 0.f);
    if (lane == 0 && m) atomicAdd(out, 1ull);
}

/* ---- host side ---------------------------------------------------------------------------------------------------------- */
size_t sel_blocks(const gsdf_ctx* c) { return c->n_slots / GSDF_BLOCK_VOX; }
unsigned long long* sel_P(const gsdf_ctx* c) { return c->sel.get() + sel_blocks(c); }
unsigned long long* sel_words(const gsdf_ctx* c) { return c->sel.get() + 2 * sel_blocks(c); }
unsigned int wave_grid(size_t n_blocks) { return (unsigned int)((n_blocks + 3) / 4); }

int sel_lost(const char* who) {
    return gsdf_fail(GSDF_ERR_INVALID, std::string(who) + ": the selection is lost -- the table was rehashed since it was made (gsdf_grow, "
                     "auto-grow or a merge that grew the map) and slots moved; select again with GSDF_SEL_REPLACE or call gsdf_select_clear");
}

/* what every entry starts with: device, the waiting fusion */
int sel_enter(gsdf_ctx* c) {
    HIP_TRY(hipSetDevice(c->device));
    return gsdf_flush_pending(c);
}

/* checks of a select call before anything is computed; afterwards the bitmaps exist */
int sel_begin(gsdf_ctx* c, int op, const char* who) {
    if (op < GSDF_SEL_REPLACE || op > GSDF_SEL_SUBTRACT) return gsdf_fail(GSDF_ERR_INVALID, std::string(who) + ": op must be one of GSDF_SEL_REPLACE / ADD / INTERSECT / SUBTRACT");
    if (c->sel_state == GSDF_SEL_LOST && op != GSDF_SEL_REPLACE) return sel_lost(who);
    if (int rc = sel_enter(c)) return rc;
    /* a rebuild of the table released the bitmaps (gsdf_rebuild_impl), so one that exists fits the present table */
    if (!c->sel) HIP_TRY(c->sel.alloc(2 * sel_blocks(c) + SW_COUNT_));
    return GSDF_OK;
}

/* S := op(S, P) or a plain count (OP_KEEP); *n_voxels / *n_blocks = the members with w > 0 and their blocks afterwards */
int sel_combine(gsdf_ctx* c, int op, int64_t* n_voxels, int64_t* n_blocks) {
    const size_t nb = sel_blocks(c);
    unsigned long long h[2] = { 0, 0 };
    HIP_TRY(hipMemsetAsync(sel_words(c), 0, SW_COUNT_ * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_sel_combine, dim3(wave_grid(nb)), dim3(256), 0, c->stream, c->tab, nb, c->sel.get(), sel_P(c), op,
                       c->sel_state == GSDF_SEL_VALID ? 0 : 1, sel_words(c));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, sel_words(c), sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (op != OP_KEEP) c->sel_state = GSDF_SEL_VALID;
    if (n_voxels) *n_voxels = (int64_t)h[SW_VOXELS];
    if (n_blocks) *n_blocks = (int64_t)h[SW_BLOCKS];
    return GSDF_OK;
}

int select_points_impl(gsdf_ctx* c, const float* pts_host, const float* pts_dev, int64_t n_pts, const float* pose7, float radius, int op,
                       int64_t* n) {
    const char* who = "gsdf_select_points";
    if (n) *n = 0;
    if (!c) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_points: null context");
    if (n_pts < 0 || (n_pts > 0 && !pts_host && !pts_dev)) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_points: negative n_pts or null points");
    if (!std::isfinite(radius) || radius < 0.f || radius > 16.f * c->voxel_size)
        return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_points: the radius must be finite, >= 0 and at most 16 voxel sizes");
    if (pose7 && !gsdf_pose7_ok(pose7)) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_points: the pose must be finite with | |q|^2 - 1 | <= 1e-4");
    if (int rc = sel_begin(c, op, who)) return rc;
    gsdf_dev<float> staged;
    if (n_pts > 0 && !pts_dev) {
        HIP_TRY(staged.alloc((size_t)n_pts * 3));
        HIP_TRY(hipMemcpyAsync(staged, pts_host, (size_t)n_pts * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        pts_dev = staged;
    }
    sel_pose pose;
    std::memset(&pose, 0, sizeof(pose));
    if (pose7) {
        gsdf_quat_to_R(pose7 + 3, pose.R);                     /* as it comes, not renormalised: the registration's R */
        std::memcpy(pose.t, pose7, sizeof(pose.t));
        pose.on = 1;
    }
    HIP_TRY(hipMemsetAsync(sel_P(c), 0, sel_blocks(c) * sizeof(unsigned long long), c->stream));
    if (n_pts > 0) {
        const long long g = (n_pts + 3) / 4;
        hipLaunchKernelGGL(k_sel_points, dim3((unsigned int)(g > 65536 ? 65536 : g)), dim3(256), 0, c->stream, c->tab, c->voxel_size, pts_dev,
                           (long long)n_pts, pose, radius, sel_P(c));
        HIP_TRY(hipGetLastError());
    }
    return sel_combine(c, op, n, nullptr);                     /* synchronises: `staged` may go */
}

/* a consumer's look at the state: *none = nothing to do */
int sel_consume(gsdf_ctx* c, const char* who, bool* none) {
    if (c->sel_state == GSDF_SEL_LOST) return sel_lost(who);
    if (int rc = sel_enter(c)) return rc;
    *none = c->sel_state == GSDF_SEL_NONE || !c->sel;
    return GSDF_OK;
}

} // namespace

extern "C" {

int gsdf_select_box(gsdf_ctx* c, const float lo[3], const float hi[3], int op, int64_t* n) {
    if (n) *n = 0;
    if (!c || !lo || !hi) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_box: null argument");
    sel_f3 l, h;
    for (int a = 0; a < 3; ++a) {
        if (std::isnan(lo[a]) || std::isnan(hi[a])) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_box: a bound is NaN");
        l.v[a] = lo[a]; h.v[a] = hi[a];
    }
    if (int rc = sel_begin(c, op, "gsdf_select_box")) return rc;
    const size_t nb = sel_blocks(c);
    hipLaunchKernelGGL(k_sel_box, dim3((unsigned int)((nb + 255) / 256)), dim3(256), 0, c->stream, c->tab.bkeys, nb, c->voxel_size, l, h, sel_P(c));
    HIP_TRY(hipGetLastError());
    return sel_combine(c, op, n, nullptr);
}

int gsdf_select_weight(gsdf_ctx* c, float w_min, float w_max, int op, int64_t* n) {
    if (n) *n = 0;
    if (!c) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_weight: null context");
    if (std::isnan(w_min) || std::isnan(w_max)) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_weight: a bound is NaN");
    if (int rc = sel_begin(c, op, "gsdf_select_weight")) return rc;
    const size_t nb = sel_blocks(c);
    hipLaunchKernelGGL(k_sel_weight, dim3(wave_grid(nb)), dim3(256), 0, c->stream, c->tab, nb, w_min, w_max, sel_P(c));
    HIP_TRY(hipGetLastError());
    return sel_combine(c, op, n, nullptr);
}

int gsdf_select_points(gsdf_ctx* c, const float* pts_host, int64_t n_pts, const float pose7[7], float radius, int op, int64_t* n) {
    return select_points_impl(c, pts_host, nullptr, n_pts, pose7, radius, op, n);
}

int gsdf_select_points_dev(gsdf_ctx* c, const float* pts_dev, int64_t n_pts, const float pose7[7], float radius, int op, int64_t* n) {
    return select_points_impl(c, nullptr, pts_dev, n_pts, pose7, radius, op, n);
}

int gsdf_select_invert(gsdf_ctx* c, int64_t* n) {
    if (n) *n = 0;
    if (!c) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_invert: null context");
    if (c->sel_state == GSDF_SEL_LOST) return sel_lost("gsdf_select_invert");
    if (int rc = sel_begin(c, GSDF_SEL_REPLACE, "gsdf_select_invert")) return rc;
    return sel_combine(c, OP_INVERT, n, nullptr);
}

int gsdf_select_clear(gsdf_ctx* c) {
    if (!c) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_clear: null context");
    if (int rc = sel_enter(c)) return rc;
    c->sel_state = GSDF_SEL_NONE;
    return GSDF_OK;
}

int gsdf_select_count(gsdf_ctx* c, int64_t* n_voxels, int64_t* n_blocks) {
    if (n_voxels) *n_voxels = 0;
    if (n_blocks) *n_blocks = 0;
    if (!c) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_count: null context");
    bool none = false;
    if (int rc = sel_consume(c, "gsdf_select_count", &none)) return rc;
    if (none) return GSDF_OK;
    return sel_combine(c, OP_KEEP, n_voxels, n_blocks);
}

int gsdf_select_export(gsdf_ctx* c, int32_t* keys, float* payload, int64_t max_n, int64_t* n_out, int raw_sums) {
    if (n_out) *n_out = 0;
    if (!c || !n_out || max_n < 0) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_export: bad argument");
    bool none = false;
    if (int rc = sel_consume(c, "gsdf_select_export", &none)) return rc;
    if (none) return GSDF_OK;
    int64_t cnt = 0;
    if (int rc = sel_combine(c, OP_KEEP, &cnt, nullptr)) return rc;
    *n_out = cnt;
    if (cnt == 0 || max_n == 0 || (!keys && !payload)) return GSDF_OK;                /* nothing to write; the sizing call */
    if (cnt > max_n) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_export: max_n too small (*n holds the need)");
    const size_t n = (size_t)cnt;
    gsdf_dev<unsigned long long> dkeys;
    gsdf_dev<float> dpay;
    HIP_TRY(dkeys.alloc(n));
    HIP_TRY(dpay.alloc(n * 5));
    HIP_TRY(gsdf_counter_zero(c));
    hipLaunchKernelGGL(k_sel_export, dim3(2048), dim3(256), 0, c->stream, c->tab, c->n_slots, c->sel.get(), dkeys.get(), (int32_t*)nullptr,
                       dpay.get(), c->counter.get(), (long long)n, raw_sums);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned long long> hk(n);
    std::vector<float> hp(n * 5);
    HIP_TRY(hipMemcpyAsync(hk.data(), dkeys, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hp.data(), dpay, n * 5 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return hk[a] < hk[b]; });      /* packed keys order like (z, y, x) */
    for (size_t i = 0; i < n; ++i) {
        const size_t j = order[i];
        if (keys) {
            int x, y, z;
            gsdf_key_unpack(hk[j], &x, &y, &z);
            keys[3 * i] = x; keys[3 * i + 1] = y; keys[3 * i + 2] = z;
        }
        if (payload) std::memcpy(payload + 5 * i, hp.data() + 5 * j, 5 * sizeof(float));
    }
    return GSDF_OK;
}

int gsdf_select_export_raw_dev(gsdf_ctx* c, int32_t* keys_dev, float* payload_raw_dev, int64_t max_n, int64_t* n_out) {
    if (n_out) *n_out = 0;
    if (!c || !n_out || max_n < 0) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_export_raw_dev: bad argument");
    bool none = false;
    if (int rc = sel_consume(c, "gsdf_select_export_raw_dev", &none)) return rc;
    if (none) return GSDF_OK;
    int64_t cnt = 0;
    if (int rc = sel_combine(c, OP_KEEP, &cnt, nullptr)) return rc;
    *n_out = cnt;
    if (cnt == 0 || max_n == 0 || !keys_dev || !payload_raw_dev) return GSDF_OK;       /* nothing to write; the sizing call */
    if (cnt > max_n) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_select_export_raw_dev: max_n too small (*n holds the need)");
    HIP_TRY(gsdf_counter_zero(c));
    hipLaunchKernelGGL(k_sel_export, dim3(2048), dim3(256), 0, c->stream, c->tab, c->n_slots, c->sel.get(), (unsigned long long*)nullptr, keys_dev,
                       payload_raw_dev, c->counter.get(), (long long)cnt, 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_erase_selected(gsdf_ctx* c, int64_t* n_voxels, int64_t* n_blocks_emptied) {
    if (n_voxels) *n_voxels = 0;
    if (n_blocks_emptied) *n_blocks_emptied = 0;
    if (!c) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_erase_selected: null context");
    bool none = false;
    if (int rc = sel_consume(c, "gsdf_erase_selected", &none)) return rc;
    if (none) { c->sel_state = GSDF_SEL_NONE; return GSDF_OK; }
    const size_t nb = sel_blocks(c);
    unsigned long long h[2] = { 0, 0 };
    HIP_TRY(hipMemsetAsync(sel_words(c), 0, SW_COUNT_ * sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_sel_erase, dim3(wave_grid(nb)), dim3(256), 0, c->stream, c->tab, nb, c->sel.get(), c->map.vis.get(),
                       c->map.vis ? c->vis_words : 0, sel_words(c));
    HIP_TRY(hipGetLastError());
    /* the map changed from here on, whatever the copies below return */
    c->sel_state = GSDF_SEL_NONE;
    c->ba.gate_list.reset();                                   /* PhotoBA's gate list and mean cache describe the old map (as gsdf_grow) */
    c->ba.mean.reset();
    c->ba_gate_fresh = false; c->ba_mean_valid = false;
    HIP_TRY(hipMemcpyAsync(h, sel_words(c), sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n_voxels) *n_voxels = (int64_t)h[SW_VOXELS];
    if (n_blocks_emptied) *n_blocks_emptied = (int64_t)h[SW_BLOCKS];
    return GSDF_OK;
}

int gsdf_compact(gsdf_ctx* c, int new_capacity_log2, int64_t* n_blocks_dropped) {
    if (n_blocks_dropped) *n_blocks_dropped = 0;
    if (!c) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_compact: null context");
    const int cap = new_capacity_log2 == 0 ? c->capacity_log2 : new_capacity_log2;
    if (cap < 10 || cap > 30) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_compact: new_capacity_log2 must be 0 (keep) or in [10, 30]");
    if (int rc = sel_enter(c)) return rc;
    const size_t nb = sel_blocks(c);
    unsigned long long live = 0;
    HIP_TRY(gsdf_counted(c, [&] { hipLaunchKernelGGL(k_sel_live, dim3(wave_grid(nb)), dim3(256), 0, c->stream, c->tab, nb, c->counter.get()); }, &live));
    const size_t entries = ((size_t)1 << cap) / GSDF_BLOCK_VOX;
    if ((size_t)live * 100u > entries * 45u)
        return gsdf_fail(GSDF_ERR_TABLE_FULL, "gsdf_compact: " + std::to_string(live) + " live blocks pass 45 % of the " + std::to_string(entries) +
                         " block entries of capacity_log2 " + std::to_string(cap) + "; the map is unchanged");
    long long dropped = 0;
    if (int rc = gsdf_rebuild_impl(c, cap, true, &dropped, "gsdf_compact")) return rc;
    c->sel_state = GSDF_SEL_NONE;
    if (n_blocks_dropped) *n_blocks_dropped = (int64_t)dropped;
    return GSDF_OK;
}

} // extern "C"
