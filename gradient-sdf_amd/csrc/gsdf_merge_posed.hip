/*
 * gsdf_merge_posed.hip -- gsdf_merge_from_posed: src resampled on dst's voxel grid under a rigid pose and added into dst (gfx950).
 * The definition is in include/gsdf.h; the enumeration and its radius in gsdf_posed.h.
 *
 *   k_posed_candidates   one thread per block entry of src: the dst blocks its receivers can lie in, as wide keys
 *   (sort + unique)      rocPRIM: every candidate block once, in key order
 *   k_posed_sample       one wave per candidate block, one lane per voxel: steps 1-6 of the definition into a dense staging row
 *                        (64 x 5 floats, the layout of gsdf_pack_blocks_dev), a flag per block, the counts
 *   (host)               blocks flagged = find-or-insert operations to come: room check, growth -- dst is untouched so far
 *   k_posed_add          one wave per candidate block, flagged ones stay: lane 0 finds or claims the block, 64 plain
 *                        read-modify-writes
 *
 * A candidate block appears once and a record has one lane, so a key gets at most one contribution and nothing is added with
 * atomics on floats; the order in which candidates were appended is removed by the sort.  The result is a function of
 * (dst, src, pose).  Both kernels over blocks are gathers over a table that is cache-resident at the project's map sizes;
 * nothing here is MFMA-shaped.  Wave = 64 lanes.
 */
#include "gsdf_ctx.h"
#include "gsdf_posed.h"
#include "gsdf_sample.h"
#include "gsdf_sweep.h"

#include <cmath>
#include <cstring>

namespace {

/* words of the call on the device */
enum { PW_UNIQUE = 0, PW_VOXELS, PW_BLOCKS, PW_RANGE, PW_DST_BLOCKS, PW_COUNT_ };

/* Counts (keys == nullptr) or appends the candidate blocks: a thread enumerates its block twice, first to reserve its run of the
 * list with ONE integer atomic, then to write it.  *range is raised when an image cannot be enumerated at all. */
__global__ __launch_bounds__(256) void k_posed_candidates(const unsigned long long* __restrict__ bkeys, size_t n_blocks, gsdf_posed_map m,
                                                          unsigned long long* __restrict__ keys, unsigned long long* counter,
                                                          long long max_n, unsigned long long* range) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_blocks; i += stride) {
        const unsigned long long bk = bkeys[i];
        if (bk == GSDF_KEY_EMPTY) continue;
        int X, Y, Z;
        gsdf_posed_block_of_key(bk, &X, &Y, &Z);
        const int n = gsdf_posed_blocks(m, X, Y, Z, [](int, int, int) {});
        if (n < 0) { atomicOr(range, 1ull); continue; }
        if (n == 0) continue;
        const unsigned long long base = atomicAdd(counter, (unsigned long long)n);
        if (!keys) continue;
        unsigned long long o = base;
        gsdf_posed_blocks(m, X, Y, Z, [&](int x, int y, int z) {
            if ((long long)o < max_n) keys[o] = gsdf_posed_wide_pack(x, y, z);
            ++o;
        });
    }
}

/* occupied entries of a key array, added to *out */
__global__ __launch_bounds__(256) void k_posed_count_blocks(const unsigned long long* __restrict__ bkeys, size_t n, unsigned long long* out) {
    unsigned int c = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) c += bkeys[i] != GSDF_KEY_EMPTY ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

/* Steps 1-6 of the definition for the 64 voxels of candidate block b.  stage[b][lane][5] = (w', s', g'), zeros where nothing is
 * received; flags[b] = some voxel of a packable block received; words: voxels that received, blocks flagged, a block beyond the
 * packable range would have received. */
__global__ __launch_bounds__(256) void k_posed_sample(gsdf_table src, float vs, float inv_vs, float T, gsdf_pose_arg pose,
                                                      const unsigned long long* __restrict__ cand, long long n,
                                                      float* __restrict__ stage, uint32_t* __restrict__ flags, unsigned long long* words) {
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n) return;
    const int lane = threadIdx.x & 63;
    int X, Y, Z;
    gsdf_posed_wide_unpack(cand[b], &X, &Y, &Z);
    const int i = 4 * X + (lane & 3), j = 4 * Y + ((lane >> 2) & 3), k = 4 * Z + (lane >> 4);
    const float Rt[9] = { pose.R[0], pose.R[3], pose.R[6], pose.R[1], pose.R[4], pose.R[7], pose.R[2], pose.R[5], pose.R[8] };
    const gsdf_v3 c = { vs * (float)i, vs * (float)j, vs * (float)k };                 /* 1: vox2float */
    const gsdf_v3 d = { c.x - pose.t[0], c.y - pose.t[1], c.z - pose.t[2] };           /* 2 */
    const gsdf_v3 q = gsdf_matvec(Rt, d);                                              /* 3 */
    float v[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
    bool got = false;
    if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z)) {                             /* 4: before any float -> int conversion */
        float w, phi;
        gsdf_v3 g;
        gsdf_grad_sample(src, vs, inv_vs, q, w, phi, g);                               /* 5: what gsdf_query returns at q */
        if (w != 0.f) {
            /* 6: the stored record of float2vox(q) (found and in range: w != 0) */
            const gsdf_payload* S = gsdf_find(src, gsdf_key_pack(gsdf_float2vox1(inv_vs, q.x), gsdf_float2vox1(inv_vs, q.y),
                                                                 gsdf_float2vox1(inv_vs, q.z)));
            const gsdf_v3 gr = gsdf_matvec(pose.R, gsdf_v3{ S->gx, S->gy, S->gz });
            v[0] = S->w;
            v[1] = S->w * gsdf_truncate(phi, T);
            v[2] = gr.x; v[3] = gr.y; v[4] = gr.z;
            got = true;
        }
    }
    const bool packable = gsdf_posed_block_in_range(X, Y, Z);
    float* o = stage + ((size_t)b * GSDF_BLOCK_VOX + lane) * 5;
#pragma unroll
    for (int e = 0; e < 5; ++e) o[e] = packable ? v[e] : 0.f;
    const unsigned long long mask = __ballot(got);
    if (lane == 0) {
        flags[b] = (packable && mask) ? 1u : 0u;
        if (mask) {
            if (packable) {
                atomicAdd(&words[PW_VOXELS], (unsigned long long)__popcll(mask));
                atomicAdd(&words[PW_BLOCKS], 1ull);
            } else {
                atomicOr(&words[PW_RANGE], 1ull);
            }
        }
    }
}

/* dst += stage for the flagged candidate blocks (step 7).  A block without a receiver is never inserted. */
__global__ __launch_bounds__(256) void k_posed_add(gsdf_table dst, const unsigned long long* __restrict__ cand, long long n,
                                                   const float* __restrict__ stage, const uint32_t* __restrict__ flags, gsdf_dev_state* st) {
    const long long b = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= n || !flags[b]) return;
    const int lane = threadIdx.x & 63;
    int X, Y, Z;
    gsdf_posed_wide_unpack(cand[b], &X, &Y, &Z);
    const unsigned long long bk = gsdf_posed_key_of_block(X, Y, Z);
    int nb = -1;
    if (lane == 0) {
        const uint32_t h = gsdf_hash(bk) & dst.block_mask;
        nb = gsdf_block_find_or_insert(dst, bk, h, dst.bkeys[h]);
        if (nb < 0) atomicOr(&st->status, GSDF_STATUS_TABLE_FULL);
    }
    nb = __shfl(nb, 0);
    if (nb < 0) return;
    const float* v = stage + ((size_t)b * GSDF_BLOCK_VOX + lane) * 5;
    if (!(v[0] > 0.f)) return;                                 /* the voxel receives nothing */
    gsdf_payload* p = dst.vox + ((size_t)nb * GSDF_BLOCK_VOX + lane);
    gsdf_payload r = *p;
    r.w += v[0]; r.s += v[1]; r.gx += v[2]; r.gy += v[3]; r.gz += v[4];
    *p = r;
}

/* events around the stages (gsdf_merge_posed_last); released on every return */
struct stage_events {
    hipEvent_t e[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    hipError_t create() {
        for (auto& x : e) { const hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; }
        return hipSuccess;
    }
    ~stage_events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
};

bool pose_ok(const float pose7[7]) { return gsdf_pose7_ok(pose7); }

} // namespace

extern "C" {

int gsdf_merge_from_posed(gsdf_ctx* dst, gsdf_ctx* src, const float pose7[7], int64_t* n_voxels, int64_t* n_blocks) {
    if (n_voxels) *n_voxels = 0;
    if (n_blocks) *n_blocks = 0;
    if (!dst || !src || dst == src) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: two different contexts are needed");
    if (!pose7) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: null pose");
    if (dst->device != src->device) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: the contexts live on different devices");
    if (dst->voxel_size != src->voxel_size || dst->T != src->T) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: voxel size / truncation differ");
    if (dst->map_type == GSDF_MAP_BASE || src->map_type == GSDF_MAP_BASE)
        return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: not available on a base-sdf context (it reads and rotates the stored gradient)");
    if (dst->map.vis || src->map.vis)
        return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: not available with gsdf_enable_vis (vis_ is not carried across a resampling)");
    if (!pose_ok(pose7)) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: the pose must be finite with | |q|^2 - 1 | <= 1e-4");
    HIP_TRY(hipSetDevice(dst->device));
    if (int rc = gsdf_flush_pending(src)) return rc;
    if (int rc = gsdf_flush_pending(dst)) return rc;
    dst->posed_last = gsdf_posed_last();

    gsdf_pose_arg pose;
    gsdf_quat_to_R(pose7 + 3, pose.R);                         /* no renormalisation: the bits of Oracle.quat_to_R */
    std::memcpy(pose.t, pose7, sizeof(pose.t));
    gsdf_posed_map pm;
    if (!gsdf_posed_map_make(pose.R, pose.t, dst->voxel_size, &pm)) return gsdf_fail(GSDF_ERR_INVALID, "gsdf_merge_from_posed: the pose's rotation is singular");

    /* the source map is complete (and stays untouched): everything from here on runs on dst's stream */
    gsdf_dev_state ss, ds;
    HIP_TRY(hipMemcpyAsync(&ss, src->st, sizeof(ss), hipMemcpyDeviceToHost, src->stream));
    HIP_TRY(hipStreamSynchronize(src->stream));
    if (ss.status & GSDF_STATUS_TABLE_FULL) return gsdf_fail(GSDF_ERR_TABLE_FULL, "gsdf_merge_from_posed: the source map reported a full table");
    stage_events ev;
    HIP_TRY(ev.create());
    gsdf_dev<unsigned long long> words;
    HIP_TRY(words.alloc(PW_COUNT_));
    HIP_TRY(hipMemsetAsync(words, 0, PW_COUNT_ * sizeof(unsigned long long), dst->stream));
    const size_t nb_src = src->n_slots / GSDF_BLOCK_VOX;
    hipLaunchKernelGGL(k_posed_count_blocks, dim3(64), dim3(256), 0, dst->stream, dst->tab.bkeys, dst->n_slots / GSDF_BLOCK_VOX, words + PW_DST_BLOCKS);
    HIP_TRY(hipMemcpyAsync(&ds, dst->st, sizeof(ds), hipMemcpyDeviceToHost, dst->stream));
    const unsigned int cgrid = (unsigned int)std::min<size_t>((nb_src + 255) / 256, 1024);
    unsigned long long n_cand = 0;
    HIP_TRY(gsdf_counted(dst, [&] {
        hipLaunchKernelGGL(k_posed_candidates, dim3(cgrid), dim3(256), 0, dst->stream, src->tab.bkeys, nb_src, pm, nullptr, dst->counter, 0, words + PW_RANGE);
    }, &n_cand));

    unsigned long long h[PW_COUNT_] = { 0 };
    gsdf_dev<unsigned long long> cand, sorted, uniq;
    gsdf_dev<void> tmp;
    gsdf_dev<float> stage;
    gsdf_dev<uint32_t> flags;
    size_t nu = 0;
    if (n_cand) {
        const size_t nc = (size_t)n_cand;
        HIP_TRY(cand.alloc(nc));
        HIP_TRY(sorted.alloc(nc));
        HIP_TRY(uniq.alloc(nc));
        size_t need = 0;
        HIP_TRY(gsdf_sort_keys_u64_need(nc, &need));
        HIP_TRY(gsdf_unique_u64_need(nc, &need));
        HIP_TRY(tmp.alloc(need));
        HIP_TRY(gsdf_counter_zero(dst));
        HIP_TRY(hipEventRecord(ev.e[0], dst->stream));
        hipLaunchKernelGGL(k_posed_candidates, dim3(cgrid), dim3(256), 0, dst->stream, src->tab.bkeys, nb_src, pm, cand.get(), dst->counter, (long long)nc, words + PW_RANGE);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[1], dst->stream));
        HIP_TRY(gsdf_sort_keys_u64(tmp, cand, sorted, nc, dst->stream));
        HIP_TRY(gsdf_unique_u64(tmp, sorted, uniq, words + PW_UNIQUE, nc, dst->stream));
        HIP_TRY(hipEventRecord(ev.e[2], dst->stream));
        HIP_TRY(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, dst->stream));
        HIP_TRY(hipStreamSynchronize(dst->stream));
        nu = (size_t)h[PW_UNIQUE];
        HIP_TRY(stage.alloc(nu * GSDF_BLOCK_VOX * 5));
        HIP_TRY(flags.alloc(nu));
        HIP_TRY(hipEventRecord(ev.e[3], dst->stream));
        hipLaunchKernelGGL(k_posed_sample, dim3((unsigned int)((nu + 3) / 4)), dim3(256), 0, dst->stream, src->tab, dst->voxel_size, dst->voxel_size_inv,
                           dst->T, pose, uniq.get(), (long long)nu, stage.get(), flags.get(), words.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[4], dst->stream));
    }
    HIP_TRY(hipMemcpyAsync(h, words, sizeof(h), hipMemcpyDeviceToHost, dst->stream));
    HIP_TRY(hipStreamSynchronize(dst->stream));
    const size_t n_dst = (size_t)h[PW_DST_BLOCKS], n_ins = (size_t)h[PW_BLOCKS];
    /* Room in dst, by the rule of gsdf_merge_from -- with the exact number of find-or-insert operations instead of a bound: at
     * most n_dst + n_ins blocks afterwards.  dst has not been touched yet. */
    if (n_ins) {
        const size_t worst = n_dst + n_ins;
        int need = dst->capacity_log2;
        while (need < 30 && worst * 100u > (((size_t)1 << need) / GSDF_BLOCK_VOX) * 45u) ++need;
        if (need > dst->capacity_log2 && dst->auto_grow_max > dst->capacity_log2) {
            if (int rc = gsdf_grow_impl(dst, std::min(need, dst->auto_grow_max))) return rc;
        }
        if (worst * 100u > (dst->n_slots / GSDF_BLOCK_VOX) * 90u)
            return gsdf_fail(GSDF_ERR_TABLE_FULL, "gsdf_merge_from_posed: dst cannot hold its blocks and the " + std::to_string(n_ins) + " the merge writes to (" +
                             std::to_string(n_dst) + " of " + std::to_string(dst->n_slots / GSDF_BLOCK_VOX) +
                             " entries in use); dst is unchanged -- gsdf_grow it or allow it with gsdf_set_auto_grow");
        hipLaunchKernelGGL(k_posed_add, dim3((unsigned int)((nu + 3) / 4)), dim3(256), 0, dst->stream, dst->tab, uniq.get(), (long long)nu, stage.get(),
                           flags.get(), dst->st.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[5], dst->stream));
        dst->occ_dirty = true;
        dst->ba_gate_fresh = false;
        dst->grow_forget = true;
        gsdf_dev_state after;
        HIP_TRY(hipMemcpyAsync(&after, dst->st, sizeof(after), hipMemcpyDeviceToHost, dst->stream));
        HIP_TRY(hipStreamSynchronize(dst->stream));
        /* (possible between 45 % and 90 % only in theory, as in gsdf_merge_from: dst then holds part of the merge) */
        if (after.status & GSDF_STATUS_TABLE_FULL) return gsdf_fail(GSDF_ERR_TABLE_FULL, "voxel hash table full (probe budget exhausted)");
    }
    gsdf_launch_set_frames(dst->stream, dst->st, (long long)(ds.frames + ss.frames));   /* Sdf::counter_ = frames of both */
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(dst->stream));
    gsdf_posed_last& L = dst->posed_last;
    L.candidates = (long long)n_cand; L.unique = (long long)nu;
    if (n_cand) {
        (void)hipEventElapsedTime(&L.ms[0], ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&L.ms[1], ev.e[1], ev.e[2]);
        (void)hipEventElapsedTime(&L.ms[2], ev.e[3], ev.e[4]);
        if (n_ins) (void)hipEventElapsedTime(&L.ms[3], ev.e[4], ev.e[5]);
        (void)hipGetLastError();
    }
    if (n_voxels) *n_voxels = (int64_t)h[PW_VOXELS];
    if (n_blocks) *n_blocks = (int64_t)n_ins;
    if (h[PW_RANGE])
        return gsdf_fail(GSDF_ERR_KEY_RANGE, "gsdf_merge_from_posed: part of src lands outside the packable +-2^20 voxel range and was left out");
    return GSDF_OK;
}

int gsdf_merge_posed_last(gsdf_ctx* dst, int64_t counts[2], float ms[4]) {
    if (!dst) return gsdf_fail(GSDF_ERR_INVALID, "null context");
    if (counts) { counts[0] = dst->posed_last.candidates; counts[1] = dst->posed_last.unique; }
    if (ms) std::memcpy(ms, dst->posed_last.ms, sizeof(dst->posed_last.ms));
    return GSDF_OK;
}

#ifdef GSDF_EXPERIMENTS
/* gsdf_posed_blocks as k_posed_candidates uses it, for the tests: no context, no device.  block3: signed block index of a src
 * block; out: up to max_n rows of 3 signed dst block indices.  Returns the number of blocks (rows beyond max_n are not written),
 * -1 for an image that is not enumerated, -2 for a bad argument. */
int gsdf_debug_posed_blocks(const float pose7[7], float vs, const int32_t block3[3], int32_t* out, int max_n) {
    if (!pose7 || !block3 || (max_n > 0 && !out)) return -2;
    float R[9];
    gsdf_quat_to_R(pose7 + 3, R);
    gsdf_posed_map pm;
    if (!gsdf_posed_map_make(R, pose7, vs, &pm)) return -2;
    int o = 0;
    return gsdf_posed_blocks(pm, block3[0], block3[1], block3[2], [&](int x, int y, int z) {
        if (o < max_n) { out[3 * o] = x; out[3 * o + 1] = y; out[3 * o + 2] = z; }
        ++o;
    });
}
#endif

} // extern "C"
