/*
 * gsdf_ctx.h -- the context behind the C-ABI handle (private to libgsdf.so: gsdf_capi.hip, gsdf_merge.hip, gsdf_color.hip).
 */
#ifndef GSDF_CTX_H_
#define GSDF_CTX_H_

#include "../../include/gsdf.h"
#include "gsdf_dev.h"
#include "gsdf_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <string>
#include <utility>
#include <vector>

#define GSDF_SCRATCH_BYTES (256 * 1024)
#define GSDF_MX_BUFS 8
#define GSDF_GROW_MAX_LAG_DEFAULT 8       /* auto-grow: frame entries the host may be ahead of the newest finished block count */
enum { GSDF_SEL_NONE = 0, GSDF_SEL_VALID = 1, GSDF_SEL_LOST = 2 };   /* gsdf_ctx::sel_state */
#define GSDF_PROF_SLOTS 5    /* gsdf_profile: 0 normals, 1 fusion, 2 tracking launches, 3 raycast, 4 tracker (whole optimize) */

inline thread_local std::string g_gsdf_err;

struct gsdf_ctx;
int gsdf_flush_pending(gsdf_ctx* c);               /* gsdf_capi.hip: launch the deferred GT-pose fusion, if one waits */
int gsdf_grow_impl(gsdf_ctx* c, int new_capacity_log2);      /* gsdf_merge.hip: rehash into a larger table */
/* gsdf_merge.hip: the rebuild behind gsdf_grow and gsdf_compact -- every block (skip_dead: every block that holds a voxel with
 * w > 0) moves into a fresh table of 2^new_capacity_log2 records; on any failure the old table stays.  *n_dropped (nullable) =
 * blocks left behind.  `who` names the entry in messages.  The caller has checked the capacity and flushed. */
int gsdf_rebuild_impl(gsdf_ctx* c, int new_capacity_log2, bool skip_dead, long long* n_dropped, const char* who);
void gsdf_enqueue_block_count(gsdf_ctx* c, unsigned int tag);   /* gsdf_merge.hip: existing blocks | tag << 32 -> pinned words progress[4..5] */

inline int gsdf_fail(int code, const std::string& msg) {
    g_gsdf_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return gsdf_fail(GSDF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

/* the pinned progress word the pass heads write: serial << 16 | done << 15 | passes (gsdf_track_params::progress) */
struct gsdf_progress { unsigned int serial; bool done; int passes; };
inline gsdf_progress gsdf_progress_decode(unsigned int w) { return { w >> 16, (w & 0x8000u) != 0u, (int)(w & 0x7FFFu) }; }

/* how a tracked frame uses what was computed ahead of it, and what it promises to the next one (gsdf_lookahead::consume) */
struct gsdf_frame_route {
    int fuse_set = 2;                              /* the normal planes the frame's fusion reads: set 2, or the hinted one */
    unsigned int ride_token = 0;                   /* != 0: the frame's normals were computed ahead under this token */
    const float* hint = nullptr;                   /* the NEXT frame, whose normals every fusion launch of this frame carries ... */
    int next_set = 0;                              /* ... into this set ... */
    unsigned int next_token = 0;                   /* ... leaving this token in st->nrm_token if its gate was open */
};

/* The frame loop's look-ahead state: everything computed or promised AHEAD of the frame an entry works on.  The operations
 * below are the only code that writes it (reading through gsdf_ctx::ahead is fine): an entry that invalidates a buffer or a
 * statistic names what happens, not the fields to null. */
struct gsdf_lookahead {
    /* a GT-pose fusion whose launch waits for the next gsdf_update_dev (its launch then also computes that frame's normals) */
    struct pending_fuse { bool valid = false; const float* depth = nullptr; gsdf_pose_arg pose; int set = 0; } pending;
    int nrm_parity = 0;                            /* which set of normal planes the next GT-pose fusion uses (0 / 1; set 2: tracked frames) */
    /* gsdf_hint_next_depth_dev: the frame the NEXT gsdf_track_and_fuse_dev will be called with (set by the caller, consumed by the
     * next frame entry), and the frame whose normals a fusion launch has already computed into set nrm_ready_set (0 / 1) */
    const float* hint_next = nullptr;
    const float* nrm_ready_depth = nullptr;
    int nrm_ready_set = -1;
    unsigned int nrm_ready_token = 0, nrm_token_ctr = 0;   /* what that fusion launch leaves in st->nrm_token when its gate was open */
    unsigned int prev_track_serial = 0; int prev_first_last = 0; bool prev_slow = false;   /* the last tracked frame: did it need more than its first batch (as far as the host knows)? */

    /* does [p, p + bytes) overlap the frame (frame_bytes long) at `frame`? */
    static bool overlaps(const void* p, size_t bytes, const float* frame, size_t frame_bytes) {
        const uintptr_t a0 = (uintptr_t)p, b0 = (uintptr_t)frame;
        return a0 < b0 + frame_bytes && b0 < a0 + bytes;
    }
    void hint(const float* next_depth) { hint_next = next_depth; }      /* nullptr withdraws it */
    /* the frames named or computed ahead are forgotten: the next frame's own tracker launches compute its normals */
    void forget_frames() { hint_next = nullptr; nrm_ready_depth = nullptr; }
    /* ... and a fusion that was never launched is dropped, the last tracked frame forgotten (a new scan) */
    void forget_all() { forget_frames(); pending.valid = false; prev_track_serial = 0; prev_slow = false; }
    /* [p, p + bytes) is about to change or go away: a hinted frame or one whose normals were computed ahead in it belongs to the
     * old contents -- forgotten.  Returns whether the waiting GT-pose fusion reads from it (the caller's to deal with). */
    bool range_changes(const void* p, size_t bytes, size_t frame_bytes) {
        for (const float** q : { &nrm_ready_depth, &hint_next })
            if (*q && overlaps(p, bytes, *q, frame_bytes)) *q = nullptr;
        return pending.valid && overlaps(p, bytes, pending.depth, frame_bytes);
    }
    /* the set of the next GT-pose fusion; sets 0 / 1 are also where a hinted tracked frame's normals wait: those are gone */
    int take_gt_set() { const int set = nrm_parity; nrm_parity ^= 1; nrm_ready_depth = nullptr; return set; }
    void hold(const float* depth, const gsdf_pose_arg& pose, int set) { pending.valid = true; pending.depth = depth; pending.pose = pose; pending.set = set; }
    void release() { pending.valid = false; }
    /* the tracked frame `serial` was queued; first_last: the last launch index of its first batch */
    void tracked(unsigned int serial, int first_last) { prev_track_serial = serial; prev_first_last = first_last; }
    /* a look at the progress word without waiting: if it tells how the last tracked frame ended, was that beyond its first batch? */
    void note_progress(unsigned int word) {
        const gsdf_progress p = gsdf_progress_decode(word);
        if (prev_track_serial && p.serial == prev_track_serial && p.done) prev_slow = p.passes > prev_first_last;
    }
    /* gsdf_hint_next_depth_dev, for the tracked frame at depth_dev: (1) its normals may already lie in set 0 / 1 -- the previous
     * frame's fusion computed them in its tail IF IT RAN (a fusion whose gate stays closed does not: its tail is not idle, the
     * tiles would run in the open); the frame's riders are queued as ever and leave at once when they find the frame's token in
     * st->nrm_token; (2) if the new route is taken every fusion launch of this frame carries the normals role for the hinted
     * NEXT frame (at most one of them passes the gate).  `ahead_ok`: false in event-timed replays (gsdf_profile) -- there the
     * fusion launch is the plain one, so that what bench.py quotes as k_fuse's duration is the fusion work alone -- and for
     * frames that are not tracked and fused. */
    gsdf_frame_route consume(const float* depth_dev, bool ahead_ok, bool new_route) {
        gsdf_frame_route r;
        if (ahead_ok && nrm_ready_depth == depth_dev && nrm_ready_set >= 0) { r.fuse_set = nrm_ready_set; r.ride_token = nrm_ready_token; }
        r.hint = new_route && hint_next != depth_dev ? hint_next : nullptr;
        forget_frames();                             /* consumed (or not ours) */
        if (r.hint) {
            r.next_set = r.fuse_set == 0 ? 1 : 0;    /* whichever of sets 0 / 1 this frame's fusion does not read */
            if (++nrm_token_ctr == 0u) nrm_token_ctr = 1u;
            r.next_token = nrm_token_ctr;
            nrm_ready_depth = r.hint; nrm_ready_set = r.next_set; nrm_ready_token = r.next_token;
        }
        return r;
    }
};

/* The context's device memory, one struct per lifetime.  Each is built in a local and moved into the context once its last
 * allocation succeeded, so the context holds a whole group or an empty one -- never half of one. */

/* the table (gsdf_create, gsdf_grow); gsdf_ctx::tab is the POD view of it the kernels take by value */
struct gsdf_map_bufs {
    gsdf_dev<gsdf_payload> vox;
    gsdf_dev<unsigned long long> bkeys;
    gsdf_dev<uint32_t> occ;                        /* block filter (64 bits per block entry), then the cell filter (1 bit per block entry, at least one word) */
    gsdf_dev<uint32_t> vis;                        /* optional vis_ bit-vectors, n_slots x vis_words (gsdf_enable_vis) */
    hipError_t alloc(size_t n_slots, size_t vis_words) {
        hipError_t e;
        if ((e = vox.alloc(n_slots)) != hipSuccess || (e = bkeys.alloc(n_slots / GSDF_BLOCK_VOX)) != hipSuccess ||
            (e = occ.alloc(n_slots / 32 + std::max<size_t>(n_slots / GSDF_BLOCK_VOX / 32, 1))) != hipSuccess) return e;
        return vis_words ? vis.alloc(n_slots * vis_words) : hipSuccess;
    }
    gsdf_table table(size_t n_slots) const { return gsdf_table{ bkeys, vox, (uint32_t)(n_slots / GSDF_BLOCK_VOX - 1), occ }; }
};

/* normal estimator, frame scratch and tracker rows: everything gsdf_normals_init allocates (planes != nullptr: there is a frame) */
struct gsdf_frame_bufs {
    gsdf_dev<float> planes;                        /* 11 planes */
    gsdf_dev<float> depth_stage;                   /* H2D staging for host-pointer entry points */
    gsdf_dev<float> normals;                       /* 3 sets of 3 planes */
    gsdf_dev<uint32_t> tile_stats;                 /* per set: [fuse_blocks][4] statistics of the frame's fusion tiles (gsdf_kernels.hip: gsdf_tile_stats) */
    gsdf_dev<double> partials;                     /* 3 rotating buffers of tracker partial sums */
    gsdf_dev<unsigned long long> blk_counters;
    gsdf_dev<unsigned int> tile_flags;             /* per-tile hand-off flags of k_fuse */
    gsdf_dev<uint32_t> tile_order;                 /* launch order of the fusion tiles (gsdf_fuse_tile_order) */
    gsdf_dev<gsdf_deferred> deferred;
    gsdf_dev<unsigned int> deferred_count;
    gsdf_dev<unsigned int> fuse_ticket;            /* arrivals of finished k_fuse workgroups (reset by the last one) */
    gsdf_dev<float> frame_log;
    gsdf_dev<float> depth_sampled;                 /* the compacted pixels of gsdf_track_sampled (sampling > 1), lazily allocated */
};

/* PhotoBA: everything gsdf_ba_setup allocates.  gate_list, gate_tmp, counter2 and mean are optional (the sweeps use the whole table) */
struct gsdf_ba_bufs {
    gsdf_dev<float> images;
    gsdf_dev<float> Rt;                            /* n x 9 rotations then n x 3 translations */
    gsdf_dev<int> frame_idx;
    gsdf_dev<double> block_E;
    gsdf_dev<float> block_part;
    gsdf_dev<float> Hb;
    gsdf_dev<uint32_t> gate_list;                  /* slots of the voxels with |dist| <= voxel size (the gate of getEnergy / solvePose), slot order */
    gsdf_dev<void> gate_tmp;                       /* rocPRIM select scratch */
    gsdf_dev<unsigned long long> counter2;         /* device word: entries of gate_list */
    gsdf_dev<void> mean;                           /* per entry of gate_list: what the last energy sweep's first loop found (24 B each; gsdf_ba_dev::mean_cache) */
    gsdf_dev<float> full_part;                     /* the coupled pose system's per-workgroup partial tiles (allocated by the first coupled call) */
    gsdf_dev<float> full_H;                        /* ... and its (6n)^2 matrix */
};

/* ColorUpsampler (gsdf_color.hip): the snapshot and the scratch of its compute; the buffers grow and are kept */
struct gsdf_color_state {
    bool valid = false;
    long long n = 0, obs = 0;
    float vs = 0.f;
    gsdf_dev<unsigned long long> keys;             /* packed (z, y, x)-ordered keys */
    gsdf_dev<float> rows;                          /* GSDF_COLOR_ROW floats per key */
    long long cloud_n = -1;                        /* the cloud of the snapshot, made on first request */
    gsdf_dev<float> cloud;
    /* scratch of the compute */
    gsdf_dev<float> images, Rt;
    gsdf_dev<int> fidx;
    gsdf_dev<uint32_t> list, slots, counts, offsets;
    gsdf_dev<unsigned long long> keys_in;
    gsdf_dev<void> tmp;                            /* rocPRIM scratch */
    gsdf_dev<unsigned long long> words;            /* [0] selected voxels, [1] observations */
    void drop() { valid = false; n = 0; obs = 0; cloud_n = -1; }   /* forgets the snapshot, keeps the buffers (gsdf_reset) */
};

/* what the last gsdf_merge_from_posed into this context did (gsdf_merge_posed_last): candidate blocks before / after unique;
 * event times of the candidate list's filling pass, sort + unique, k_posed_sample, k_posed_add (ms) */
struct gsdf_posed_last {
    long long candidates = 0, unique = 0;
    float ms[4] = { 0.f, 0.f, 0.f, 0.f };
};

struct gsdf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    gsdf_lookahead ahead;                          /* the frame loop's look-ahead state (above) */
    int defer = 1;                                 /* pipeline runs of gsdf_update_dev that way (GSDF_DEFER=0: launch at once) */
    int nrm_split = 30, nrm_split2 = 40;           /* per cent of a tracked frame's normals tiles computed in its first / second tracker launch (rest: third) */
    /* MapGradPixelSdf / Sdf members */
    float voxel_size = 0, voxel_size_inv = 0, T = 0, inv_T = 0;
    float zmin = 0.5f, zmax = 3.5f;                /* Sdf.h:67-68 */
    int map_type = GSDF_MAP_GRAD;                  /* gsdf_set_map_type: GSDF_MAP_BASE = MapPixelSdf (gather and query differ) */
    int factor = 0;
    /* table */
    int capacity_log2 = 0;
    size_t n_slots = 0;
    gsdf_map_bufs map;
    gsdf_table tab{ nullptr, nullptr, 0, nullptr };  /* = map.table(n_slots) */
    /* normal estimator + frame scratch */
    int W = 0, H = 0, win = 0;
    float K[9] = { 0 };
    gsdf_frame_bufs frame;
    /* tracker */
    gsdf_dev<gsdf_dev_state> st;
    unsigned int track_rot = 0;                    /* tracker launches issued so far, mod 3 (selects the sum buffers) */
    int track_blocks = 0;
    int fuse_blocks = 0;                           /* tiles of a frame */
    unsigned int deferred_cap = 0;
    unsigned int fuse_tag = 0;                     /* serial of the last fusion launch */
    int vis_words = 0;                             /* words per voxel of map.vis */
    gsdf_dev<unsigned long long> rc_counts;        /* raycaster: per-workgroup rows of 8 (samples, records, fast / slow iterations of wave 0) */
    long long rc_iters[2] = { 0, 0 };              /* loop iterations of the workgroups' wave 0 as of the last gsdf_raycast_counters */
    bool fuse_head = true;                         /* the frame's first fusion launch performs the head of the first batch's last tracker launch (GSDF_FUSE_HEAD) */
    gsdf_dev<void> scratch;                        /* device scratch of gsdf_query / gsdf_get_voxels for small batches (GSDF_SCRATCH_BYTES) */
    gsdf_dev<void> align;                          /* gsdf_align_points: the run's state, then the partial rows (allocated by the first call) */
    bool occ_dirty = false;                        /* blocks may have been inserted since the raycaster's filters (gsdf_table::occ) were built */
    /* the reference's map grows without bound (MapGradPixelSdf.h:65-68); here: gsdf_grow, or by itself when gsdf_set_auto_grow
     * named a limit -- every few fusions the number of existing blocks is counted into a pinned word, and a frame entry that
     * finds the key array more than GSDF_GROW_LOAD full doubles the table first */
    int auto_grow_max = 0;                         /* largest capacity_log2 auto-grow may reach; 0 = off */
    unsigned int grow_seq = 0;                     /* frame entries since auto-grow was switched on / the map was reset or grown */
    unsigned int grow_last_enq = 0;                /* entry whose count was enqueued last */
    unsigned int grow_prev_seq = 0, grow_prev_cnt = 0;   /* the newest finished count the growth rate was updated from */
    unsigned int grow_rate = 0;                    /* blocks a frame added lately (max over recent counts, decaying) */
    int grow_counts_seen = 0;                      /* finished counts seen since grow_seq restarted (the rate needs two) */
    bool grow_forget = false;                      /* set by gsdf_grow / gsdf_reset: restart the bookkeeping above */
    int grow_max_lag = GSDF_GROW_MAX_LAG_DEFAULT;
    long long grow_syncs = 0;                      /* entries that had to wait for an exact count (statistics for the tests) */
    gsdf_dev<unsigned int> grow_scratch;           /* two device words of k_count_blocks */
    bool merged = false;                           /* gsdf_merge_allreduce has run: the map is the sum of all ranks (one-shot) */
    gsdf_dev<void> mx[GSDF_MX_BUFS];               /* scratch of the exchange (gsdf_merge.hip): grows, never shrinks */
    gsdf_posed_last posed_last;                    /* gsdf_merge_from_posed with this context as dst (gsdf_merge_posed.hip) */
    /* the selection (gsdf_select.hip): one 64-bit word per block entry of the PRESENT table, bit = gsdf_block_local; allocated by
     * the first select call, with a second bitmap of the same size behind it (the predicate set of the running call) */
    gsdf_dev<unsigned long long> sel;
    int sel_state = GSDF_SEL_NONE;                 /* none / valid / lost (a rehash moved the slots) */
    /* PhotoBA (PhotometricOptimizer) */
    int ba_n = 0;
    float ba_reg = 10.f;
    float ba_trunc_sq = -1.f;                      /* OptSettings::lambda_sq when loss == TRUNC_L2, else < 0 */
    gsdf_ba_bufs ba;
    std::vector<float> ba_R, ba_t;                 /* host copies of the keyframe poses being optimised */
    bool ba_gate_fresh = false;                    /* ba.gate_list matches the distances in the table */
    int ba_pose_step = 0;                          /* gsdf_ba_set_pose_step: the pose step of gsdf_ba_optimize (0 solvePose, 1 solvePoseFull) */
#ifdef GSDF_EXPERIMENTS
    std::vector<float> ba_last_delta;              /* gsdf_debug_ba_delta */
#endif
    int ba_mean_on = 1;                            /* GSDF_BA_MEAN_CACHE (read by gsdf_ba_setup) */
    bool ba_mean_valid = false;                    /* ... at the very state (poses, distances, gate list) the next pose sweep will see */
    long long ba_last_voxels = 0, ba_last_obs = 0; /* what the last energy sweep read back counted (gsdf_ba_counters) */
    gsdf_color_state color;                        /* ColorUpsampler (gsdf_color_compute) */
    unsigned int track_serial = 0;                 /* optimize() call counter */
    gsdf_pinned<unsigned int> progress;            /* 16 pinned host words written by the tracker epilogue, the fusion and the block count */
    int adaptive = 1;                              /* issue tracker passes in batches, following the device (see enqueue_track) */
    int far_table = -1;                            /* fusion kernel's LDS table: -1 chosen per launch from the previous fusions, 0 / 1 pinned */
    long long fuse_launches = 0, far_table_launches = 0; /* fusion launches since create/reset, and those with the larger table (gsdf_get_stats) */
    int first_batch = 5, next_batch = 8;           /* launches per batch: 5 cover the usual <= 4 passes + their last head; a frame that needs
                                                      more is most likely one that runs all 25 (pass counts on the bench stream: 142 x <= 6, 7 x 7..22,
                                                      51 x 25) -- batches of 8 behind the first: 6 656 -> 6 815 frames/s on the default window (4 / 12 / 21: 6 656 / 6 780 / 6 760) */
    int lazy_fuse = 1;                             /* the frame's fusion is queued behind the first and the last batch of passes only; in between once optimize() has ended */
    gsdf_dev<unsigned long long> trace;            /* test build: per-workgroup time stamps of k_fuse (gsdf_debug_flags & 64) */
    int debug = 0;                                 /* path-forcing / measurement switches (gsdf_debug_flags; test build only) */
    long long frame_log_cap = 0;
    /* misc */
    gsdf_dev<unsigned long long> counter;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool profiling = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events[GSDF_PROF_SLOTS];
    std::vector<hipEvent_t> event_pool;
    /* gsdf_mark: events recorded on the stream, retired in order */
    std::deque<std::pair<long long, hipEvent_t>> marks;
    std::vector<hipEvent_t> mark_pool, upload_pool;
    long long mark_serial = 0;
    hipStream_t copy_stream = nullptr;             /* gsdf_dev_upload_ahead: created on first use */
    std::deque<std::pair<long long, hipEvent_t>> uploads;
    long long upload_serial = 0;
    double prof_ms[GSDF_PROF_SLOTS] = { 0 };
    std::vector<float> prof_each[GSDF_PROF_SLOTS];  /* every launch's duration since the last gsdf_profile(c, 1) (gsdf_profile_read_launches) */
    long long prof_n[GSDF_PROF_SLOTS] = { 0 };

    size_t frame_bytes() const { return (size_t)W * H * sizeof(float); }
    gsdf_frame_geom geom() const {
        gsdf_frame_geom g;
        g.W = W; g.H = H;
        g.fx = K[0]; g.fy = K[4]; g.cx = K[2]; g.cy = K[5];
        g.vs = voxel_size; g.inv_vs = voxel_size_inv; g.T = T; g.inv_T = inv_T;
        g.zmin = zmin; g.zmax = zmax; g.factor = factor;
        return g;
    }
    gsdf_ncache ncache() const {
        const size_t N = (size_t)W * H;
        gsdf_ncache nc;
        const float* planes = frame.planes;
        nc.x0 = planes; nc.y0 = planes + N; nc.x0n = planes + 2 * N; nc.y0n = planes + 3 * N;
        nc.ninv = planes + 4 * N; nc.q11 = planes + 5 * N; nc.q12 = planes + 6 * N; nc.q13 = planes + 7 * N;
        nc.q22 = planes + 8 * N; nc.q23 = planes + 9 * N; nc.q33 = planes + 10 * N;
        return nc;
    }
};

#endif /* GSDF_CTX_H_ */
