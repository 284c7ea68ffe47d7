/*
 * gsdf_capi.hip -- host side of libgsdf.so: the C-ABI declared in include/gsdf.h.
 *
 * Owns the HBM-resident state (voxel hash table, cached normal-estimator planes, frame
 * scratch, tracker state) and enqueues the gfx950 kernels on one HIP stream.  There is no
 * CPU implementation behind these entry points: without a GPU gsdf_create fails with
 * GSDF_ERR_NO_DEVICE.
 */
#include "../../include/gsdf.h"
#include "../../include/gsdf_mc_tables.h"
#include "gsdf_ctx.h"
#include "gsdf_kernels.h"
#include "gsdf_align_loss.h"
#include "gsdf_math.h"
#include "gsdf_sweep.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

static int fail(int code, const std::string& msg) { return gsdf_fail(code, msg); }

namespace {

hipEvent_t take_event(gsdf_ctx* c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    /* timing events only: no system-scope fence when they are recorded (the cache write-back and invalidation it implies would
     * be charged to the kernels they bracket, and slow the ones behind them) */
    hipEvent_t e = nullptr;
    (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
    return e;
}

struct prof_scope {
    gsdf_ctx* c; int which; hipEvent_t a = nullptr, b = nullptr;
    prof_scope(gsdf_ctx* c_, int w) : c(c_), which(w) {
        if (c->profiling) { a = take_event(c); b = take_event(c); (void)hipEventRecord(a, c->stream); }
    }
    ~prof_scope() {
        if (c->profiling) { (void)hipEventRecord(b, c->stream); c->prof_events[which].push_back({ a, b }); }
    }
};

void prof_collect(gsdf_ctx* c) {
    for (int k = 0; k < GSDF_PROF_SLOTS; ++k) {
        for (auto& pr : c->prof_events[k]) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                c->prof_ms[k] += ms; c->prof_n[k] += 1;
                if (c->prof_each[k].size() < (size_t)1 << 20) c->prof_each[k].push_back(ms);
            }
            c->event_pool.push_back(pr.first);
            c->event_pool.push_back(pr.second);
        }
        c->prof_events[k].clear();
    }
}

int status_to_code(int status) {
    if (status & GSDF_STATUS_TABLE_FULL) return fail(GSDF_ERR_TABLE_FULL, "voxel hash table full (probe budget exhausted)");
    if (status & GSDF_STATUS_KEY_RANGE) return fail(GSDF_ERR_KEY_RANGE, "voxel index outside the packable +-2^20 range");
    return GSDF_OK;
}

int require_frame(gsdf_ctx* c) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    if (!c->frame.planes) return fail(GSDF_ERR_INVALID, "gsdf_normals_init must be called first (NEst == nullptr, MapGradPixelSdf.cpp:55-58)");
    return GSDF_OK;
}

/* Which size of the fusion kernel's LDS table (gsdf_kernels.hip, FUSE_LCAP): the larger one while many tiles did not fit the
 * small one lately (far geometry).  The count comes from a pinned word the last workgroup of every fusion writes; it lags by a
 * launch or two -- a hint, never a condition for correctness (either kernel fuses any tile). */
static int fuse_far_table(const gsdf_ctx* c) {
#ifdef GSDF_EXPERIMENTS
    if (c->debug & 1024) return 1;                         /* tests: pin the larger table */
    if (c->debug & 2048) return 0;
#endif
    if (c->far_table >= 0) return c->far_table;
    return c->progress && c->progress[3] * 16u > (unsigned int)c->fuse_blocks ? 1 : 0;
}

/* the spin-wait hint of an x86 host; elsewhere the core is given away */
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
}
/* Polls until done() holds: spins briefly (what the host waits for takes ~50 us), then yields the core between looks; bounded by
 * TIME, not by iterations.  false = gave up after limit_s seconds */
template <class Done>
static bool spin_until(Done done, double limit_s) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long spin = 0; !done(); ++spin) {
        if (spin < 4096) { cpu_relax(); continue; }
        if ((spin & 63) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit_s) return false;
        std::this_thread::yield();
    }
    return true;
}

/* Auto-grow (gsdf_set_auto_grow): called at the top of the frame entries (gsdf_update_dev, gsdf_track_and_fuse_dev).
 *
 * The table is doubled once 45 % of its block entries are in use (the probe budget runs out near 95 %).  The load is the
 * count a 64-workgroup kernel leaves in a pinned word; it is enqueued at the top of every entry (every fourth while the
 * estimate is below 25 %), tagged with the entry's
 * number, and read without waiting -- so the number the host sees is some entries old, and the host may run ahead of the
 * device (an unsynchronised gsdf_update_dev loop).  What keeps the doubling in time:
 *  - the age of the count is known (the tag), and so is how fast the map grew lately (max over the recent counts, decaying):
 *    while  count + 2 x (entries not covered) x (blocks per frame)  stays below the 45 % the host does not wait;
 *  - otherwise, and whenever the count is more than grow_max_lag (8) entries old, the entry waits: for the lag it polls the
 *    pinned word (the device keeps running, no bubble); for the load it flushes, counts and synchronises -- the EXACT load
 *    decides the doubling;
 *  - until two counts have been seen (the first entries of a scan, after a reset or a doubling) every entry is exact: a
 *    first frame that fills half the table is seen before the second one is queued.
 * What remains possible: ONE frame that adds more blocks than the table has room for (more than half its entries beyond the
 * 45 %) still sets the sticky GSDF_STATUS_TABLE_FULL -- its samples are dropped where the probes run out, which no later
 * doubling can undo.  Size the initial table for at least two frames' blocks (the CLI's 2^22 holds 65 536 blocks, a
 * 640x480 frame at 1 cm touches ~9 000). */
static int auto_grow_step(gsdf_ctx* c) {
    if (!c->auto_grow_max || !c->progress) return GSDF_OK;
    volatile unsigned long long* word = reinterpret_cast<volatile unsigned long long*>(c->progress + 4);
    if (c->grow_forget) {                                   /* a reset or a doubling: the counts so far describe another table */
        c->grow_forget = false;
        c->grow_seq = 0; c->grow_prev_seq = 0; c->grow_prev_cnt = 0; c->grow_rate = 0; c->grow_counts_seen = 0; c->grow_last_enq = 0;
        HIP_TRY(hipStreamSynchronize(c->stream));           /* no count kernel of the old numbering is in flight any more */
        *word = 0ull;
    }
    const unsigned int k = ++c->grow_seq;
    const size_t cap_blocks = c->n_slots / GSDF_BLOCK_VOX;
    auto look = [&](unsigned int& cnt, unsigned int& seen) {
        const unsigned long long w = *word;
        cnt = (unsigned int)(w & 0xFFFFFFFFull); seen = (unsigned int)(w >> 32);
        if (seen > c->grow_prev_seq) {                       /* a newer finished count: update the growth per frame */
            if (c->grow_counts_seen > 0) {
                const unsigned int d = cnt > c->grow_prev_cnt ? cnt - c->grow_prev_cnt : 0u, n = seen - c->grow_prev_seq;
                const unsigned int rate = (d + n - 1) / n;
                c->grow_rate = std::max(rate, c->grow_rate - c->grow_rate / 16u);
            }
            c->grow_prev_seq = seen; c->grow_prev_cnt = cnt; ++c->grow_counts_seen;
        }
    };
    unsigned int cnt = 0, seen = 0;
    look(cnt, seen);
    /* the count tagged `seen` was enqueued at the top of entry `seen`: it holds the fusions of the entries before it, except
     * one that a pipelined gsdf_update_dev still kept back => entries seen - 1 ... k - 1 are not in it */
    unsigned int uncovered = k - seen + 1;
    if (c->grow_counts_seen >= 2 && (int)uncovered > c->grow_max_lag + 1) {
        /* far ahead of the device: wait for it to come within grow_max_lag / 2 entries (it is working; nothing is drained) */
        /* ... but never for a count that was not enqueued: counts are tagged with the entry that queued them (every fourth
         * entry while the estimate is low), so `seen` cannot pass grow_last_enq (with a small GSDF_GROW_MAX_LAG the
         * old target k - seen <= lag / 2 was unreachable and the loop spun out its whole timeout on every entry) */
        const int target = std::max(c->grow_max_lag / 2, (int)(k - c->grow_last_enq));
        spin_until([&] { look(cnt, seen); return (int)(k - seen) <= target; }, 2.0);
        uncovered = k - seen + 1;
    }
    const bool safe = c->grow_counts_seen >= 2 && (int)uncovered <= c->grow_max_lag + 1 &&
                      ((size_t)cnt + 2u * (size_t)uncovered * std::max(c->grow_rate, 1u)) * 100u <= cap_blocks * 45u;
    if (!safe && c->capacity_log2 < c->auto_grow_max) {
        int rc = gsdf_flush_pending(c);                      /* a fusion kept back by the pipelined path counts too */
        if (rc) return rc;
        gsdf_enqueue_block_count(c, k);
        c->grow_last_enq = k;
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++c->grow_syncs;
        look(cnt, seen);
        if ((size_t)cnt * 100u > cap_blocks * 45u) {
            rc = gsdf_grow_impl(c, c->capacity_log2 + 1);    /* (sets grow_forget: the next entry starts the bookkeeping afresh) */
            if (rc) return rc;
        }
        return GSDF_OK;
    }
    /* far below the limit (estimate under 25 % of the entries) a count every fourth entry will do: the 3 us kernel and its
     * launch boundary are ~4 % of a tracked frame */
    const bool near = ((size_t)cnt + 2u * (size_t)uncovered * std::max(c->grow_rate, 1u)) * 100u > cap_blocks * 25u;
    if (near || k - c->grow_last_enq >= 4u) { gsdf_enqueue_block_count(c, k); c->grow_last_enq = k; }
    return GSDF_OK;
}

/* the tile statistics that belong to a set of normal planes (written by whatever computes the normals, read by the set's k_fuse) */
static uint32_t* stats_of(const gsdf_ctx* c, const float* nrm) {
    const size_t N = (size_t)c->W * c->H;
    const size_t set = (size_t)(nrm - c->frame.normals) / (3 * N);
    return c->frame.tile_stats + set * (size_t)c->fuse_blocks * 4;
}

/* one k_fuse launch: depth + its normal planes `nrm` (3 x N floats) -> the map.  next_depth (nullable): the launch's extra
 * workgroups compute the normals of that frame into next_nrm */
int launch_fuse(gsdf_ctx* c, const float* depth_dev, const float* nrm, const gsdf_pose_arg& pose, int use_dev_pose, int far_table,
                const float* next_depth, float* next_nrm, const gsdf_fuse_head* head = nullptr, unsigned int next_token = 0u) {
    const size_t N = (size_t)c->W * c->H;
    c->occ_dirty = true;                                      /* new blocks: the raycaster's filters are rebuilt when it next runs */
    c->fuse_launches += 1;
    c->far_table_launches += far_table ? 1 : 0;
    {
        prof_scope ps(c, 1);
        c->fuse_tag += 1;
        if (c->fuse_tag == 0) {                                /* wrapped: no stale flag may equal a new tag */
            c->fuse_tag = 1;
            HIP_TRY(hipMemsetAsync(c->frame.tile_flags, 0, (size_t)c->fuse_blocks * sizeof(unsigned int), c->stream));
        }
        gsdf_fuse_launch f;
        f.g = c->geom(); f.nc = c->ncache();
        f.depth = depth_dev; f.nx = nrm; f.ny = nrm + N; f.nz = nrm + 2 * N; f.tile_stats = stats_of(c, nrm);
        f.pose = pose; f.use_dev_pose = use_dev_pose;
        f.tab = c->tab; f.st = c->st; f.blk_counters = c->frame.blk_counters;
        f.deferred = c->frame.deferred; f.deferred_count = c->frame.deferred_count; f.deferred_cap = c->deferred_cap;
        f.tag = c->fuse_tag; f.tile_flags = c->frame.tile_flags; f.tile_order = c->frame.tile_order; f.ticket = c->frame.fuse_ticket;
        f.log_rows = c->frame.frame_log; f.max_rows = c->frame_log_cap; f.vis = c->map.vis; f.vis_words = c->vis_words;
        f.debug = c->debug & 0xFFFF;
        /* long deferred lists lately (the note lags by a launch or two: a hint, not a condition) */
        f.resolve_follows = c->progress && c->progress[2] > 8192u ? 1 : 0;
        f.host_note = c->progress ? c->progress.dev() + 2 : nullptr;
        /* many tiles did not fit the small LDS table lately (far geometry): the kernel with the larger one.  Like the note
         * above a hint that lags by a launch or two, never a condition for correctness; the caller read it once for the whole
         * frame entry (fuse_far_table) */
        f.far_table = far_table;
        f.head = head;
        f.next_depth = next_depth; f.next_nx = next_nrm; f.next_ny = next_nrm ? next_nrm + N : nullptr; f.next_nz = next_nrm ? next_nrm + 2 * N : nullptr;
        f.next_tile_stats = next_nrm ? stats_of(c, next_nrm) : nullptr; f.next_token = next_token;
        f.win = c->win;
        gsdf_launch_fuse(c->stream, f);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GSDF_ERR_HIP, std::string("fusion launch: ") + hipGetErrorString(e));
    return GSDF_OK;
}

/* normals (unless the frame's were computed beside its first tracker pass: normals_done) + fusion, in stream order */
int enqueue_fuse(gsdf_ctx* c, const float* depth_dev, const gsdf_pose_arg& pose, int use_dev_pose, int far_table, bool normals_done,
                 const gsdf_frame_route& route = gsdf_frame_route(), const gsdf_fuse_head* head = nullptr) {
    const size_t N = (size_t)c->W * c->H;
    /* tracked frames: set 2, filled beside the first tracker passes -- or the set the PREVIOUS frame's fusion filled in its
     * tail (gsdf_hint_next_depth_dev) */
    float* nrm = c->frame.normals + (size_t)route.fuse_set * 3 * N;
    const float* next_depth = route.hint;
    if (!normals_done) {
        nrm = c->frame.normals + (size_t)c->ahead.take_gt_set() * 3 * N;
        prof_scope ps(c, 0);
        gsdf_launch_normals(c->stream, c->geom(), c->win, c->ncache(), depth_dev, nrm, nrm + N, nrm + 2 * N, nullptr, nullptr, stats_of(c, nrm));
        next_depth = nullptr;
    }
    /* gsdf_hint_next_depth_dev: the launch's last workgroups compute NormalEstimator::compute of the NEXT frame into set
     * next_set -- if the launch's gate is open -- and leave next_token in st->nrm_token */
    float* next_nrm = next_depth ? c->frame.normals + (size_t)route.next_set * 3 * N : nullptr;
    return launch_fuse(c, depth_dev, nrm, pose, use_dev_pose, far_table, next_depth, next_nrm, head, route.next_token);
}

/* The end of a batch, seen from the host: *ended = 1 optimize() ended, 0 = the head of launch `last` ran and it has not ended.
 * Follows the progress word; if the device is far behind (2 s), waits for it properly. */
int batch_ended(gsdf_ctx* c, unsigned int serial, int last, int* ended) {
    *ended = -1;
    spin_until([&] {
        const gsdf_progress p = gsdf_progress_decode(c->progress[0]);
        if (p.serial == serial && (p.done || p.passes >= last)) *ended = p.done ? 1 : 0;
        return *ended >= 0;
    }, 2.0);
    if (*ended < 0) {
        gsdf_dev_state s;
        if (hipMemcpyAsync(&s, c->st, sizeof(s), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(GSDF_ERR_HIP, "tracking: device state read failed");
        *ended = s.done;
    }
    return GSDF_OK;
}

/* The frame's normals tiles ride in its first launches: nrm_split per cent in launch 0, nrm_split2 in launch 1, the rest
 * in launch 2.  Launch 1 always exists (it is at least the head of pass 0), launch 2 when the first batch has three
 * launches and optimize() may take two passes.  Next to the one tracker workgroup per CU a launch hides a share of the
 * tiles; launch 0 has no head and ends early, so it takes the smallest one.  Tile 0 (it resets the frame's deferred list)
 * stays in launch 0.
 * The tiles [*lo, *hi) of launch k, or false = none.  nl: tracker launches of the batch (of the first one: the fusion launch may
 * stand in for its last one, no riders there; later batches: 3); batch: its length as planned. */
bool normals_tile_split(int tiles, int k, int nl, int iters, int batch, int nrm_split, int nrm_split2, int* lo, int* hi) {
    if (k > 2) return false;
    const bool three = iters >= 2 && batch >= 3 && nl >= 3;
    const int b1 = nl >= 2 ? std::max(1, tiles * nrm_split / 100) : tiles;
    const int b2 = three ? std::min(tiles, std::max(b1, tiles * (nrm_split + nrm_split2) / 100)) : tiles;
    *lo = k == 0 ? 0 : k == 1 ? b1 : b2;
    *hi = k == 0 ? b1 : k == 1 ? b2 : tiles;
    return *hi > *lo && (k < 2 || three);
}

/* one frame on its way through enqueue_track */
struct track_frame {
    gsdf_ctx* c;
    const float* depth;                  /* the frame, or the compaction of its sampled pixels ... */
    gsdf_frame_geom g;                   /* ... and the pixel grid that goes with it */
    int iters;
    bool fuse_after;                     /* the Scan3D loop body: the frame's fusion, gated on the device, behind its passes */
    int far;                             /* fuse_far_table, read once for the frame */
    bool new_route;                      /* the round-6 steps are taken (see track_route) */
    gsdf_frame_route route;
    bool adaptive;
    gsdf_track_params tp;
    gsdf_normals_job nj;

    /* queues the frame's fusion (main_scan_3d.cpp:261-265), optionally with the closing head of optimize() in it */
    int queue_fusion(const gsdf_fuse_head* head = nullptr) const {
        gsdf_pose_arg unused;
        std::memset(&unused, 0, sizeof(unused));
        return enqueue_fuse(c, depth, unused, 1, far, iters > 0, route, head);
    }
};

/* optimize_sampled(depth, K, sampling) -- RigidPointOptimizer.cpp:62: the pixels (x, y) = (i * s, j * s).  They are
 * compacted into their own image (so that the pass kernel's coalesced pixel -> lane mapping serves them unchanged) and the
 * passes run on the grid of sampled pixels; k_track_pass<true> turns a grid index back into the pixel coordinate. */
int compact_sampled(track_frame& f, int sampling) {
    gsdf_ctx* c = f.c;
    if (f.fuse_after) return fail(GSDF_ERR_INVALID, "the frame loop tracks every pixel (RigidPointOptimizer.h:69-72)");
    const int Ws = (c->W + sampling - 1) / sampling, Hs = (c->H + sampling - 1) / sampling;
    if (!c->frame.depth_sampled) HIP_TRY(c->frame.depth_sampled.alloc((size_t)((c->W + 1) / 2) * ((c->H + 1) / 2)));
    gsdf_launch_subsample(c->stream, f.depth, c->W, c->H, sampling, c->frame.depth_sampled);
    f.depth = c->frame.depth_sampled;
    f.g.W = Ws; f.g.H = Hs;
    return GSDF_OK;
}

/* Which route the frame takes (gsdf_lookahead::consume has the look-ahead side of it).
 * Both round-6 steps -- the next frame's normals in the fusion's tail, the fusion launch standing in for the first batch's last
 * tracker launch -- pay where optimize() ends within the first batch and the fusion RUNS behind it.  Frames that converge late or
 * never come in stretches (the reference's tracker cycles on them), and there the extra workgroups only look at a closed gate
 * and the stand-in's head is followed by a head-less launch anyway (measured: -1 ... -2 % on the bench's default window): the
 * host takes the old route while the last tracked frame whose end it KNOWS needed more than the first batch (a hint for the
 * hint: the progress word of that frame's heads, read without waiting -- in such a stretch the host has just waited for it). */
void track_route(track_frame& f) {
    gsdf_ctx* c = f.c;
    const bool ahead_ok = f.fuse_after && !c->profiling && f.iters > 0;
    if (f.fuse_after && c->progress) c->ahead.note_progress(c->progress[0]);
    /* ... and not while the fusion uses the larger LDS table (far geometry): that instantiation with the normals role is at the
     * register limit and moves its records unpaired, with the head it spills -- both cost more than the step saves.  The choice is
     * read ONCE here and handed to every fusion launch of this frame: the word it comes from is written by the device while the
     * host runs, and a second read could pick the larger table for a launch that carries the normals role or the head. */
    f.far = fuse_far_table(c);
    f.new_route = ahead_ok && !c->ahead.prev_slow && !f.far;
    f.route = c->ahead.consume(f.depth, ahead_ok, f.new_route);
}

/* the per-launch parameters of the frame's passes and the job of the normals riders; takes the frame's serial */
void track_jobs(track_frame& f, float conv, float damping, int sampling) {
    gsdf_ctx* c = f.c;
    std::memset(&f.nj, 0, sizeof(f.nj));
    if (f.fuse_after) {                  /* the frame's normals ride along with its first passes (unless computed ahead: ride_token) */
        const size_t N = (size_t)c->W * c->H;
        f.nj.nc = c->ncache();
        f.nj.nx = c->frame.normals + (size_t)(3 * f.route.fuse_set) * N; f.nj.ny = f.nj.nx + N; f.nj.nz = f.nj.nx + 2 * N;    /* set 2, or the hinted one */
        f.nj.token = f.route.ride_token;
        f.nj.deferred_count = c->frame.deferred_count;
        f.nj.stats = stats_of(c, f.nj.nx);
        f.nj.r = c->win / 2; f.nj.ntx = 0;
        f.nj.tile_first = 0; f.nj.tile_count = 0;
    }
    gsdf_track_params& tp = f.tp;
    tp.max_passes = f.iters;
    tp.conv_sq = conv * conv;                                /* RigidOptimizer.h:72 */
    tp.damping = damping;
    c->track_serial = (c->track_serial + 1u) & 0xFFFFu;
    if (c->track_serial == 0) c->track_serial = 1;
    tp.serial = c->track_serial;
    f.adaptive = c->adaptive && c->progress;
    /* (the last launch index of this frame's first batch) */
    if (f.fuse_after) c->ahead.tracked(tp.serial, std::min(f.iters, (f.adaptive ? c->first_batch : f.iters + 1) - 1));
    tp.progress = f.adaptive ? c->progress.dev() : nullptr;
    tp.debug = c->debug >> 16;
    tp.n_track_blocks = c->track_blocks;
    tp.sampling = sampling;
    tp.head_done = 0;
}

/* optimize() as batches of per-pass launches, the host following the device between them (see enqueue_track) */
int track_batched(track_frame& f, int base) {
    gsdf_ctx* c = f.c;
    gsdf_track_params& tp = f.tp;
    const int iters = f.iters, tiles = gsdf_normals_tiles(c->W, c->H);
    int k = 0, batch_no = 0;
    int batch = f.adaptive ? c->first_batch : iters + 1;
    /* The frame's first fusion launch stands in for the LAST tracker launch of the first batch (k_fuse<.., HEAD>): that launch's
     * head -- for the usual frame the closing one of optimize() -- runs in workgroup 0 of the fusion launch, which every other
     * workgroup of it follows; a launch and a kernel boundary less per frame.  If optimize() has not ended with that head the
     * next batch starts with a tracker launch of the same index that skips its head (head_done).  Not in event-timed replays:
     * what bench.py quotes as k_fuse's duration is the fusion work alone. */
    const bool fuse_head = f.new_route && f.adaptive && c->fuse_head;
    bool headless = false;                                   /* the next launch's head was performed by a fusion launch */
    while (k <= iters) {
        const int last = std::min(iters, k + batch - 1);
        const bool stand_in = fuse_head && batch_no == 0 && last >= 1;
        const int nl = batch_no == 0 ? (stand_in ? last : last + 1) : 3;   /* tracker launches of the batch, as normals_tile_split counts them */
        for (; k <= last; ++k) {
            if (stand_in && k == last) continue;             /* its head is the fusion launch's */
            tp.pass_index = k;
            tp.head_done = headless ? 1 : 0;
            headless = false;
            tp.rot = c->track_rot;
            c->track_rot = (c->track_rot + 1u) % 3u;          /* kept in [0, 3): no discontinuity at wrap-around */
            const gsdf_normals_job* job = nullptr;
            int lo = 0, hi = 0;
            if (f.fuse_after && normals_tile_split(tiles, k, nl, iters, batch, c->nrm_split, c->nrm_split2, &lo, &hi)) {
                f.nj.tile_first = lo; f.nj.tile_count = hi - lo; job = &f.nj;
            }
            prof_scope ps(c, 2);
            gsdf_launch_track_pass(c->stream, f.g, f.depth, c->tab, c->st, c->frame.partials, c->track_blocks, tp, job, base);
        }
        /* The fusion is queued behind the FIRST batch unseen (the usual frame ends there and must not wait for the host) and
         * behind the last one (nothing follows it).  Behind the batches in between it would nearly always be a gated launch
         * that finds optimize() still running -- 3 us each, 3 per frame that never converges -- so there it is queued only
         * once the progress word says that optimize() has ended (the frame that converges late pays the host's look). */
        bool fuse_queued = false;
        if (f.fuse_after && (batch_no == 0 || last == iters || !c->lazy_fuse)) {
            gsdf_fuse_head hd;
            std::memset(&hd, 0, sizeof(hd));
            if (stand_in) {
                hd.k = last;
                hd.rot_prev = (c->track_rot + 2u) % 3u;      /* the buffer the last launch issued (pass last - 1) accumulated into */
                hd.conv_sq = tp.conv_sq; hd.damping = tp.damping; hd.max_passes = tp.max_passes;
                hd.serial = tp.serial; hd.progress = tp.progress; hd.rows = c->frame.partials; hd.debug = tp.debug;
            }
            const int rc = f.queue_fusion(stand_in ? &hd : nullptr);
            if (rc) return rc;
            fuse_queued = true;
        }
        ++batch_no;
        if (last == iters) break;                            /* the head-only launch always ends optimize() */
        int ended = 0;
        const int rc = batch_ended(c, tp.serial, last, &ended);
        if (rc) return rc;
        if (ended) return f.fuse_after && !fuse_queued ? f.queue_fusion() : GSDF_OK;
        if (stand_in) { k = last; headless = true; }         /* launch `last` comes now, without the head the fusion launch performed */
        batch = c->next_batch;
    }
    return GSDF_OK;
}

/* RigidPointOptimizer::optimize_sampled as a chain of per-pass launches.  The convergence test, the pose update
 * and the done/converged flags live on the device; launches after `done` return immediately.  Launch k > 0
 * first finishes pass k-1 (reduce, solve, update: the "head"), launch `iters` is head-only.
 *
 * The host issues the launches in BATCHES and never waits in the common case: the first batch covers the usual
 * 3-4 passes; behind every batch it queues the frame's fusion (fuse_after: the Scan3D loop body), which is gated
 * on the device by done && converged, so it runs exactly once -- behind the batch in which optimize() ended.
 * While that batch (and the fusion) execute, the host follows one pinned word the pass heads write (serial,
 * done, passes) and only issues a further batch if the optimisation has not ended by the last head of the
 * previous one.  Correctness never depends on what the host sees: a late or lost observation only costs empty
 * launches. */
int enqueue_track(gsdf_ctx* c, const float* depth_dev, int iters, float conv, float damping, bool fuse_after, int sampling = 1) {
    track_frame f;
    f.c = c; f.depth = depth_dev; f.g = c->geom(); f.iters = iters; f.fuse_after = fuse_after;
    if (sampling > 1) {
        const int rc = compact_sampled(f, sampling);
        if (rc) return rc;
    }
    track_route(f);
    if (iters <= 0) {
        gsdf_launch_track_none(c->stream, c->st);
        return fuse_after ? f.queue_fusion() : GSDF_OK;
    }
    if (iters > 0x7FFF) return fail(GSDF_ERR_INVALID, "num_iterations must be <= 32767");
    track_jobs(f, conv, damping, sampling);
    const int base = c->map_type == GSDF_MAP_BASE;
    const int rc = track_batched(f, base);
    if (rc) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GSDF_ERR_HIP, std::string("tracking launch: ") + hipGetErrorString(e));
    return GSDF_OK;
}

/* alloc(count), and the zeroes queued on the stream */
template <class T>
hipError_t alloc_zeroed(gsdf_dev<T>& b, size_t count, hipStream_t s) {
    const hipError_t e = b.alloc(count);
    return e != hipSuccess ? e : hipMemsetAsync(b, 0, b.bytes(), s);
}

int read_state(gsdf_ctx* c, gsdf_dev_state* out) {
    HIP_TRY(hipMemcpyAsync(out, c->st, sizeof(gsdf_dev_state), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

} // namespace

/* launches the GT-pose fusion that waits for its successor (gsdf_update_dev), if any */
int gsdf_flush_pending(gsdf_ctx* c) {
    if (!c || !c->ahead.pending.valid) return GSDF_OK;
    c->ahead.release();
    if (hipSetDevice(c->device) != hipSuccess) return fail(GSDF_ERR_HIP, "hipSetDevice");
    const size_t N = (size_t)c->W * c->H;
    const gsdf_lookahead::pending_fuse& p = c->ahead.pending;
    return launch_fuse(c, p.depth, c->frame.normals + (size_t)p.set * 3 * N, p.pose, 0, fuse_far_table(c), nullptr, nullptr);
}
#define GSDF_FLUSH(c) do { if ((c) && (c)->ahead.pending.valid) { const int rc_ = gsdf_flush_pending(c); if (rc_) return rc_; } } while (0)
/* The staging entries (gsdf_dev_upload*) write device memory the caller names.  A GT-pose fusion that still waits for its
 * successor reads its depth image when it is LAUNCHED, so a copy into that image has to come behind the launch: the pattern
 * upload(buf) -> update_dev(buf) -> upload(buf) -> update_dev(buf) on ONE staging buffer is correct by stream order only if
 * the waiting fusion is launched before the second copy is queued.  Copies elsewhere leave the pipelining alone. */
static int flush_if_overlaps(gsdf_ctx* c, const void* dst, int64_t bytes) {
    /* (a copy into a frame whose normals were computed ahead (gsdf_hint_next_depth_dev), or that is hinted: those belong to the
     * old contents -- forgotten, the frame's own tracker launches compute its normals then) */
    if (c && c->ahead.range_changes(dst, (size_t)std::max<int64_t>(bytes, 0), c->frame_bytes())) return gsdf_flush_pending(c);
    return GSDF_OK;
}

extern "C" {

const char* gsdf_last_error(void) { return g_gsdf_err.c_str(); }
#ifdef GSDF_EXPERIMENTS
/* Test / measurement build only (libgsdf_test.so, make EXPERIMENTS=1); not part of include/gsdf.h and absent from the
 * production library.  Per context.  Bits 0-15 go to k_fuse: 4 every tile defers, 256 single band, 512 four bands,
 * 8192 every hand-off wait expires at once, 1024 / 2048 pin the larger / smaller LDS table, 1/2/16/32/64/128/4096 measurement
 * switches of tools/; bits 16+ go to the tracker. */
#define GSDF_TRACE_WG 8192
#define GSDF_TRACE_COLS 16
int gsdf_debug_flags(gsdf_ctx* c, int flags) {
    GSDF_FLUSH(c);
    if (!c) return GSDF_ERR_INVALID;
    c->debug = flags;
    if (flags & 64) {                                  /* k_fuse trace: GSDF_TRACE_COLS time stamps per workgroup, pointer in dbg[23] */
        if (hipStreamSynchronize(c->stream) != hipSuccess) return GSDF_ERR_HIP;
        if (!c->trace && c->trace.alloc((size_t)GSDF_TRACE_WG * GSDF_TRACE_COLS) != hipSuccess) return GSDF_ERR_HIP;
        if (hipMemset(c->trace, 0, (size_t)GSDF_TRACE_WG * GSDF_TRACE_COLS * 8) != hipSuccess) return GSDF_ERR_HIP;
        const unsigned long long ptr = (unsigned long long)(uintptr_t)c->trace.get();
        if (hipMemcpy(&c->st->dbg[23], &ptr, 8, hipMemcpyHostToDevice) != hipSuccess) return GSDF_ERR_HIP;
    }
    return GSDF_OK;
}
/* the trace of the last k_fuse launch: n_wg rows of GSDF_TRACE_COLS (16) values */
int gsdf_debug_trace(gsdf_ctx* c, unsigned long long* out, int n_wg) {
    GSDF_FLUSH(c);
    if (!c || !out || !c->trace || n_wg > GSDF_TRACE_WG) return GSDF_ERR_INVALID;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return GSDF_ERR_HIP;
    if (hipMemcpy(out, c->trace, (size_t)n_wg * GSDF_TRACE_COLS * 8, hipMemcpyDeviceToHost) != hipSuccess) return GSDF_ERR_HIP;
    return GSDF_OK;
}
/* the raycaster's per-workgroup rows (8 values each, see gsdf_launch_raycast), tools/raycast_bench.py */
int gsdf_debug_raycast_rows(gsdf_ctx* c, unsigned long long* out, int n_rows) {
    GSDF_FLUSH(c);
    if (!c || !out || !c->rc_counts || (size_t)n_rows > c->rc_counts.count() / 8) return GSDF_ERR_INVALID;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return GSDF_ERR_HIP;
    if (hipMemcpy(out, c->rc_counts, (size_t)n_rows * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return GSDF_ERR_HIP;
    return GSDF_OK;
}
/* experiments with the launch order of the fusion tiles (tools/fuse_order.py): the per-tile counter rows (last n_upd, last
 * n_valid, totals) and a caller-made order (same encoding as gsdf_fuse_tile_order; n = workgroups) */
int gsdf_debug_tile_counters(gsdf_ctx* c, unsigned long long* out, int n_rows) {
    GSDF_FLUSH(c);
    if (!c || !out || !c->frame.blk_counters || n_rows > c->fuse_blocks) return GSDF_ERR_INVALID;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return GSDF_ERR_HIP;
    if (hipMemcpy(out, c->frame.blk_counters, (size_t)n_rows * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) return GSDF_ERR_HIP;
    return GSDF_OK;
}
int gsdf_debug_set_tile_order(gsdf_ctx* c, const uint32_t* order, int n) {
    GSDF_FLUSH(c);
    if (!c || !order || !c->frame.tile_order || n != c->fuse_blocks) return GSDF_ERR_INVALID;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return GSDF_ERR_HIP;
    if (hipMemcpy(c->frame.tile_order, order, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) return GSDF_ERR_HIP;
    return GSDF_OK;
}
int gsdf_debug_get_tile_order(gsdf_ctx* c, uint32_t* order, int* n) {
    if (!c || !order || !n || !c->frame.tile_order) return GSDF_ERR_INVALID;
    if (hipMemcpy(order, c->frame.tile_order, (size_t)c->fuse_blocks * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return GSDF_ERR_HIP;
    *n = c->fuse_blocks;
    return GSDF_OK;
}
int gsdf_debug_read(gsdf_ctx* c, unsigned long long out[24]) {
    GSDF_FLUSH(c);
    if (!c || !out) return GSDF_ERR_INVALID;
    if (hipStreamSynchronize(c->stream) != hipSuccess) return GSDF_ERR_HIP;
    gsdf_dev_state h;
    if (hipMemcpy(&h, c->st, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return GSDF_ERR_HIP;
    for (int i = 0; i < 24; ++i) out[i] = h.dbg[i];
    return GSDF_OK;
}
/* normals_tile_split as enqueue_track uses it, for the tests: no context, no device.  1 = launch k computes the tiles [*lo, *hi) */
int gsdf_debug_normals_tile_split(int tiles, int k, int launches, int iters, int batch, int nrm_split, int nrm_split2, int* lo, int* hi) {
    return lo && hi && normals_tile_split(tiles, k, launches, iters, batch, nrm_split, nrm_split2, lo, hi) ? 1 : 0;
}
/* The nth allocation the owning types (gsdf_dev.h) make from now on fails once with hipErrorOutOfMemory, without calling the
 * runtime; 0 disarms.  Returns the owned allocations made since the previous call.  Process-wide. */
int gsdf_debug_fail_alloc(int nth) {
    const int made = g_gsdf_alloc_count;
    g_gsdf_alloc_count = 0;
    g_gsdf_alloc_fail_at = nth > 0 ? nth : 0;
    return made;
}
const char* gsdf_version(void) { return "gsdf-mi355x 0.2 (gfx950) +experiments"; }
#else
const char* gsdf_version(void) { return "gsdf-mi355x 0.2 (gfx950)"; }
#endif

static int create_impl(gsdf_ctx** out, float voxel_size, float trunc_dist, int capacity_log2, int device, bool other_queue);
int gsdf_create(gsdf_ctx** out, float voxel_size, float trunc_dist, int capacity_log2, int device) {
    return create_impl(out, voxel_size, trunc_dist, capacity_log2, device, false);
}
/* n contexts for n frame shards on ONE device (gsdf_merge_from adds them up): their streams are created with the device's
 * HIGHEST stream priority.  The HIP runtime keeps one pool of hardware queues per priority and hands a new stream the
 * least-used queue of its pool; the normal pool is shared with every other stream of the process (the contexts' copy streams,
 * PyTorch's, ...), and two streams that land in one queue do not overlap -- measured inside bench.py: two normal-priority
 * contexts fused 24 500 frames/s where two on separate queues reach 31 600.  Nothing else uses the high-priority pool, so up to
 * four shard contexts get a queue each, at EQUAL priority. */
int gsdf_create_shards(gsdf_ctx** out, int n, float voxel_size, float trunc_dist, int capacity_log2, int device) {
    if (!out || n < 1 || n > 4) return fail(GSDF_ERR_INVALID, "gsdf_create_shards: 1..4 contexts (one hardware queue each)");
    for (int i = 0; i < n; ++i) out[i] = nullptr;
    for (int i = 0; i < n; ++i) {
        const int rc = create_impl(&out[i], voxel_size, trunc_dist, capacity_log2, device, true);
        if (rc) { for (int j = 0; j < i; ++j) { gsdf_destroy(out[j]); out[j] = nullptr; } return rc; }
    }
    return GSDF_OK;
}
static int create_impl(gsdf_ctx** out, float voxel_size, float trunc_dist, int capacity_log2, int device, bool other_queue) {
    if (!out) return fail(GSDF_ERR_INVALID, "out == NULL");
    *out = nullptr;
    if (!(voxel_size > 0.f) || !(trunc_dist > 0.f)) return fail(GSDF_ERR_INVALID, "voxel_size and trunc_dist must be > 0");
    if (capacity_log2 < 10 || capacity_log2 > 30) return fail(GSDF_ERR_INVALID, "capacity_log2 must be in [10, 30]");
    if (!(trunc_dist < 2.f)) return fail(GSDF_ERR_INVALID, "trunc_dist must be < 2 m (fixed-point range of the fusion kernel's accumulators)");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        return fail(GSDF_ERR_NO_DEVICE, "no HIP device visible: libgsdf has no CPU fallback");
    }
    if (device < 0 || device >= n_dev) return fail(GSDF_ERR_INVALID, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device));
    gsdf_ctx* c = new gsdf_ctx();
    c->device = device;
    c->voxel_size = voxel_size;
    c->voxel_size_inv = (float)(1. / voxel_size);            /* MapGradPixelSdf.h:99-103 */
    c->T = trunc_dist;
    c->inv_T = (float)(1. / trunc_dist);                     /* Sdf.h:103-107 */
    c->factor = (int)std::floor(c->T / c->voxel_size);       /* MapGradPixelSdf.cpp:79 */
    c->capacity_log2 = capacity_log2;
    c->n_slots = (size_t)1 << capacity_log2;
    hipError_t e;
    int prio_least = 0, prio_greatest = 0;
    if (other_queue) {
        /* the separate-queue guarantee of gsdf_create_shards rests on a priority pool of its own: without one it is
         * not claimed -- an error, not a silent default-priority stream */
        if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess || prio_greatest == prio_least) {
            (void)hipGetLastError();
            delete c;
            return fail(GSDF_ERR_HIP, "gsdf_create_shards: the device offers no stream priority range, so separate hardware queues cannot be guaranteed (use gsdf_create)");
        }
    }
    if ((e = (other_queue ? hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_greatest)
                          : hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking))) != hipSuccess ||
        (e = c->map.alloc(c->n_slots, 0)) != hipSuccess || (e = c->st.alloc(1)) != hipSuccess || (e = c->counter.alloc(1)) != hipSuccess ||
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) {
        std::string m = std::string("gsdf_create: ") + hipGetErrorString(e);
        gsdf_destroy(c);
        return fail(GSDF_ERR_HIP, m);
    }
    {
        const char* env = getenv("GSDF_DEFER");                    /* 0: every gsdf_update_dev launches its normals and its fusion at once */
        if (env) c->defer = atoi(env);
    }
    c->tab = c->map.table(c->n_slots);
    {
        if (c->progress.alloc(16) != hipSuccess) (void)hipGetLastError();   /* optional: without them no adaptive batches, no auto-grow */
        const char* env = getenv("GSDF_ADAPTIVE");
        if (env) c->adaptive = atoi(env);
        if ((env = getenv("GSDF_FIRST_BATCH")) && atoi(env) >= 2) c->first_batch = atoi(env);
        if ((env = getenv("GSDF_FUSE_HEAD"))) c->fuse_head = atoi(env) != 0;   /* 0: the first batch's last launch is a tracker launch again */
        if ((env = getenv("GSDF_NRM_SPLIT"))) {            /* experiments: "a" or "a,b" = per cent of the normals tiles in launch 0 (and 1) */
            int a = -1, b = -1;
            const int n = sscanf(env, "%d,%d", &a, &b);
            if (n >= 1 && a >= 0 && a <= 100) { c->nrm_split = a; c->nrm_split2 = 100 - a; }
            if (n >= 2 && b >= 0 && a + b <= 100) c->nrm_split2 = b;
        }
        if ((env = getenv("GSDF_NEXT_BATCH")) && atoi(env) >= 1) c->next_batch = atoi(env);
        if ((env = getenv("GSDF_LAZY_FUSE"))) c->lazy_fuse = atoi(env);
        if ((env = getenv("GSDF_FAR_TABLE"))) c->far_table = atoi(env);       /* experiments: 0 / 1 pin the fusion kernel's table size */
        /* auto-grow: entries the host may be ahead of the newest count.  Counts are queued every fourth entry while the load
         * is low, so a lag below 8 could never be "safe" between two of them: smaller values are raised to 8 */
        if ((env = getenv("GSDF_GROW_MAX_LAG")) && atoi(env) >= 1) c->grow_max_lag = std::max(8, atoi(env));
    }
    int rc = gsdf_reset(c);
    if (rc != GSDF_OK) { gsdf_destroy(c); return rc; }
    *out = c;
    return GSDF_OK;
}

void gsdf_destroy(gsdf_ctx* c) {
    if (!c) return;
    (void)gsdf_flush_pending(c);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);    /* the context's buffers go with it: nothing may still run on them */
    prof_collect(c);
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    for (auto& u : c->uploads) { (void)hipEventSynchronize(u.second); (void)hipEventDestroy(u.second); }
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    for (hipEvent_t e : c->mark_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->upload_pool) (void)hipEventDestroy(e);
    for (auto& m : c->marks) (void)hipEventDestroy(m.second);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int gsdf_reset(gsdf_ctx* c) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    c->ahead.forget_all();                                 /* a fusion that was never launched is dropped with the map; gsdf_hint_next_depth_dev: a new scan starts without them */
    c->fuse_launches = 0; c->far_table_launches = 0;
    if (c->frame.deferred_count) HIP_TRY(hipMemsetAsync(c->frame.deferred_count, 0, sizeof(unsigned int), c->stream));
    gsdf_launch_table_clear(c->stream, c->tab, c->n_slots);
    if (c->map.vis) HIP_TRY(hipMemsetAsync(c->map.vis, 0, c->n_slots * (size_t)c->vis_words * sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemsetAsync(c->st, 0, sizeof(gsdf_dev_state), c->stream));
    if (c->trace) {                                          /* test build: the memset cleared the trace pointer kept in dbg[23] */
        const unsigned long long ptr = (unsigned long long)(uintptr_t)c->trace.get();
        HIP_TRY(hipMemcpyAsync(&c->st->dbg[23], &ptr, 8, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));            /* `ptr` is a stack variable */
    }
    const float ident[7] = { 0, 0, 0, 0, 0, 0, 1 };          /* pose_ = SE3() -- RigidOptimizer.h:64 */
    gsdf_launch_set_pose(c->stream, c->st, nullptr, ident);
    if (c->frame.blk_counters)
        HIP_TRY(hipMemsetAsync(c->frame.blk_counters, 0, (size_t)c->fuse_blocks * 4 * sizeof(unsigned long long), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->merged = false;
    c->color.drop();                                         /* the ColorUpsampler snapshot describes the old map */
    c->grow_forget = true;                                   /* auto-grow's block counts describe the old map (a grown table keeps its size) */
    c->occ_dirty = false;                                    /* the table clear zeroed the filters as well */
    c->sel_state = GSDF_SEL_NONE;                            /* the selection goes with the map */
    return GSDF_OK;
}

int gsdf_set_map_type(gsdf_ctx* c, int type) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    if (type != GSDF_MAP_GRAD && type != GSDF_MAP_BASE) return fail(GSDF_ERR_INVALID, "unknown map type");
    if (type == c->map_type) return GSDF_OK;
    int64_t n = 0;
    const int rc = gsdf_count(c, &n);
    if (rc) return rc;
    if (n != 0) return fail(GSDF_ERR_INVALID, "the map type can only change while the map is empty (gsdf_reset first)");
    c->map_type = type;
    return GSDF_OK;
}

int gsdf_get_map_type(gsdf_ctx* c, int* type) {
    if (!c || !type) return fail(GSDF_ERR_INVALID, "null argument");
    *type = c->map_type;
    return GSDF_OK;
}

int gsdf_set_auto_grow(gsdf_ctx* c, int max_capacity_log2) {
    GSDF_FLUSH(c);
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    if (max_capacity_log2 != 0 && (max_capacity_log2 < c->capacity_log2 || max_capacity_log2 > 30))
        return fail(GSDF_ERR_INVALID, "gsdf_set_auto_grow: 0 (off) or a capacity_log2 between the present one and 30");
    HIP_TRY(hipSetDevice(c->device));
    if (max_capacity_log2 && !c->grow_scratch) {
        HIP_TRY(c->grow_scratch.alloc(2));
        HIP_TRY(hipMemsetAsync(c->grow_scratch, 0, 2 * sizeof(unsigned int), c->stream));
    }
    if (max_capacity_log2 && !c->progress) return fail(GSDF_ERR_HIP, "gsdf_set_auto_grow: no pinned progress words on this context");
    c->auto_grow_max = max_capacity_log2;
    c->grow_forget = true;
    return GSDF_OK;
}

int gsdf_capacity(gsdf_ctx* c, int* capacity_log2) {
    if (!c || !capacity_log2) return fail(GSDF_ERR_INVALID, "null argument");
    *capacity_log2 = c->capacity_log2;
    return GSDF_OK;
}

int gsdf_set_zrange(gsdf_ctx* c, float zmin, float zmax) {
    GSDF_FLUSH(c);
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    if (!std::isfinite(zmin) || !std::isfinite(zmax) || !(zmax > zmin))
        return fail(GSDF_ERR_INVALID, "gsdf_set_zrange: finite zmin < zmax required");
    if (zmin != c->zmin || zmax != c->zmax) {
        /* the tile statistics of normals computed ahead (gsdf_hint_next_depth_dev) were taken under the old range: a tile with no
         * pixel inside it would count no valid pixel and never be walked.  Forget them; the next frame computes its own. */
        c->ahead.forget_frames();
    }
    c->zmin = zmin; c->zmax = zmax;
    return GSDF_OK;
}

int gsdf_normals_init(gsdf_ctx* c, int W, int H, const float K[9], int win) {
    GSDF_FLUSH(c);
    if (!c || !K) return fail(GSDF_ERR_INVALID, "null argument");
    if (W <= 0 || H <= 0 || win <= 0 || !(win & 1) || win / 2 > 7)
        return fail(GSDF_ERR_INVALID, "W,H > 0 and odd window <= 15 required");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->frame = gsdf_frame_bufs();                            /* the old frame goes first (peak memory); until the commit below there is none */
    c->ahead.forget_frames();
    gsdf_frame_bufs f;
    const size_t N = (size_t)W * H;
    HIP_TRY(f.planes.alloc(11 * N));
    HIP_TRY(f.depth_stage.alloc(N));
    /* three sets of 3 planes: sets 0 / 1 alternate between GT-pose fusions (the normals of frame i + 1 are computed on a second
     * stream while frame i is being fused), set 2 belongs to the main stream (tracked frames, gsdf_normals_compute) */
    HIP_TRY(f.normals.alloc(3 * 3 * N));
    /* tracker grid: a multiple of the 256 CUs when the frame is large enough, 1-4 pixels per lane */
    const int track_blocks = N >= (size_t)1 << 20 ? 2 * GSDF_TRACK_MAXBLK : N >= (size_t)1 << 18 ? GSDF_TRACK_MAXBLK
                                                  : (int)std::max<size_t>(1, (N + 511) / 512);
    HIP_TRY(alloc_zeroed(f.partials, (size_t)3 * GSDF_TRACK_ROWSET, c->stream));
    const int fuse_blocks = gsdf_fuse_grid_blocks(W, H);
    /* per set of normal planes: the statistics of the frame's fusion tiles (depth range, valid pixels), written with the normals */
    HIP_TRY(alloc_zeroed(f.tile_stats, (size_t)3 * fuse_blocks * 4, c->stream));
    HIP_TRY(alloc_zeroed(f.blk_counters, (size_t)fuse_blocks * 4, c->stream));
    HIP_TRY(alloc_zeroed(f.tile_flags, (size_t)fuse_blocks, c->stream));
    {
        std::vector<uint32_t> order((size_t)fuse_blocks);
        gsdf_fuse_tile_order(W, H, order.data());
        HIP_TRY(f.tile_order.alloc(order.size()));
        HIP_TRY(hipMemcpy(f.tile_order, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    /* deferred list: contributions of near tiles and LDS overflow; bounded by the samples of a frame */
    const unsigned int deferred_cap = (unsigned int)std::min<size_t>((size_t)1 << 26, std::max<size_t>((size_t)1 << 18,
                                                                     N * (size_t)(2 * c->factor + 1)));   /* every sample of a frame */
    HIP_TRY(f.deferred.alloc(deferred_cap));
    HIP_TRY(alloc_zeroed(f.deferred_count, 1, c->stream));
    HIP_TRY(alloc_zeroed(f.fuse_ticket, 2, c->stream));
    const long long frame_log_cap = 1 << 16;
    HIP_TRY(f.frame_log.alloc((size_t)frame_log_cap * 10));
    {
        gsdf_dev<void> scratch;                              /* the row sums of the six moment planes, in double */
        HIP_TRY(scratch.alloc(gsdf_normals_cache_scratch_bytes(W, H)));
        gsdf_launch_normals_cache(c->stream, W, H, K, win, f.planes, scratch.as<double>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    /* the commit: only a complete frame, with the numbers that describe it, reaches the context */
    c->frame = std::move(f);
    c->W = W; c->H = H; c->win = win;
    std::memcpy(c->K, K, 9 * sizeof(float));
    c->track_blocks = track_blocks; c->track_rot = 0;
    c->fuse_blocks = fuse_blocks; c->deferred_cap = deferred_cap; c->frame_log_cap = frame_log_cap;
    return GSDF_OK;
}

int gsdf_normals_cache(gsdf_ctx* c, float* planes11_host) {
    GSDF_FLUSH(c);
    int rc = require_frame(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(planes11_host, c->frame.planes, 11 * (size_t)c->W * c->H * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_normals_compute(gsdf_ctx* c, const float* depth_host, float* nx, float* ny, float* nz) {
    GSDF_FLUSH(c);
    int rc = require_frame(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)c->W * c->H;
    HIP_TRY(hipMemcpyAsync(c->frame.depth_stage, depth_host, N * sizeof(float), hipMemcpyHostToDevice, c->stream));
    float* set2 = c->frame.normals + 6 * N;
    gsdf_launch_normals(c->stream, c->geom(), c->win, c->ncache(), c->frame.depth_stage, set2, set2 + N, set2 + 2 * N, nullptr, nullptr, stats_of(c, set2));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(nx, set2, N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(ny, set2 + N, N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(nz, set2 + 2 * N, N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_update_dev(gsdf_ctx* c, const float* depth_dev, const float R[9], const float t[3]) {
    int rc = require_frame(c);
    if (rc) return rc;
    if (!depth_dev || !R || !t) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = auto_grow_step(c))) return rc;
    gsdf_pose_arg pose;
    std::memcpy(pose.R, R, sizeof(pose.R));
    std::memcpy(pose.t, t, sizeof(pose.t));
    if (!c->defer || c->profiling) {                       /* event-timed replays: normals and fusion as two launches, in order */
        int rc = gsdf_flush_pending(c);
        if (rc) return rc;
        return enqueue_fuse(c, depth_dev, pose, 0, fuse_far_table(c), false);
    }
    /* MapGradPixelSdf.cpp:60: the normals of a frame depend on its depth only.  A run of GT-pose fusions (the branch
     * main_scan_3d.cpp:250-254; frame-sharded fusion) is pipelined by ONE call: the k_fuse of frame i is launched when frame
     * i + 1 arrives, and that launch's last workgroups compute the normals of frame i + 1 -- in the tail of the fusion,
     * where two thirds of the CUs idle, instead of as a launch of their own in front of the next fusion (10 us + a gap on
     * the critical path of every frame before).  Anything else the caller does with the context launches the waiting
     * fusion first (gsdf_flush_pending at the top of every other entry), so the deferral is invisible except in time.
     * The two sets of normal planes alternate. */
    const size_t N = (size_t)c->W * c->H;
    const int set = c->ahead.take_gt_set();                /* sets 0 / 1 are this path's: a hinted tracked frame's normals are gone */
    float* nrm = c->frame.normals + (size_t)set * 3 * N;
    if (!c->ahead.pending.valid) {
        gsdf_launch_normals(c->stream, c->geom(), c->win, c->ncache(), depth_dev, nrm, nrm + N, nrm + 2 * N, nullptr, nullptr, stats_of(c, nrm));
        HIP_TRY(hipGetLastError());
    } else {
        const gsdf_lookahead::pending_fuse& p = c->ahead.pending;
        int rc = launch_fuse(c, p.depth, c->frame.normals + (size_t)p.set * 3 * N, p.pose, 0, fuse_far_table(c), depth_dev, nrm);
        c->ahead.release();
        if (rc) return rc;
    }
    c->ahead.hold(depth_dev, pose, set);
    return GSDF_OK;
}

int gsdf_update(gsdf_ctx* c, const float* depth_host, const float R[9], const float t[3]) {
    GSDF_FLUSH(c);
    int rc = require_frame(c);
    if (rc) return rc;
    if (!depth_host) return fail(GSDF_ERR_INVALID, "null depth");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->frame.depth_stage, depth_host, (size_t)c->W * c->H * sizeof(float), hipMemcpyHostToDevice, c->stream));
    rc = gsdf_update_dev(c, c->frame.depth_stage, R, t);
    if (rc) return rc;
    return gsdf_sync(c);
}

int gsdf_set_pose(gsdf_ctx* c, const float pose7[7]) {
    GSDF_FLUSH(c);
    if (!c || !pose7) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    gsdf_launch_set_pose(c->stream, c->st, nullptr, pose7);
    HIP_TRY(hipGetLastError());
    return GSDF_OK;
}

int gsdf_get_pose(gsdf_ctx* c, float pose7[7]) {
    GSDF_FLUSH(c);
    if (!c || !pose7) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev_state s;
    int rc = read_state(c, &s);
    if (rc) return rc;
    std::memcpy(pose7, s.pose7, 7 * sizeof(float));
    return GSDF_OK;
}

int gsdf_track(gsdf_ctx* c, const float* depth_host, const float K[9], float pose7[7], int num_iterations,
               float conv_threshold, float damping, int* converged, int* passes) {
    return gsdf_track_sampled(c, depth_host, K, pose7, num_iterations, conv_threshold, damping, 1, converged, passes);
}

int gsdf_track_sampled(gsdf_ctx* c, const float* depth_host, const float K[9], float pose7[7], int num_iterations,
                       float conv_threshold, float damping, int sampling, int* converged, int* passes) {
    GSDF_FLUSH(c);
    int rc = require_frame(c);
    if (rc) return rc;
    if (!depth_host || !K || !pose7) return fail(GSDF_ERR_INVALID, "null argument");
    /* size_t sampling of the reference: 0 never ends its loops (y += 0); a stride beyond the image is the single pixel (0, 0) */
    if (sampling < 1) return fail(GSDF_ERR_INVALID, "sampling must be >= 1");
    if (sampling > std::max(c->W, c->H)) sampling = std::max(c->W, c->H);
    if (std::memcmp(K, c->K, 9 * sizeof(float)) != 0)
        return fail(GSDF_ERR_INVALID, "K differs from the intrinsics given to gsdf_normals_init");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(c->frame.depth_stage, depth_host, (size_t)c->W * c->H * sizeof(float), hipMemcpyHostToDevice, c->stream));
    gsdf_launch_set_pose(c->stream, c->st, nullptr, pose7);
    rc = enqueue_track(c, c->frame.depth_stage, num_iterations, conv_threshold, damping, false, sampling);
    if (rc) return rc;
    gsdf_dev_state s;
    rc = read_state(c, &s);
    if (rc) return rc;
    std::memcpy(pose7, s.pose7, 7 * sizeof(float));
    if (converged) *converged = s.converged;
    if (passes) *passes = s.passes;
    return status_to_code(s.status);
}

int gsdf_hint_next_depth_dev(gsdf_ctx* c, const float* next_depth_dev) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    c->ahead.hint(next_depth_dev);                       /* nullptr withdraws it; no device work, no flush */
    return GSDF_OK;
}

int gsdf_track_and_fuse_ahead_dev(gsdf_ctx* c, const float* depth_dev, const float* next_depth_dev, const float K[9],
                                  int num_iterations, float conv_threshold, float damping) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    c->ahead.hint(next_depth_dev);
    return gsdf_track_and_fuse_dev(c, depth_dev, K, num_iterations, conv_threshold, damping);
}

int gsdf_track_and_fuse_dev(gsdf_ctx* c, const float* depth_dev, const float K[9], int num_iterations,
                            float conv_threshold, float damping) {
    GSDF_FLUSH(c);
    int rc = require_frame(c);
    if (rc) return rc;
    if (!depth_dev || !K) return fail(GSDF_ERR_INVALID, "null argument");
    if (std::memcmp(K, c->K, 9 * sizeof(float)) != 0)
        return fail(GSDF_ERR_INVALID, "K differs from the intrinsics given to gsdf_normals_init");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = auto_grow_step(c))) return rc;
    rc = enqueue_track(c, depth_dev, num_iterations, conv_threshold, damping, true);   /* main_scan_3d.cpp:258-265 */
    if (rc) return rc;
    HIP_TRY(hipGetLastError());                  /* the frame's log row is written on the device: by the last workgroup of the
                                                    k_fuse that fused it, or by the gated k_fuse that found it not converged */
    return GSDF_OK;
}

int gsdf_read_frame_log(gsdf_ctx* c, float* rows10, int64_t max_rows, int64_t* n_rows) {
    GSDF_FLUSH(c);
    int rc = require_frame(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev_state s;
    rc = read_state(c, &s);
    if (rc) return rc;
    int64_t n = std::min<int64_t>(s.log_rows, c->frame_log_cap);
    if (n_rows) *n_rows = n;
    n = std::min<int64_t>(n, max_rows);
    if (n > 0 && rows10) {
        HIP_TRY(hipMemcpyAsync(rows10, c->frame.frame_log, (size_t)n * 10 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return GSDF_OK;
}

int gsdf_sync(gsdf_ctx* c) {
    GSDF_FLUSH(c);
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev_state s;
    int rc = read_state(c, &s);
    if (rc) return rc;
    prof_collect(c);
    return status_to_code(s.status);
}

int gsdf_get_stats(gsdf_ctx* c, gsdf_stats* out) {
    GSDF_FLUSH(c);
    if (!c || !out) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev_state s;
    int rc = read_state(c, &s);
    if (rc) return rc;
    std::memset(out, 0, sizeof(*out));
    if (c->frame.blk_counters) {
        std::vector<unsigned long long> h((size_t)c->fuse_blocks * 4);
        HIP_TRY(hipMemcpy(h.data(), c->frame.blk_counters, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long cu = 0, cv = 0;
        for (int b = 0; b < c->fuse_blocks; ++b) { cu += h[4 * b + 2]; cv += h[4 * b + 3]; }
        out->n_upd = (int64_t)cu;
        out->n_valid = (int64_t)cv;
    }
    out->n_hit = (int64_t)s.n_hit;
    out->track_passes = s.passes;
    out->converged = s.converged;
    out->frames = s.frames;
    out->n_deferred = (int64_t)s.n_deferred;
    out->fuse_timeouts = (int64_t)s.fuse_timeouts;
    out->far_tiles = c->progress ? (int64_t)c->progress[3] : 0;
    out->fuse_blocks = c->fuse_blocks;
    out->fuse_launches = c->fuse_launches;
    out->far_table_launches = c->far_table_launches;
    return GSDF_OK;
}

int gsdf_count(gsdf_ctx* c, int64_t* n) {
    GSDF_FLUSH(c);
    if (!c || !n) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h = 0;
    HIP_TRY(gsdf_counted(c, [&] { gsdf_launch_export(c->stream, c->tab, c->n_slots, nullptr, nullptr, c->counter, 0, 0, nullptr, 0, nullptr); }, &h));
    *n = (int64_t)h;
    return GSDF_OK;
}

static int export_impl(gsdf_ctx* c, int32_t* keys, float* payload, uint32_t* vis_words_out, int64_t max_n, int64_t* n_out,
                       int sorted, int raw_sums);

int gsdf_export(gsdf_ctx* c, int32_t* keys, float* payload, int64_t max_n, int64_t* n_out, int sorted, int raw_sums) {
    GSDF_FLUSH(c);
    return export_impl(c, keys, payload, nullptr, max_n, n_out, sorted, raw_sums);
}

int gsdf_enable_vis(gsdf_ctx* c, int max_frames) {
    GSDF_FLUSH(c);
    if (!c || max_frames <= 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->vis_words = (max_frames + 31) / 32;
    HIP_TRY(alloc_zeroed(c->map.vis, c->n_slots * (size_t)c->vis_words, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_export_vis(gsdf_ctx* c, int32_t* keys, uint32_t* words, int words_per_voxel, int64_t max_n, int64_t* n_out) {
    GSDF_FLUSH(c);
    if (!c || !words) return fail(GSDF_ERR_INVALID, "null argument");
    if (!c->map.vis) return fail(GSDF_ERR_INVALID, "gsdf_enable_vis was not called");
    if (words_per_voxel != c->vis_words) return fail(GSDF_ERR_INVALID, "words_per_voxel differs from gsdf_enable_vis");
    return export_impl(c, keys, nullptr, words, max_n, n_out, 1, 0);
}

static int export_impl(gsdf_ctx* c, int32_t* keys, float* payload, uint32_t* vis_words_out, int64_t max_n, int64_t* n_out,
                       int sorted, int raw_sums) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    int64_t n = 0;
    int rc = gsdf_count(c, &n);
    if (rc) return rc;
    if (n_out) *n_out = n;
    if (n == 0 || max_n <= 0 || (!keys && !payload && !vis_words_out)) return GSDF_OK;
    if (max_n < n) return fail(GSDF_ERR_INVALID, "export buffer too small (call gsdf_count first)");
    gsdf_dev<unsigned long long> dkeys;
    gsdf_dev<float> dpay;
    gsdf_dev<uint32_t> dvis;
    const int vw = vis_words_out ? c->vis_words : 0;
    HIP_TRY(dkeys.alloc((size_t)n));
    HIP_TRY(dpay.alloc((size_t)n * 5));
    if (vw) HIP_TRY(dvis.alloc((size_t)n * vw));
    HIP_TRY(gsdf_counter_zero(c));
    gsdf_launch_export(c->stream, c->tab, c->n_slots, dkeys, dpay, c->counter, n, raw_sums, c->map.vis, vw, dvis);
    std::vector<unsigned long long> hk((size_t)n);
    std::vector<float> hp((size_t)n * 5);
    std::vector<uint32_t> hv((size_t)n * vw);
    HIP_TRY(hipMemcpyAsync(hk.data(), dkeys, hk.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hp.data(), dpay, hp.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (vw) HIP_TRY(hipMemcpyAsync(hv.data(), dvis, hv.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<size_t> order((size_t)n);
    std::iota(order.begin(), order.end(), (size_t)0);
    if (sorted)   /* packed keys order like (z, y, x) */
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return hk[a] < hk[b]; });
    for (int64_t i = 0; i < n; ++i) {
        const size_t j = order[(size_t)i];
        if (keys) {
            int x, y, z;
            gsdf_key_unpack(hk[j], &x, &y, &z);
            keys[3 * i] = x; keys[3 * i + 1] = y; keys[3 * i + 2] = z;
        }
        if (payload) std::memcpy(payload + 5 * i, hp.data() + 5 * j, 5 * sizeof(float));
        if (vis_words_out) std::memcpy(vis_words_out + (size_t)vw * i, hv.data() + (size_t)vw * j, vw * sizeof(uint32_t));
    }
    return GSDF_OK;
}

int gsdf_merge_raw(gsdf_ctx* c, const int32_t* keys, const float* payload_raw, int64_t n) {
    GSDF_FLUSH(c);
    if (!c || (n > 0 && (!keys || !payload_raw))) return fail(GSDF_ERR_INVALID, "null argument");
    if (n <= 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev<int32_t> dk;
    gsdf_dev<float> dp;
    HIP_TRY(dk.alloc((size_t)n * 3));
    HIP_TRY(dp.alloc((size_t)n * 5));
    HIP_TRY(hipMemcpyAsync(dk, keys, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dp, payload_raw, (size_t)n * 5 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    c->occ_dirty = true;
    gsdf_launch_merge_raw(c->stream, c->tab, dk, dp, n, c->st);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return gsdf_sync(c);
}

int gsdf_export_raw_dev(gsdf_ctx* c, int32_t* keys_dev, float* payload_dev, int64_t max_n, int64_t* n) {
    GSDF_FLUSH(c);
    if (!c || !keys_dev || !payload_dev || max_n < 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long h = 0;
    HIP_TRY(gsdf_counted(c, [&] { gsdf_launch_export_raw(c->stream, c->tab, c->n_slots, keys_dev, payload_dev, c->counter, max_n); }, &h));
    if (n) *n = (int64_t)h;
    if ((int64_t)h > max_n) return fail(GSDF_ERR_INVALID, "export buffer too small (call gsdf_count first)");
    return GSDF_OK;
}

int gsdf_merge_raw_dev(gsdf_ctx* c, const int32_t* keys_dev, const float* payload_raw_dev, int64_t n) {
    GSDF_FLUSH(c);
    if (!c || (n > 0 && (!keys_dev || !payload_raw_dev))) return fail(GSDF_ERR_INVALID, "null argument");
    if (n <= 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    c->occ_dirty = true;
    gsdf_launch_merge_raw(c->stream, c->tab, keys_dev, payload_raw_dev, n, c->st);
    HIP_TRY(hipGetLastError());
    return gsdf_sync(c);
}

/* ---- PhotoBA: PhotometricOptimizer (ps_optimizer/PhotometricOptimizer.cpp) ------------------------------- */
static gsdf_ba_dev ba_dev(gsdf_ctx* c) {
    gsdf_ba_dev d;
    d.tab = c->tab; d.n_slots = c->n_slots; d.vis = c->map.vis; d.vis_words = c->vis_words;
    d.n = c->ba_n; d.W = c->W; d.H = c->H;
    d.images = c->ba.images; d.R = c->ba.Rt; d.t = c->ba.Rt + 9 * (size_t)c->ba_n; d.frame_idx = c->ba.frame_idx;
    d.fx = c->K[0]; d.fy = c->K[4]; d.cx = c->K[2]; d.cy = c->K[5]; d.vs = c->voxel_size; d.reg_weight = c->ba_reg;
    d.trunc_sq = c->ba_trunc_sq;
    d.gate_list = c->ba_gate_fresh ? c->ba.gate_list : nullptr;
    d.gate_count = c->ba.counter2;
    d.mean_cache = c->ba.mean;
    return d;
}
/* (re)builds the list of the voxels inside the |dist| <= vs gate, if the distances may have changed since it was made.  Enqueue
 * only; failures leave the sweeps on their whole-table form (gate_list == nullptr). */
static void ba_refresh_gate(gsdf_ctx* c) {
    if (c->ba_gate_fresh || !c->ba.gate_list || !c->ba.counter2) return;
    gsdf_ba_dev d = ba_dev(c);
    if (gsdf_ba_compact(c->ba.gate_tmp, c->stream, d, c->ba.gate_list, c->ba.counter2) == hipSuccess) c->ba_gate_fresh = true;
    else (void)hipGetLastError();
}
static int ba_upload_poses(gsdf_ctx* c) {
    HIP_TRY(hipMemcpyAsync(c->ba.Rt, c->ba_R.data(), c->ba_R.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ba.Rt + 9 * (size_t)c->ba_n, c->ba_t.data(), c->ba_t.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}
static int ba_require(gsdf_ctx* c) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    if (!c->ba_n) return fail(GSDF_ERR_INVALID, "gsdf_ba_setup was not called");
    return GSDF_OK;
}

int gsdf_ba_set_loss(gsdf_ctx* c, int loss, float lambda) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    if (loss < 0 || loss > 4 || !(lambda >= 0.f)) return fail(GSDF_ERR_INVALID, "loss must be a LossFunction value (0..4), lambda >= 0");
    c->ba_trunc_sq = loss == 4 ? lambda * lambda : -1.f;          /* the reference's code only distinguishes TRUNC_L2 */
    return GSDF_OK;
}

int gsdf_ba_setup(gsdf_ctx* c, int n, const float* images_bgr_host, const float* poses16_host, const int* frame_idx,
                  float reg_weight) {
    GSDF_FLUSH(c);
    int rc = require_frame(c);
    if (rc) return rc;
    if (c->map_type != GSDF_MAP_GRAD) return fail(GSDF_ERR_INVALID, "PhotoBA needs the Gradient-SDF map (a base-sdf context has no gradient)");
    if (!c->map.vis) return fail(GSDF_ERR_INVALID, "PhotoBA needs the vis_ bit-vectors: call gsdf_enable_vis before fusing");
    if (n <= 0 || n > 64 || !images_bgr_host || !poses16_host || !frame_idx) return fail(GSDF_ERR_INVALID, "bad argument (1..64 keyframes)");
    /* what the sweeps cannot index: ba_visible turns an id into a word and a bit of vis_ (a negative one lies in front of the
     * buffer), and computeImageGradient's border branch reads column / row -1 of an image with fewer than 2 */
    for (int i = 0; i < n; ++i)
        if (frame_idx[i] < 0) return fail(GSDF_ERR_INVALID, "frame_idx: keyframe ids must be >= 0");
    if (c->W < 2 || c->H < 2) return fail(GSDF_ERR_INVALID, "PhotoBA needs frames of at least 2 x 2 pixels (the image gradient reads a neighbour)");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->ba = gsdf_ba_bufs();                                  /* the old setup goes first; until the commit below there is none */
    c->ba_n = 0; c->ba_gate_fresh = false; c->ba_mean_valid = false; c->ba_pose_step = 0;
    gsdf_ba_bufs b;
    const size_t img_count = (size_t)n * c->W * c->H * 3;
    HIP_TRY(b.images.alloc(img_count));
    HIP_TRY(b.Rt.alloc((size_t)n * 12));
    HIP_TRY(b.frame_idx.alloc((size_t)n));
    /* two sets of 3 x blocks doubles (energy, voxels, observations per workgroup): gsdf_ba_optimize keeps the sweep behind the
     * pose step and the one behind the distance step apart and reads both with one synchronisation */
    HIP_TRY(b.block_E.alloc((size_t)2 * 3 * gsdf_ba_blocks()));
    HIP_TRY(b.block_part.alloc((size_t)gsdf_ba_blocks() * n * 27));
    HIP_TRY(b.Hb.alloc((size_t)n * 27));
    {   /* the gate list of the energy / pose sweeps: optional (without it they sweep the whole table) */
        size_t bytes = 0;
        if (gsdf_ba_compact_need(ba_dev(c), &bytes) == hipSuccess &&
            b.gate_list.alloc(c->n_slots) == hipSuccess && b.gate_tmp.alloc(bytes) == hipSuccess && b.counter2.alloc(1) == hipSuccess) {
            /* optional on top: 24 B per possible list entry for what the energy sweep hands to the pose sweep (100 MB at 2^22 records) */
            /* GSDF_BA_MEAN_CACHE (read here, so that a test can switch within one context): 0 the pose sweep computes its means
             * itself; 2 (tests only) the stand-alone gsdf_ba_solve_pose trusts that nothing changed since the last energy sweep */
            const char* env = getenv("GSDF_BA_MEAN_CACHE");
            c->ba_mean_on = env ? atoi(env) : 1;
            if (c->ba_mean_on && b.mean.alloc(c->n_slots * 24) != hipSuccess) (void)hipGetLastError();
        } else {
            (void)hipGetLastError();
            b.gate_list.reset(); b.gate_tmp.reset(); b.counter2.reset();
        }
    }
    std::vector<float> R(9 * (size_t)n), t(3 * (size_t)n);
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k) R[9 * i + 3 * r + k] = poses16_host[16 * i + 4 * r + k];
            t[3 * i + r] = poses16_host[16 * i + 4 * r + 3];
        }
    HIP_TRY(hipMemcpyAsync(b.images, images_bgr_host, img_count * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.frame_idx, frame_idx, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.Rt, R.data(), R.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(b.Rt + R.size(), t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    /* the commit: only a complete setup, with its keyframe count and poses, reaches the context */
    c->ba = std::move(b);
    c->ba_n = n; c->ba_reg = reg_weight;
    c->ba_R = std::move(R); c->ba_t = std::move(t);
    return GSDF_OK;
}

/* the energy sweep enqueued into set `which` of the per-workgroup sums; ba_energy_sum adds a set up in the fixed order */
static int ba_energy_enqueue(gsdf_ctx* c, int which, bool pose_sweep_follows = true) {
    ba_refresh_gate(c);
    const gsdf_ba_dev d = ba_dev(c);
    /* the sweep leaves every gated voxel's mean intensity / keyframe set behind for a pose sweep at this same state */
    const bool write_mean = pose_sweep_follows && d.gate_list && d.mean_cache && c->ba_trunc_sq < 0.f;
    gsdf_launch_ba_energy(c->stream, d, c->ba.block_E + (size_t)which * 3 * gsdf_ba_blocks(), write_mean);
    c->ba_mean_valid = write_mean;
    HIP_TRY(hipGetLastError());
    return GSDF_OK;
}
static float ba_energy_sum(gsdf_ctx* c, const double* h) {
    const size_t nb = (size_t)gsdf_ba_blocks();
    double s = 0.0, a = 0.0, o = 0.0;
    for (size_t i = 0; i < nb; ++i) { s += h[i]; a += h[nb + i]; o += h[2 * nb + i]; }
    c->ba_last_voxels = (long long)a; c->ba_last_obs = (long long)o;
    return (float)s;
}

int gsdf_ba_energy(gsdf_ctx* c, float* E) {
    GSDF_FLUSH(c);
    int rc = ba_require(c);
    if (rc) return rc;
    c->ba_gate_fresh = false;                                 /* the map may have changed since the last BA call */
    if (!E) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = ba_energy_enqueue(c, 0))) return rc;
    std::vector<double> h((size_t)3 * gsdf_ba_blocks());
    HIP_TRY(hipMemcpyAsync(h.data(), c->ba.block_E, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *E = ba_energy_sum(c, h.data());
    return GSDF_OK;
}

int gsdf_ba_counters(gsdf_ctx* c, int64_t* voxels, int64_t* observations) {
    if (!c || !voxels || !observations) return fail(GSDF_ERR_INVALID, "null argument");
    *voxels = c->ba_last_voxels; *observations = c->ba_last_obs;
    return GSDF_OK;
}

static int ba_dist_enqueue(gsdf_ctx* c, float damping, double* block_cnt = nullptr) {
    gsdf_launch_ba_dist(c->stream, ba_dev(c), damping, block_cnt);
    c->ba_gate_fresh = false;                                 /* the distances moved: voxels may have crossed the gate */
    c->ba_mean_valid = false;
    HIP_TRY(hipGetLastError());
    return GSDF_OK;
}
int gsdf_ba_solve_dist(gsdf_ctx* c, float damping) {
    GSDF_FLUSH(c);
    int rc = ba_require(c);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    /* the stand-alone entry also counts what the sweep visited (gsdf_ba_counters); gsdf_ba_optimize's sweeps do not */
    double* cnt = c->ba.block_E + (size_t)3 * gsdf_ba_blocks();
    if ((rc = ba_dist_enqueue(c, damping, cnt))) return rc;
    std::vector<double> h((size_t)2 * gsdf_ba_blocks());
    HIP_TRY(hipMemcpyAsync(h.data(), cnt, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    double a = 0.0, o = 0.0;
    for (size_t i = 0; i < (size_t)gsdf_ba_blocks(); ++i) { a += h[i]; o += h[(size_t)gsdf_ba_blocks() + i]; }
    c->ba_last_voxels = (long long)a; c->ba_last_obs = (long long)o;
    return GSDF_OK;
}

/* one keyframe's update from its six components of the step: t_i -= dp[0..2], R_i = R_i * SO3::exp(-dp[3..5]) (solvePose
 * :584-588, solvePoseFull :491-494) */
static void ba_apply_delta(gsdf_ctx* c, int i, const float* dp) {
    for (int k = 0; k < 3; ++k) c->ba_t[3 * i + k] -= dp[k];
    float pose[7] = { 0, 0, 0, 0, 0, 0, 1 };
    const float xi[6] = { 0, 0, 0, -dp[3], -dp[4], -dp[5] };
    gsdf_se3_exp_mul(xi, pose);                               /* SO3::exp(-omega) */
    float Ex[9], Rn[9];
    gsdf_quat_to_R(pose + 3, Ex);
    const float* Ri = &c->ba_R[9 * (size_t)i];
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) Rn[3 * r + k] = gsdf_sum3(Ri[3 * r] * Ex[k], Ri[3 * r + 1] * Ex[3 + k], Ri[3 * r + 2] * Ex[6 + k]);
    std::memcpy(&c->ba_R[9 * (size_t)i], Rn, sizeof(Rn));
}

/* the pose sweep + the per-keyframe 6x6 solves; wait_upload: block until the new poses are on the device (the public entry)
 * or leave the copy queued in front of whatever the caller enqueues next (gsdf_ba_optimize) */
static int ba_solve_pose(gsdf_ctx* c, bool wait_upload) {
    const int n = c->ba_n;
    const bool list_was_fresh = c->ba_gate_fresh;
    ba_refresh_gate(c);
    /* (the cache belongs to the list the energy sweep walked: a list rebuilt since then has other entries) */
    gsdf_launch_ba_pose(c->stream, ba_dev(c), c->ba.block_part, c->ba.Hb, c->ba_mean_valid && list_was_fresh);
    c->ba_mean_valid = false;                                 /* the poses move */
    std::vector<float> hb((size_t)n * 27);
    HIP_TRY(hipMemcpyAsync(hb.data(), c->ba.Hb, hb.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));                 /* the 6x6 systems are solved on the host (:577-589) */
    for (int i = 0; i < n; ++i) {                             /* per-keyframe 6x6 LDLT + pose update (:577-589) */
        const float* v = &hb[27 * (size_t)i];
        float H[36], dp[6];
        int q = 6;
        for (int a1 = 0; a1 < 6; ++a1) for (int a2 = a1; a2 < 6; ++a2) { H[6 * a1 + a2] = v[q]; H[6 * a2 + a1] = v[q]; ++q; }
        gsdf_ldlt_solve6(H, v, dp);
        bool nan = false;
        for (int k = 0; k < 6; ++k) nan = nan || std::isnan(dp[k]);
        if (nan) continue;
        ba_apply_delta(c, i, dp);
    }
    if (wait_upload) return ba_upload_poses(c);
    /* c->ba_R / ba_t are members: they stay untouched until the caller's next synchronisation, which is behind these copies */
    HIP_TRY(hipMemcpyAsync(c->ba.Rt, c->ba_R.data(), c->ba_R.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ba.Rt + 9 * (size_t)c->ba_n, c->ba_t.data(), c->ba_t.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return GSDF_OK;
}
int gsdf_ba_solve_pose(gsdf_ctx* c, float damping) {
    GSDF_FLUSH(c);
    (void)damping;                                            /* unused by the reference as well (:499) */
    int rc = ba_require(c);
    if (rc) return rc;
    if (c->ba_mean_on != 2) {
        c->ba_gate_fresh = false;                             /* the map may have changed since the last BA call */
        c->ba_mean_valid = false;
    }
    HIP_TRY(hipSetDevice(c->device));
    return ba_solve_pose(c, true);
}

/* ---- solvePoseFull (:392-496): the coupled 6n x 6n system ---- */
/* H (6n)^2 row-major, b 6n, at the current state.  The diagonal blocks and b are the pose sweep's 27 sums per keyframe -- bit for
 * bit what the decoupled step solves -- and the off-diagonal blocks come from the contraction of gsdf_ba_full.hip.  Its two
 * buffers are allocated here, by the first coupled call after a gsdf_ba_setup. */
static int ba_full_system(gsdf_ctx* c, std::vector<float>& H, std::vector<float>& b) {
    const int n = c->ba_n, N = 6 * n;
    HIP_TRY(c->ba.full_part.grow(gsdf_ba_full_part_floats(n)));
    HIP_TRY(c->ba.full_H.grow((size_t)N * N));
    const bool list_was_fresh = c->ba_gate_fresh;
    ba_refresh_gate(c);
    const gsdf_ba_dev d = ba_dev(c);
    gsdf_launch_ba_pose(c->stream, d, c->ba.block_part, c->ba.Hb, c->ba_mean_valid && list_was_fresh);
    gsdf_launch_ba_full(c->stream, d, c->ba.full_part, c->ba.full_H);
    HIP_TRY(hipGetLastError());
    std::vector<float> hb((size_t)n * 27);
    H.resize((size_t)N * N); b.resize((size_t)N);
    HIP_TRY(hipMemcpyAsync(hb.data(), c->ba.Hb, hb.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(H.data(), c->ba.full_H, H.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; ++i) {                             /* :461-466 */
        const float* v = &hb[27 * (size_t)i];
        for (int k = 0; k < 6; ++k) b[6 * (size_t)i + k] = v[k];
        int q = 6;
        for (int a1 = 0; a1 < 6; ++a1)
            for (int a2 = a1; a2 < 6; ++a2) {
                H[(size_t)(6 * i + a1) * N + 6 * i + a2] = v[q]; H[(size_t)(6 * i + a2) * N + 6 * i + a1] = v[q]; ++q;
            }
    }
    return GSDF_OK;
}
int gsdf_ba_pose_system(gsdf_ctx* c, float* H, float* b) {
    GSDF_FLUSH(c);
    int rc = ba_require(c);
    if (rc) return rc;
    if (!H && !b) return fail(GSDF_ERR_INVALID, "null argument (H and b)");
    if (c->ba_mean_on != 2) {
        c->ba_gate_fresh = false;                             /* the map may have changed since the last BA call */
        c->ba_mean_valid = false;
    }
    HIP_TRY(hipSetDevice(c->device));
    std::vector<float> Hh, bh;
    if ((rc = ba_full_system(c, Hh, bh))) return rc;
    if (H) std::memcpy(H, Hh.data(), Hh.size() * sizeof(float));
    if (b) std::memcpy(b, bh.data(), bh.size() * sizeof(float));
    return GSDF_OK;
}
/* the coupled system + one LDLT of the whole of it (:483) + the pose update; wait_upload as in ba_solve_pose */
static int ba_solve_pose_full(gsdf_ctx* c, bool wait_upload) {
    const int n = c->ba_n;
    std::vector<float> H, b;
    int rc = ba_full_system(c, H, b);
    if (rc) return rc;
    c->ba_mean_valid = false;                                 /* the poses move */
    std::vector<float> delta((size_t)6 * n);
    gsdf_ldlt_solve(6 * n, H.data(), b.data(), delta.data());
    bool nan = false;                                         /* :488-490: any NaN and no pose moves */
    for (float v : delta) nan = nan || std::isnan(v);
    if (!nan)
        for (int i = 0; i < n; ++i) ba_apply_delta(c, i, &delta[6 * (size_t)i]);
#ifdef GSDF_EXPERIMENTS
    c->ba_last_delta = delta;
#endif
    if (wait_upload) return ba_upload_poses(c);
    HIP_TRY(hipMemcpyAsync(c->ba.Rt, c->ba_R.data(), c->ba_R.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->ba.Rt + 9 * (size_t)c->ba_n, c->ba_t.data(), c->ba_t.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return GSDF_OK;
}
int gsdf_ba_solve_pose_full(gsdf_ctx* c, float damping) {
    GSDF_FLUSH(c);
    (void)damping;                                            /* unused by the reference as well (:392) */
    int rc = ba_require(c);
    if (rc) return rc;
    if (c->ba_mean_on != 2) {
        c->ba_gate_fresh = false;                             /* the map may have changed since the last BA call */
        c->ba_mean_valid = false;
    }
    HIP_TRY(hipSetDevice(c->device));
    return ba_solve_pose_full(c, true);
}
int gsdf_ba_set_pose_step(gsdf_ctx* c, int mode) {
    int rc = ba_require(c);
    if (rc) return rc;
    if (mode != 0 && mode != 1) return fail(GSDF_ERR_INVALID, "pose step must be 0 (solvePose) or 1 (solvePoseFull)");
    c->ba_pose_step = mode;
    return GSDF_OK;
}
#ifdef GSDF_EXPERIMENTS
/* test build only: the 6n components of the last coupled step's solution */
int gsdf_debug_ba_delta(gsdf_ctx* c, float* delta) {
    if (!c || !delta || c->ba_last_delta.size() != (size_t)6 * c->ba_n) return GSDF_ERR_INVALID;
    std::memcpy(delta, c->ba_last_delta.data(), c->ba_last_delta.size() * sizeof(float));
    return GSDF_OK;
}
#endif

/* optimize (:611-662).  Per iteration the host needs two things from the device: the 27 sums per keyframe of the pose sweep
 * (it solves the 6x6 systems) and, for the stop rule, the two energies.  So an iteration synchronises twice: behind the pose
 * sweep, and ONCE behind [energy -> distance sweep -> energy], both energies in one read (they used to be four waits). */
int gsdf_ba_optimize(gsdf_ctx* c, int max_it, float* energies, int* n_energies, int* converged) {
    GSDF_FLUSH(c);
    int rc = ba_require(c);
    if (rc) return rc;
    c->ba_gate_fresh = false;                                 /* the map may have changed since the last BA call */
    if (!energies || !n_energies || !converged || max_it < 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    int ne = 0;
    float E = 0.f, E_pose = 0.f;
    *converged = 0;
    if ((rc = gsdf_ba_energy(c, &E))) return rc;
    energies[ne++] = E;
    const size_t set = (size_t)3 * gsdf_ba_blocks();
    std::vector<double> h(2 * set);
    for (int iter = 0; iter < max_it; ++iter) {               /* :621-657 */
        if ((rc = c->ba_pose_step ? ba_solve_pose_full(c, false) : ba_solve_pose(c, false))) return rc;   /* :627-628 */
        if ((rc = ba_energy_enqueue(c, 0, false))) return rc;  /* (the distance sweep follows: nobody reads its means) */
        if ((rc = ba_dist_enqueue(c, 1.0f))) return rc;
        if ((rc = ba_energy_enqueue(c, 1))) return rc;
        HIP_TRY(hipMemcpyAsync(h.data(), c->ba.block_E, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        E_pose = ba_energy_sum(c, h.data());
        E = ba_energy_sum(c, h.data() + set);
        energies[ne++] = E_pose;
        energies[ne++] = E;
        const float rel = std::fabs(E_pose - E) / E_pose;
        if (rel < 0.0005f) { *converged = 1; break; }
        if (E_pose < E) break;                                /* diverged */
    }
    *n_energies = ne;
    return GSDF_OK;
}

int gsdf_ba_get_poses(gsdf_ctx* c, float* poses16_host) {
    int rc = ba_require(c);
    if (rc) return rc;
    if (!poses16_host) return fail(GSDF_ERR_INVALID, "null argument");
    for (int i = 0; i < c->ba_n; ++i) {
        float* P = poses16_host + 16 * (size_t)i;
        for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) P[4 * r + k] = c->ba_R[9 * (size_t)i + 3 * r + k]; P[4 * r + 3] = c->ba_t[3 * (size_t)i + r]; }
        P[12] = P[13] = P[14] = 0.f; P[15] = 1.f;
    }
    return GSDF_OK;
}

/* device scratch for a batch of `bytes`: the context's own for single points / small batches (no allocation per call), else
 * `big`, which lives as long as the caller's frame */
static int batch_scratch(gsdf_ctx* c, size_t bytes, gsdf_dev<void>& big, void** out) {
    const bool small = bytes <= GSDF_SCRATCH_BYTES;
    gsdf_dev<void>& b = small ? c->scratch : big;
    HIP_TRY(b.grow(small ? GSDF_SCRATCH_BYTES : bytes));
    *out = b;
    return GSDF_OK;
}

int gsdf_query(gsdf_ctx* c, const float* pts_host, int64_t n, float* dist, float* grad, float* w) {
    GSDF_FLUSH(c);
    if (!c || (n > 0 && (!pts_host || !dist || !grad || !w))) return fail(GSDF_ERR_INVALID, "null argument");
    if (n <= 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev<void> big;
    float* d = nullptr;
    if (int rc = batch_scratch(c, (size_t)n * 8 * sizeof(float), big, (void**)&d)) return rc;
    float *dp = d, *dd = d + 3 * n, *dg = d + 4 * n, *dw = d + 7 * n;
    HIP_TRY(hipMemcpyAsync(dp, pts_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    gsdf_launch_query(c->stream, c->tab, c->voxel_size, c->voxel_size_inv, dp, n, dd, dg, dw,
                      c->map_type == GSDF_MAP_BASE ? c->T : -1.f);
    HIP_TRY(hipMemcpyAsync(dist, dd, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(grad, dg, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(w, dw, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_get_voxels(gsdf_ctx* c, const int32_t* keys_host, int64_t n, float* payload, int32_t* found) {
    GSDF_FLUSH(c);
    if (!c || (n > 0 && (!keys_host || !payload || !found))) return fail(GSDF_ERR_INVALID, "null argument");
    if (n <= 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev<void> big;
    char* d = nullptr;
    if (int rc = batch_scratch(c, (size_t)n * (3 * sizeof(int32_t) + 5 * sizeof(float) + sizeof(int32_t)), big, (void**)&d)) return rc;
    int32_t* dk = (int32_t*)d;
    float* dp = (float*)(d + (size_t)n * 3 * sizeof(int32_t));
    int32_t* df = (int32_t*)(d + (size_t)n * (3 * sizeof(int32_t) + 5 * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(dk, keys_host, (size_t)n * 3 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    gsdf_launch_get_voxels(c->stream, c->tab, dk, n, dp, df);
    HIP_TRY(hipMemcpyAsync(payload, dp, (size_t)n * 5 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(found, df, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

/* RigidPointOptimizer.cpp:51-96 over points already on the device.  Pairs of pass + head are queued in batches (both kernels
 * return at once when the run has ended); the host reads the run's small state once per batch, never per pass. */
/* loss < 0: the plain pair and rows of 36 floats (gsdf_align_points); loss in 0..4: the robust pair and rows of 38 */
static int align_points_impl(gsdf_ctx* c, const float* pts_dev, int64_t n, float pose7[7], int num_iterations, float conv_threshold,
                             float damping, int* converged, int* passes, float* trace36, int loss = -1, float scale = 0.f) {
    const size_t row = loss >= 0 ? 38 : 36;
    const size_t part_bytes = (size_t)GSDF_ALIGN_MAXBLK * GSDF_ALIGN_ROW * sizeof(double);
    HIP_TRY(c->align.grow(256 + part_bytes));
    gsdf_align_state* d_st = c->align.as<gsdf_align_state>();
    double* d_part = (double*)(c->align.as<char>() + 256);
    gsdf_dev<float> d_trace;
    if (trace36) HIP_TRY(d_trace.alloc((size_t)num_iterations * row));
    gsdf_align_state h;
    std::memcpy(h.pose7, pose7, sizeof(h.pose7));
    h.done = 0; h.converged = 0; h.passes = 0;
    HIP_TRY(hipMemcpyAsync(d_st, &h, sizeof(h), hipMemcpyHostToDevice, c->stream));
    const float conv_sq = conv_threshold * conv_threshold;                 /* RigidOptimizer.h:72 */
    int queued = 0;
    while (queued < num_iterations) {
        const int batch = std::min(num_iterations - queued, queued == 0 ? c->first_batch : c->next_batch);
        for (int k = 0; k < batch; ++k)
            gsdf_launch_align_pass(c->stream, c->tab, c->voxel_size, c->voxel_size_inv, pts_dev, n, d_st, d_part, conv_sq, damping,
                                   num_iterations, d_trace, loss, scale);
        HIP_TRY(hipGetLastError());
        queued += batch;
        HIP_TRY(hipMemcpyAsync(&h, d_st, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (h.done) break;
    }
    if (trace36 && h.passes > 0) {
        HIP_TRY(hipMemcpyAsync(trace36, d_trace, (size_t)h.passes * row * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    std::memcpy(pose7, h.pose7, sizeof(h.pose7));
    *converged = h.converged;
    *passes = h.passes;
    return GSDF_OK;
}

static int align_points_check(gsdf_ctx* c, const float* pts, int64_t n, const float* pose7, int num_iterations, const int* converged,
                              const int* passes) {
    if (!c || !pose7 || !converged || !passes) return fail(GSDF_ERR_INVALID, "gsdf_align_points: null argument");
    if (n < 0 || num_iterations < 0) return fail(GSDF_ERR_INVALID, "gsdf_align_points: negative n or num_iterations");
    if (n > 0 && !pts) return fail(GSDF_ERR_INVALID, "gsdf_align_points: null points");
    if (c->map_type == GSDF_MAP_BASE)
        return fail(GSDF_ERR_INVALID, "gsdf_align_points: not available on a base-sdf context (it reads the stored gradient)");
    return GSDF_OK;
}

int gsdf_align_points_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float pose7[7], int num_iterations, float conv_threshold,
                          float damping, int* converged, int* passes, float* trace36) {
    GSDF_FLUSH(c);
    if (int rc = align_points_check(c, pts_dev, n, pose7, num_iterations, converged, passes)) return rc;
    *converged = 0; *passes = 0;
    if (num_iterations == 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    return align_points_impl(c, pts_dev, n, pose7, num_iterations, conv_threshold, damping, converged, passes, trace36);
}

int gsdf_align_points(gsdf_ctx* c, const float* pts_host, int64_t n, float pose7[7], int num_iterations, float conv_threshold,
                      float damping, int* converged, int* passes, float* trace36) {
    GSDF_FLUSH(c);
    if (int rc = align_points_check(c, pts_host, n, pose7, num_iterations, converged, passes)) return rc;
    *converged = 0; *passes = 0;
    if (num_iterations == 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev<void> big;
    float* d = nullptr;
    if (int rc = batch_scratch(c, (size_t)n * 3 * sizeof(float), big, (void**)&d)) return rc;
    if (n > 0) HIP_TRY(hipMemcpyAsync(d, pts_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return align_points_impl(c, d, n, pose7, num_iterations, conv_threshold, damping, converged, passes, trace36);
}

/* m runs of align_points_impl side by side.  Scratch in c->align: the m states, the list of live runs behind them (at byte
 * 64 m), then from byte 256 m the partial rows part[m][grid][GSDF_ALIGN_ROW].  The batches are those of the single call; after
 * each the host reads the m states and packs the runs that have not ended into the list of the next batch's launches. */
static int align_multi_impl(gsdf_ctx* c, const float* pts_dev, int64_t n, float* poses7, int m, int num_iterations, float conv_threshold,
                            float damping, int* converged, int* passes, float* last36, float* trace36, int loss = -1, float scale = 0.f) {
    const size_t row = loss >= 0 ? 38 : 36;                                /* as align_points_impl */
    const int grid = gsdf_align_grid(n);
    const size_t need = (size_t)m * (256 + (size_t)grid * GSDF_ALIGN_ROW * sizeof(double));
    if (c->align.bytes() < need) {                                         /* a failed allocation leaves the old scratch in place */
        gsdf_dev<void> bigger;
        HIP_TRY(bigger.alloc(need));
        c->align = std::move(bigger);
    }
    gsdf_align_state* d_st = c->align.as<gsdf_align_state>();
    int* d_live = (int*)(c->align.as<char>() + (size_t)m * 64);
    double* d_part = (double*)(c->align.as<char>() + (size_t)m * 256);
    gsdf_dev<float> d_trace, d_last;
    const size_t trace_n = (size_t)m * num_iterations * row;
    if (trace36) HIP_TRY(d_trace.alloc(trace_n));
    if (last36) HIP_TRY(d_last.alloc((size_t)m * row));
    std::vector<gsdf_align_state> h((size_t)m);
    std::vector<int> live((size_t)m);
    for (int i = 0; i < m; ++i) {
        std::memcpy(h[i].pose7, poses7 + 7 * i, sizeof(h[i].pose7));
        h[i].done = 0; h[i].converged = 0; h[i].passes = 0;
        live[i] = i;
    }
    HIP_TRY(hipMemcpyAsync(d_st, h.data(), (size_t)m * sizeof(gsdf_align_state), hipMemcpyHostToDevice, c->stream));
    if (trace36) HIP_TRY(hipMemsetAsync(d_trace, 0, trace_n * sizeof(float), c->stream));       /* rows beyond a run's end stay zero */
    if (last36) HIP_TRY(hipMemsetAsync(d_last, 0, (size_t)m * row * sizeof(float), c->stream));
    const float conv_sq = conv_threshold * conv_threshold;                 /* RigidOptimizer.h:72 */
    int queued = 0, n_live = m;
    while (queued < num_iterations && n_live > 0) {
        const int batch = std::min(num_iterations - queued, queued == 0 ? c->first_batch : c->next_batch);
        HIP_TRY(hipMemcpyAsync(d_live, live.data(), (size_t)n_live * sizeof(int), hipMemcpyHostToDevice, c->stream));
        for (int k = 0; k < batch; ++k)
            gsdf_launch_align_pass_multi(c->stream, c->tab, c->voxel_size, c->voxel_size_inv, pts_dev, n, d_st, d_part, d_live, n_live,
                                         conv_sq, damping, num_iterations, d_trace, d_last, loss, scale);
        HIP_TRY(hipGetLastError());
        queued += batch;
        HIP_TRY(hipMemcpyAsync(h.data(), d_st, (size_t)m * sizeof(gsdf_align_state), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        int kept = 0;
        for (int i = 0; i < n_live; ++i)
            if (!h[live[i]].done) live[kept++] = live[i];                 /* index order is kept; the order has no bearing on a run's bytes */
        n_live = kept;
    }
    if (trace36) HIP_TRY(hipMemcpyAsync(trace36, d_trace, trace_n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (last36) HIP_TRY(hipMemcpyAsync(last36, d_last, (size_t)m * row * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (trace36 || last36) HIP_TRY(hipStreamSynchronize(c->stream));
    for (int i = 0; i < m; ++i) {
        std::memcpy(poses7 + 7 * i, h[i].pose7, sizeof(h[i].pose7));
        converged[i] = h[i].converged;
        passes[i] = h[i].passes;
    }
    return GSDF_OK;
}

static int align_multi_check(gsdf_ctx* c, const float* pts, int64_t n, const float* poses7, int m, int num_iterations,
                             const int* converged, const int* passes) {
    if (int rc = align_points_check(c, pts, n, poses7, num_iterations, converged, passes)) return rc;
    if (m < 1 || m > GSDF_ALIGN_MAX_STARTS) return fail(GSDF_ERR_INVALID, "gsdf_align_points_multi: m outside 1 .. GSDF_ALIGN_MAX_STARTS");
    return GSDF_OK;
}

/* num_iterations == 0, per run as the single call: nothing executed */
static int align_multi_none(int m, int* converged, int* passes, float* last36, size_t row = 36) {
    std::fill(converged, converged + m, 0);
    std::fill(passes, passes + m, 0);
    if (last36) std::fill(last36, last36 + (size_t)m * row, 0.f);
    return GSDF_OK;
}

int gsdf_align_points_multi_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float* poses7, int m, int num_iterations,
                                float conv_threshold, float damping, int* converged, int* passes, float* last36, float* trace36) {
    GSDF_FLUSH(c);
    if (int rc = align_multi_check(c, pts_dev, n, poses7, m, num_iterations, converged, passes)) return rc;
    if (num_iterations == 0) return align_multi_none(m, converged, passes, last36);
    HIP_TRY(hipSetDevice(c->device));
    return align_multi_impl(c, pts_dev, n, poses7, m, num_iterations, conv_threshold, damping, converged, passes, last36, trace36);
}

int gsdf_align_points_multi(gsdf_ctx* c, const float* pts_host, int64_t n, float* poses7, int m, int num_iterations,
                            float conv_threshold, float damping, int* converged, int* passes, float* last36, float* trace36) {
    GSDF_FLUSH(c);
    if (int rc = align_multi_check(c, pts_host, n, poses7, m, num_iterations, converged, passes)) return rc;
    if (num_iterations == 0) return align_multi_none(m, converged, passes, last36);
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev<void> big;
    float* d = nullptr;
    if (int rc = batch_scratch(c, (size_t)n * 3 * sizeof(float), big, (void**)&d)) return rc;
    if (n > 0) HIP_TRY(hipMemcpyAsync(d, pts_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return align_multi_impl(c, d, n, poses7, m, num_iterations, conv_threshold, damping, converged, passes, last36, trace36);
}

/* host only: the grid of starting poses around a centre (include/gsdf.h states the arithmetic; all of it in double) */
int gsdf_align_starts(const float center7[7], const float pivot[3], float rot_step_rad, int rot_k, float trans_step, int trans_k,
                      float* poses7_out, int max_m, int* m) {
    if (!center7 || !pivot || !m) return fail(GSDF_ERR_INVALID, "gsdf_align_starts: null argument");
    if (rot_k < 0 || trans_k < 0 || max_m < 0) return fail(GSDF_ERR_INVALID, "gsdf_align_starts: negative rot_k, trans_k or max_m");
    bool finite = std::isfinite(rot_step_rad) && std::isfinite(trans_step);
    for (int i = 0; i < 7; ++i) finite = finite && std::isfinite(center7[i]);
    for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(pivot[i]);
    if (!finite) return fail(GSDF_ERR_INVALID, "gsdf_align_starts: an input is not finite");
    const double cq[4] = { center7[3], center7[4], center7[5], center7[6] };
    const double cn = std::sqrt(cq[0] * cq[0] + cq[1] * cq[1] + cq[2] * cq[2] + cq[3] * cq[3]);
    if (!(std::fabs(cn - 1.0) <= 1e-4)) return fail(GSDF_ERR_INVALID, "gsdf_align_starts: the centre's quaternion is not of unit length");
    const long long Rn = 2LL * rot_k + 1, Tn = 2LL * trans_k + 1;
    /* Rn, Tn < 2^32: a product that would pass 2^31 - 1 is reported as that */
    long long count = 1;
    for (const long long f : { Rn, Rn, Rn, Tn, Tn, Tn }) count = std::min<long long>(count * f, 0x7fffffffLL);
    const int total = (int)count;
    *m = total;
    if (total > GSDF_ALIGN_MAX_STARTS) return fail(GSDF_ERR_INVALID, "gsdf_align_starts: more than GSDF_ALIGN_MAX_STARTS starts");
    if (!poses7_out || max_m == 0) return GSDF_OK;                          /* the sizing call */
    if (max_m < total) return fail(GSDF_ERR_INVALID, "gsdf_align_starts: max_m too small (*m holds the need)");
    auto quat_R = [](const double q[4], double R[9]) {                      /* x y z w, unit length */
        const double x = q[0], y = q[1], z = q[2], w = q[3];
        R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w);     R[2] = 2 * (x * z + y * w);
        R[3] = 2 * (x * y + z * w);     R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
        R[6] = 2 * (x * z - y * w);     R[7] = 2 * (y * z + x * w);     R[8] = 1 - 2 * (x * x + y * y);
    };
    auto matvec = [](const double R[9], const double v[3], double o[3]) {
        for (int i = 0; i < 3; ++i) o[i] = R[3 * i] * v[0] + R[3 * i + 1] * v[1] + R[3 * i + 2] * v[2];
    };
    const double qc[4] = { cq[0] / cn, cq[1] / cn, cq[2] / cn, cq[3] / cn };
    const double tc[3] = { center7[0], center7[1], center7[2] }, pv[3] = { pivot[0], pivot[1], pivot[2] };
    const double rs = rot_step_rad, ts = trans_step;
    double Rc[9];
    quat_R(qc, Rc);
    int h = 0;
    for (int a = 0; a < Rn; ++a) for (int b = 0; b < Rn; ++b) for (int cc = 0; cc < Rn; ++cc) {
        const double r[3] = { rs * (a - rot_k), rs * (b - rot_k), rs * (cc - rot_k) };
        const double th = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        double qd[4] = { 0, 0, 0, 1 };
        if (th > 0) {
            const double s = std::sin(0.5 * th) / th;
            qd[0] = s * r[0]; qd[1] = s * r[1]; qd[2] = s * r[2]; qd[3] = std::cos(0.5 * th);
        }
        /* q = qc (x) qd, Hamilton product */
        double q[4] = { qc[3] * qd[0] + qc[0] * qd[3] + qc[1] * qd[2] - qc[2] * qd[1],
                        qc[3] * qd[1] - qc[0] * qd[2] + qc[1] * qd[3] + qc[2] * qd[0],
                        qc[3] * qd[2] + qc[0] * qd[1] - qc[1] * qd[0] + qc[2] * qd[3],
                        qc[3] * qd[3] - qc[0] * qd[0] - qc[1] * qd[1] - qc[2] * qd[2] };
        const double qn = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
        const double sg = q[3] < 0 ? -1.0 : 1.0;
        for (int i = 0; i < 4; ++i) q[i] = sg * (q[i] / qn);
        double Rd[9], dp[3], u[3], base[3];
        quat_R(qd, Rd);
        matvec(Rd, pv, dp);
        for (int i = 0; i < 3; ++i) u[i] = pv[i] - dp[i];
        matvec(Rc, u, base);
        for (int d = 0; d < Tn; ++d) for (int e = 0; e < Tn; ++e) for (int f = 0; f < Tn; ++f, ++h) {
            const double o[3] = { ts * (d - trans_k), ts * (e - trans_k), ts * (f - trans_k) };
            float* out = poses7_out + 7 * (size_t)h;
            for (int i = 0; i < 3; ++i) out[i] = (float)(base[i] + tc[i] + o[i]);
            for (int i = 0; i < 4; ++i) out[3 + i] = (float)q[i];
        }
    }
    return GSDF_OK;
}

/* host only: the run with the smallest E / count among the eligible ones */
int gsdf_align_best(int m, const int* converged, const int* passes, const float* last36, int64_t min_count, int require_converged,
                    int* best) {
    if (m < 1 || !converged || !passes || !last36 || !best) return fail(GSDF_ERR_INVALID, "gsdf_align_best: bad argument");
    int pick = -1;
    double score = 0.0;
    for (int h = 0; h < m; ++h) {
        const float E = last36[36 * (size_t)h], count = last36[36 * (size_t)h + 28];
        if (passes[h] <= 0 || (require_converged && !converged[h])) continue;
        if (!((double)count >= (double)min_count) || !(count > 0.f) || !std::isfinite(E)) continue;   /* no hit: E / count is no score */
        const double s = (double)E / (double)count;
        if (pick < 0 || s < score) { pick = h; score = s; }
    }
    *best = pick;
    return GSDF_OK;
}

/* ---- the robust registration: the four entries above with a loss's weight on every term (gsdf_align_loss.h) ---- */
int gsdf_align_loss_weight(int loss, float scale, float phi, float* w) {
    if (!w || !gsdf_align_loss_valid(loss, scale)) return fail(GSDF_ERR_INVALID, "gsdf_align_loss_weight: bad loss, scale or a null w");
    *w = gsdf_align_weight(loss, scale, phi);
    return GSDF_OK;
}

static int align_loss_check(int loss, float scale) {
    if (loss < 0 || loss > 4) return fail(GSDF_ERR_INVALID, "gsdf_align_points_robust: loss outside 0 .. 4");
    if (!gsdf_align_loss_valid(loss, scale)) return fail(GSDF_ERR_INVALID, "gsdf_align_points_robust: the scale is not finite and > 0");
    return GSDF_OK;
}

int gsdf_align_points_robust_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float pose7[7], int num_iterations, float conv_threshold,
                                 float damping, int loss, float scale, int* converged, int* passes, float* trace38) {
    GSDF_FLUSH(c);
    if (int rc = align_points_check(c, pts_dev, n, pose7, num_iterations, converged, passes)) return rc;
    if (int rc = align_loss_check(loss, scale)) return rc;
    *converged = 0; *passes = 0;
    if (num_iterations == 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    return align_points_impl(c, pts_dev, n, pose7, num_iterations, conv_threshold, damping, converged, passes, trace38, loss, scale);
}

int gsdf_align_points_robust(gsdf_ctx* c, const float* pts_host, int64_t n, float pose7[7], int num_iterations, float conv_threshold,
                             float damping, int loss, float scale, int* converged, int* passes, float* trace38) {
    GSDF_FLUSH(c);
    if (int rc = align_points_check(c, pts_host, n, pose7, num_iterations, converged, passes)) return rc;
    if (int rc = align_loss_check(loss, scale)) return rc;
    *converged = 0; *passes = 0;
    if (num_iterations == 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev<void> big;
    float* d = nullptr;
    if (int rc = batch_scratch(c, (size_t)n * 3 * sizeof(float), big, (void**)&d)) return rc;
    if (n > 0) HIP_TRY(hipMemcpyAsync(d, pts_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return align_points_impl(c, d, n, pose7, num_iterations, conv_threshold, damping, converged, passes, trace38, loss, scale);
}

int gsdf_align_points_multi_robust_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float* poses7, int m, int num_iterations,
                                       float conv_threshold, float damping, int loss, float scale, int* converged, int* passes,
                                       float* last38, float* trace38) {
    GSDF_FLUSH(c);
    if (int rc = align_multi_check(c, pts_dev, n, poses7, m, num_iterations, converged, passes)) return rc;
    if (int rc = align_loss_check(loss, scale)) return rc;
    if (num_iterations == 0) return align_multi_none(m, converged, passes, last38, 38);
    HIP_TRY(hipSetDevice(c->device));
    return align_multi_impl(c, pts_dev, n, poses7, m, num_iterations, conv_threshold, damping, converged, passes, last38, trace38, loss,
                            scale);
}

int gsdf_align_points_multi_robust(gsdf_ctx* c, const float* pts_host, int64_t n, float* poses7, int m, int num_iterations,
                                   float conv_threshold, float damping, int loss, float scale, int* converged, int* passes,
                                   float* last38, float* trace38) {
    GSDF_FLUSH(c);
    if (int rc = align_multi_check(c, pts_host, n, poses7, m, num_iterations, converged, passes)) return rc;
    if (int rc = align_loss_check(loss, scale)) return rc;
    if (num_iterations == 0) return align_multi_none(m, converged, passes, last38, 38);
    HIP_TRY(hipSetDevice(c->device));
    gsdf_dev<void> big;
    float* d = nullptr;
    if (int rc = batch_scratch(c, (size_t)n * 3 * sizeof(float), big, (void**)&d)) return rc;
    if (n > 0) HIP_TRY(hipMemcpyAsync(d, pts_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return align_multi_impl(c, d, n, poses7, m, num_iterations, conv_threshold, damping, converged, passes, last38, trace38, loss, scale);
}

/* host only: the run with the smallest E / wsum among the eligible ones */
int gsdf_align_best_robust(int m, const int* converged, const int* passes, const float* last38, float min_wsum, int require_converged,
                           int* best) {
    if (m < 1 || !converged || !passes || !last38 || !best) return fail(GSDF_ERR_INVALID, "gsdf_align_best_robust: bad argument");
    int pick = -1;
    double score = 0.0;
    for (int h = 0; h < m; ++h) {
        const float E = last38[38 * (size_t)h], wsum = last38[38 * (size_t)h + 36];
        if (passes[h] <= 0 || (require_converged && !converged[h])) continue;
        if (!(wsum >= min_wsum) || !(wsum > 0.f) || !std::isfinite(E)) continue;   /* no weight: E / wsum is no score */
        const double s = (double)E / (double)wsum;
        if (pick < 0 || s < score) { pick = h; score = s; }
    }
    *best = pick;
    return GSDF_OK;
}

/* what a pass from pose7 sees per point; pts_dev == nullptr: the points are staged from pts_host */
static int align_residuals_impl(gsdf_ctx* c, const float* pts_host, const float* pts_dev, int64_t n, const float* pose7, float* phi_out,
                                float* w_out) {
    if (!c || !pose7) return fail(GSDF_ERR_INVALID, "gsdf_align_residuals: null argument");
    if (n < 0) return fail(GSDF_ERR_INVALID, "gsdf_align_residuals: negative n");
    if (n > 0 && ((!pts_host && !pts_dev) || !phi_out || !w_out)) return fail(GSDF_ERR_INVALID, "gsdf_align_residuals: null points or outputs");
    if (c->map_type == GSDF_MAP_BASE)
        return fail(GSDF_ERR_INVALID, "gsdf_align_residuals: not available on a base-sdf context (it reads the stored gradient)");
    if (n == 0) return GSDF_OK;
    HIP_TRY(hipSetDevice(c->device));
    const size_t un = (size_t)n;
    gsdf_dev<void> big;
    float* d = nullptr;
    if (int rc = batch_scratch(c, un * (pts_dev ? 2 : 5) * sizeof(float), big, (void**)&d)) return rc;
    float *dphi = d, *dw = d + un;
    if (!pts_dev) {
        HIP_TRY(hipMemcpyAsync(d + 2 * un, pts_host, un * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        pts_dev = d + 2 * un;
    }
    gsdf_launch_align_residuals(c->stream, c->tab, c->voxel_size, c->voxel_size_inv, pts_dev, n, pose7, dphi, dw);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(phi_out, dphi, un * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(w_out, dw, un * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_align_residuals(gsdf_ctx* c, const float* pts_host, int64_t n, const float pose7[7], float* phi_out, float* w_out) {
    GSDF_FLUSH(c);
    return align_residuals_impl(c, pts_host, nullptr, n, pose7, phi_out, w_out);
}

int gsdf_align_residuals_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, const float pose7[7], float* phi_out, float* w_out) {
    GSDF_FLUSH(c);
    return align_residuals_impl(c, nullptr, pts_dev, n, pose7, phi_out, w_out);
}

/* MapGradPixelSdf::extract_pc's rows (MapGradPixelSdf.cpp:182-195) into `out_dev` (rows_dev != nullptr) or `rows_host` */
static int surface_cloud_impl(gsdf_ctx* c, float* rows_host, float* rows_dev, int64_t max_n, int64_t* n_out) {
    if (!c || !n_out || max_n < 0) return fail(GSDF_ERR_INVALID, "gsdf_surface_cloud: bad argument");
    if (c->map_type == GSDF_MAP_BASE)
        return fail(GSDF_ERR_INVALID, "gsdf_surface_cloud: not available on a base-sdf context (extract_pc is MapGradPixelSdf's)");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long cnt = 0;
    HIP_TRY(gsdf_counted(c, [&] { gsdf_launch_surface_flag(c->stream, c->tab, c->n_slots, c->voxel_size, nullptr, nullptr, c->counter, 0); }, &cnt));
    *n_out = (int64_t)cnt;
    if (cnt == 0 || max_n == 0 || (!rows_host && !rows_dev)) return GSDF_OK;      /* nothing to write; the sizing call */
    if ((int64_t)cnt > max_n) return fail(GSDF_ERR_INVALID, "gsdf_surface_cloud: max_n too small (*n holds the need)");
    const size_t n = (size_t)cnt;
    gsdf_dev<unsigned long long> ukeys, skeys;
    gsdf_dev<uint32_t> uslots, sslots;
    gsdf_dev<float> rows;
    gsdf_dev<void> tmp;
    HIP_TRY(ukeys.alloc(n));
    HIP_TRY(skeys.alloc(n));
    HIP_TRY(uslots.alloc(n));
    HIP_TRY(sslots.alloc(n));
    if (!rows_dev) HIP_TRY(rows.alloc(n * 6));
    size_t need = 0;
    HIP_TRY(gsdf_sort_pairs_u64_need(n, &need));
    HIP_TRY(tmp.alloc(need));
    HIP_TRY(gsdf_counter_zero(c));
    gsdf_launch_surface_flag(c->stream, c->tab, c->n_slots, c->voxel_size, ukeys, uslots, c->counter, (long long)n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(gsdf_sort_pairs_u64(tmp, ukeys, skeys, uslots, sslots, n, c->stream));
    float* out = rows_dev ? rows_dev : rows.get();
    gsdf_launch_surface_rows(c->stream, c->tab, c->voxel_size, skeys, sslots, n, out);
    HIP_TRY(hipGetLastError());
    if (rows_host) HIP_TRY(hipMemcpyAsync(rows_host, out, n * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_surface_cloud(gsdf_ctx* c, float* rows6_host, int64_t max_n, int64_t* n) {
    GSDF_FLUSH(c);
    return surface_cloud_impl(c, rows6_host, nullptr, max_n, n);
}

int gsdf_surface_cloud_dev(gsdf_ctx* c, float* rows6_dev, int64_t max_n, int64_t* n) {
    GSDF_FLUSH(c);
    return surface_cloud_impl(c, nullptr, rows6_dev, max_n, n);
}

static int raycast_enqueue(gsdf_ctx* c, const float K[9], const float R[9], const float t[3], int W, int H, float zmin, float zmax,
                           float* depth_dev, float* normals_dev) {
    gsdf_pose_arg pose;
    std::memcpy(pose.R, R, sizeof(pose.R));
    std::memcpy(pose.t, t, sizeof(pose.t));
    /* per-workgroup counter rows (samples, records): sized for the largest grid seen, kept until reset */
    const size_t n_wg = (size_t)((W + 15) / 16) * (size_t)((H + 15) / 16);
    if (n_wg * 8 > c->rc_counts.count()) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        HIP_TRY(alloc_zeroed(c->rc_counts, n_wg * 8, c->stream));
    }
    if (c->occ_dirty) {                                       /* the map changed since the filters were built */
        gsdf_launch_occ_rebuild(c->stream, c->tab);
        c->occ_dirty = false;
    }
    prof_scope ps(c, 3);
    gsdf_launch_raycast(c->stream, c->tab, c->voxel_size, c->voxel_size_inv, c->factor, W, H, K, pose, zmin, zmax, depth_dev,
                        normals_dev, c->rc_counts, c->debug & 0xFFFF);
    return GSDF_OK;
}

int gsdf_raycast_dev(gsdf_ctx* c, const float K[9], const float R[9], const float t[3], int W, int H, float zmin, float zmax,
                     float* depth_dev, float* normals_dev) {
    GSDF_FLUSH(c);
    if (!c || !K || !R || !t || !depth_dev) return fail(GSDF_ERR_INVALID, "null argument");
    if (W <= 0 || H <= 0 || !(zmax > zmin) || !(zmin > 0.f)) return fail(GSDF_ERR_INVALID, "W,H > 0 and 0 < zmin < zmax required");
    HIP_TRY(hipSetDevice(c->device));
    int rc = raycast_enqueue(c, K, R, t, W, H, zmin, zmax, depth_dev, normals_dev);
    if (rc) return rc;
    HIP_TRY(hipGetLastError());
    return GSDF_OK;
}

int gsdf_raycast(gsdf_ctx* c, const float K[9], const float R[9], const float t[3], int W, int H, float zmin, float zmax,
                 float* depth_out, float* normals_out) {
    GSDF_FLUSH(c);
    if (!c || !K || !R || !t || !depth_out) return fail(GSDF_ERR_INVALID, "null argument");
    if (W <= 0 || H <= 0 || !(zmax > zmin) || !(zmin > 0.f)) return fail(GSDF_ERR_INVALID, "W,H > 0 and 0 < zmin < zmax required");
    HIP_TRY(hipSetDevice(c->device));
    const size_t N = (size_t)W * H;
    gsdf_dev<float> d;
    HIP_TRY(d.alloc(4 * N));
    if (int rc = raycast_enqueue(c, K, R, t, W, H, zmin, zmax, d, normals_out ? d + N : nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(depth_out, d, N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (normals_out) HIP_TRY(hipMemcpyAsync(normals_out, d + N, 3 * N * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_raycast_counters(gsdf_ctx* c, int64_t* samples, int64_t* records, int reset) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long tot[4] = { 0, 0, 0, 0 };
    if (c->rc_counts) {
        std::vector<unsigned long long> h(c->rc_counts.count());
        HIP_TRY(hipMemcpyAsync(h.data(), c->rc_counts, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < h.size() / 8; ++i) for (int k = 0; k < 4; ++k) tot[k] += h[8 * i + k];
        if (reset) HIP_TRY(hipMemsetAsync(c->rc_counts, 0, h.size() * sizeof(unsigned long long), c->stream));
    }
    if (samples) *samples = (int64_t)tot[0];
    if (records) *records = (int64_t)tot[1];
    c->rc_iters[0] = (long long)tot[2]; c->rc_iters[1] = (long long)tot[3];
    return GSDF_OK;
}

int gsdf_extract_mesh(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16], float* triangles_out, int64_t max_tris,
                      int64_t* n_tris) {
    GSDF_FLUSH(c);
    if (!c || !n_tris || (max_tris > 0 && !triangles_out)) return fail(GSDF_ERR_INVALID, "null argument");
    if (!tri_table) tri_table = GSDF_MC_TRI_TABLE;            /* the reference's triTable (LayeredMarchingCubesNoColor.cpp:96-352) */
    HIP_TRY(hipSetDevice(c->device));
    *n_tris = 0;
    /* upper bound of the output: 5 triangles per cube, one cube per voxel; sized by the caller through max_tris */
    const long long cap = max_tris > 0 ? (long long)max_tris : 0;
    gsdf_dev<int> d_mn;
    gsdf_dev<signed char> d_tab;
    gsdf_dev<float> d_tris;
    gsdf_dev<unsigned long long> d_keys;
    HIP_TRY(d_mn.alloc(3));
    HIP_TRY(d_tab.alloc(256 * 16));
    if (cap) HIP_TRY(d_tris.alloc((size_t)cap * 9));
    if (cap) HIP_TRY(d_keys.alloc((size_t)cap));
    const int big[3] = { 2147483647, 2147483647, 2147483647 };
    HIP_TRY(hipMemcpyAsync(d_mn, big, sizeof(big), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_tab, tri_table, 256 * 16, hipMemcpyHostToDevice, c->stream));
    unsigned long long n = 0;
    HIP_TRY(gsdf_counted(c, [&] { gsdf_launch_mesh(c->stream, c->tab, c->n_slots, c->voxel_size, iso, d_mn, d_tab, d_tris, d_keys, c->counter, cap); }, &n));
    const size_t got = (size_t)std::min<unsigned long long>(n, (unsigned long long)cap);
    /* the reference's order (z-y-x sweep, triangles of a cube in table order) = ascending sort key: radix sort of (key, index)
     * on the device, the triangles gathered into that order on the device, ONE copy of the sorted list to the caller */
    if (got && n <= (unsigned long long)cap) {
        gsdf_key_order ord;
        gsdf_dev<float> d_sorted;
        HIP_TRY(ord.alloc(got));
        HIP_TRY(d_sorted.alloc(got * 9));
        HIP_TRY(ord.run(c, d_keys, got));
        gsdf_launch_gather_tris(c->stream, d_tris, ord.order, d_sorted, got);
        HIP_TRY(hipMemcpyAsync(triangles_out, d_sorted, got * 9 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *n_tris = (int64_t)n;                                    /* total found, also when it exceeds max_tris */
    if (n > (unsigned long long)cap) return cap ? fail(GSDF_ERR_INVALID, "gsdf_extract_mesh: max_tris too small (n_tris holds the need)") : GSDF_OK;
    return GSDF_OK;
}

/* The steps are listed at the head of gsdf_mesh_index.hip.  The counting pass is gsdf_extract_mesh's own sizing pass (k_mesh_bbox
 * + k_mesh with no room): it leaves the bounding-box minimum on the device and the triangle count, so the corner pass runs once,
 * into buffers of the exact size, whatever the caller's maxima are -- the vertex count is known only after the weld, and it is
 * reported also when the caller's buffers are too small.
 *
 * indexed_mesh_dev is the device part, shared by gsdf_extract_mesh_indexed and the entries that work on the welded arrays
 * (gsdf_mesh_components, gsdf_extract_mesh_indexed_filtered): indexed_mesh_count runs up to the vertex count and synchronises,
 * indexed_mesh_weld enqueues the weld and the normals and leaves faces / v / n on the device. */
namespace {
struct indexed_mesh_dev {
    gsdf_dev<int> mn;
    gsdf_dev<signed char> tab;
    gsdf_dev<float> tris, v, n;
    gsdf_dev<unsigned long long> keys, ekeys, ck, ck2, vkeys;
    gsdf_dev<uint32_t> muw, rank, rank2, heads, before, vmuw;
    gsdf_dev<int32_t> faces;
    gsdf_key_order soup;                                       /* the soup's order; its scratch also serves the corner sort and the heads scan */
    size_t nt = 0, nc = 0, nv = 0;                             /* faces, corners, vertices */
};

int indexed_mesh_count(gsdf_ctx* c, float iso, const int8_t* tri_table, const char* who, indexed_mesh_dev& m) {
    m.nt = m.nc = m.nv = 0;
    HIP_TRY(m.mn.alloc(3));
    HIP_TRY(m.tab.alloc(256 * 16));
    const int big[3] = { 2147483647, 2147483647, 2147483647 };
    HIP_TRY(hipMemcpyAsync(m.mn, big, sizeof(big), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(m.tab, tri_table, 256 * 16, hipMemcpyHostToDevice, c->stream));
    unsigned long long n = 0, n2 = 0;
    HIP_TRY(gsdf_counted(c, [&] { gsdf_launch_mesh(c->stream, c->tab, c->n_slots, c->voxel_size, iso, m.mn, m.tab, nullptr, nullptr, c->counter, 0); }, &n));
    if (n == 0) return GSDF_OK;
    if (n > 2147483647ull / 3)
        return fail(GSDF_ERR_INVALID, std::string(who) + ": more than (2^31 - 1) / 3 triangles (vertex ids and corner ranks are 32-bit)");
    const size_t nt = (size_t)n, nc = 3 * nt;
    HIP_TRY(m.tris.alloc(nt * 9));
    HIP_TRY(m.keys.alloc(nt));
    HIP_TRY(m.ekeys.alloc(nc));
    HIP_TRY(m.muw.alloc(nc));
    HIP_TRY(m.ck.alloc(nc));
    HIP_TRY(m.ck2.alloc(nc));
    HIP_TRY(m.rank.alloc(nc));
    HIP_TRY(m.rank2.alloc(nc));
    HIP_TRY(m.heads.alloc(nc));
    HIP_TRY(m.before.alloc(nc));
    size_t need = 0;
    HIP_TRY(gsdf_sort_pairs_u64_need(nc, &need));
    HIP_TRY(gsdf_run_heads_scan_need(nc, &need));
    HIP_TRY(m.soup.alloc(nt, need));
    HIP_TRY(gsdf_counter_zero(c));
    gsdf_launch_mesh_corners(c->stream, c->tab, c->n_slots, c->voxel_size, iso, m.mn, m.tab, m.tris, m.keys, m.ekeys, m.muw, c->counter,
                             (long long)nt);
    HIP_TRY(gsdf_counter_read(c, &n2));
    /* the soup's order, then the weld: stable sort of (edge key, corner rank), run starts, their scan */
    HIP_TRY(m.soup.run(c, m.keys, nt));
    gsdf_launch_corner_keys(c->stream, m.ekeys, m.soup.order, m.ck, m.rank, nt);
    HIP_TRY(gsdf_sort_pairs_u64(m.soup.tmp, m.ck, m.ck2, m.rank, m.rank2, nc, c->stream));
    HIP_TRY(gsdf_run_heads_scan(m.soup.tmp, m.ck2, m.heads, m.before, nc, c->stream));
    uint32_t last[2] = { 0u, 0u };
    HIP_TRY(gsdf_scan_total_read(c->stream, m.before, m.heads, nc, last));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n2 != n) return fail(GSDF_ERR_HIP, std::string(who) + ": the map changed between the counting and the corner pass");
    m.nt = nt; m.nc = nc; m.nv = (size_t)last[0] + last[1];
    return GSDF_OK;
}

int indexed_mesh_weld(gsdf_ctx* c, bool normals, indexed_mesh_dev& m) {
    HIP_TRY(m.faces.alloc(m.nc));
    HIP_TRY(m.v.alloc(m.nv * 3));
    HIP_TRY(m.vkeys.alloc(m.nv));
    HIP_TRY(m.vmuw.alloc(m.nv));
    if (normals) HIP_TRY(m.n.alloc(m.nv * 3));
    gsdf_launch_weld(c->stream, m.ck2, m.rank2, m.heads, m.before, m.soup.order, m.tris, m.muw, m.nc, m.faces, m.v, m.vkeys, m.vmuw);
    if (normals) gsdf_launch_vertex_normals(c->stream, c->tab, m.mn, m.vkeys, m.vmuw, m.nv, m.n);
    HIP_TRY(hipGetLastError());
    return GSDF_OK;
}
} // namespace

int gsdf_extract_mesh_indexed(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16], float* vertices_out, float* normals_out,
                              int32_t* faces_out, int64_t max_vertices, int64_t max_faces, int64_t* n_vertices, int64_t* n_faces) {
    GSDF_FLUSH(c);
    if (!c || !n_vertices || !n_faces || (max_vertices > 0 && !vertices_out) || (max_faces > 0 && !faces_out))
        return fail(GSDF_ERR_INVALID, "null argument");
    if (!tri_table) tri_table = GSDF_MC_TRI_TABLE;
    HIP_TRY(hipSetDevice(c->device));
    *n_vertices = 0; *n_faces = 0;
    indexed_mesh_dev m;
    if (int rc = indexed_mesh_count(c, iso, tri_table, "gsdf_extract_mesh_indexed", m)) return rc;
    if (m.nt == 0) return GSDF_OK;
    const size_t nv = m.nv, nt = m.nt, nc = m.nc;
    *n_vertices = (int64_t)nv; *n_faces = (int64_t)nt;
    if (max_vertices == 0 && max_faces == 0) return GSDF_OK;                    /* the sizing call */
    if ((int64_t)nv > max_vertices || (int64_t)nt > max_faces)
        return fail(GSDF_ERR_INVALID, "gsdf_extract_mesh_indexed: max_vertices or max_faces too small (n_vertices / n_faces hold the need)");
    if (int rc = indexed_mesh_weld(c, normals_out != nullptr, m)) return rc;
    HIP_TRY(hipMemcpyAsync(vertices_out, m.v, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(faces_out, m.faces, nc * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (normals_out) HIP_TRY(hipMemcpyAsync(normals_out, m.n, nv * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

/* The components of the welded mesh (steps at the head of gsdf_mesh_components.hip), shared by gsdf_mesh_components and
 * gsdf_extract_mesh_indexed_filtered: labels, ids, and -- where asked for -- the tables.  Synchronises once, for the count. */
namespace {
struct mesh_components_dev {
    gsdf_dev<uint32_t> parent, root, flags, before, box_bits;
    gsdf_dev<int32_t> vcomp, fcomp, counts;
    gsdf_dev<float> box;
    gsdf_dev<void> tmp;
    size_t n_comp = 0;
};

int mesh_components_label(gsdf_ctx* c, const indexed_mesh_dev& m, bool boxes, mesh_components_dev& cc) {
    const size_t nv = m.nv, nt = m.nt;
    HIP_TRY(cc.parent.alloc(nv));
    HIP_TRY(cc.root.alloc(nv));
    HIP_TRY(cc.flags.alloc(std::max(nv, nt)));                  /* reused for the keep flags of vertices, then of faces */
    HIP_TRY(cc.before.alloc(nv));
    HIP_TRY(cc.vcomp.alloc(nv));
    HIP_TRY(cc.fcomp.alloc(nt));
    size_t need = 0;
    HIP_TRY(gsdf_scan_u32_need(std::max(nv, nt), &need));
    HIP_TRY(cc.tmp.alloc(need));
    gsdf_launch_cc_label(c->stream, m.faces, nt, nv, cc.parent, cc.root, cc.flags);
    HIP_TRY(gsdf_scan_u32(cc.tmp, cc.flags, cc.before, nv, c->stream));
    uint32_t last[2] = { 0u, 0u };
    HIP_TRY(gsdf_scan_total_read(c->stream, cc.before, cc.flags, nv, last));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    cc.n_comp = (size_t)last[0] + last[1];
    HIP_TRY(cc.counts.alloc(cc.n_comp * 2));
    if (boxes) { HIP_TRY(cc.box_bits.alloc(cc.n_comp * 6)); HIP_TRY(cc.box.alloc(cc.n_comp * 6)); }
    gsdf_launch_cc_tables(c->stream, m.faces, m.v, cc.root, cc.before, nt, nv, cc.n_comp, cc.vcomp, cc.fcomp, cc.counts,
                          boxes ? cc.box_bits.get() : nullptr, boxes ? cc.box.get() : nullptr);
    HIP_TRY(hipGetLastError());
    return GSDF_OK;
}
} // namespace

int gsdf_mesh_components(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16], int32_t* vertex_comp, int32_t* face_comp,
                         int64_t max_vertices, int64_t max_faces, int32_t* comp_counts, float* comp_bbox, int64_t max_components,
                         int64_t* n_vertices, int64_t* n_faces, int64_t* n_components) {
    GSDF_FLUSH(c);
    if (!c || !n_vertices || !n_faces || !n_components) return fail(GSDF_ERR_INVALID, "null argument");
    if (max_vertices < 0 || max_faces < 0 || max_components < 0) return fail(GSDF_ERR_INVALID, "gsdf_mesh_components: a negative maximum");
    if (!tri_table) tri_table = GSDF_MC_TRI_TABLE;
    HIP_TRY(hipSetDevice(c->device));
    *n_vertices = 0; *n_faces = 0; *n_components = 0;
    indexed_mesh_dev m;
    if (int rc = indexed_mesh_count(c, iso, tri_table, "gsdf_mesh_components", m)) return rc;
    if (m.nt == 0) return GSDF_OK;
    if (int rc = indexed_mesh_weld(c, false, m)) return rc;
    mesh_components_dev cc;
    if (int rc = mesh_components_label(c, m, comp_bbox != nullptr, cc)) return rc;
    const size_t nv = m.nv, nt = m.nt, ncomp = cc.n_comp;
    *n_vertices = (int64_t)nv; *n_faces = (int64_t)nt; *n_components = (int64_t)ncomp;
    if (max_vertices == 0 && max_faces == 0 && max_components == 0) {           /* the sizing call */
        HIP_TRY(hipStreamSynchronize(c->stream));
        return GSDF_OK;
    }
    if ((vertex_comp && (int64_t)nv > max_vertices) || (face_comp && (int64_t)nt > max_faces) ||
        ((comp_counts || comp_bbox) && (int64_t)ncomp > max_components)) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        return fail(GSDF_ERR_INVALID, "gsdf_mesh_components: max_vertices, max_faces or max_components too small (the counts hold the need)");
    }
    if (vertex_comp) HIP_TRY(hipMemcpyAsync(vertex_comp, cc.vcomp, nv * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (face_comp) HIP_TRY(hipMemcpyAsync(face_comp, cc.fcomp, nt * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (comp_counts) HIP_TRY(hipMemcpyAsync(comp_counts, cc.counts, ncomp * 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (comp_bbox) HIP_TRY(hipMemcpyAsync(comp_bbox, cc.box, ncomp * 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_extract_mesh_indexed_filtered(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16], int64_t min_faces, float* vertices_out,
                                       float* normals_out, int32_t* faces_out, int64_t max_vertices, int64_t max_faces,
                                       int64_t* n_vertices, int64_t* n_faces, int64_t* n_components, int64_t* n_kept) {
    GSDF_FLUSH(c);
    if (!c || !n_vertices || !n_faces || !n_components || !n_kept || (max_vertices > 0 && !vertices_out) || (max_faces > 0 && !faces_out))
        return fail(GSDF_ERR_INVALID, "null argument");
    if (min_faces < 1 && min_faces != GSDF_MESH_KEEP_LARGEST)
        return fail(GSDF_ERR_INVALID, "gsdf_extract_mesh_indexed_filtered: min_faces must be >= 1 or GSDF_MESH_KEEP_LARGEST");
    if (!tri_table) tri_table = GSDF_MC_TRI_TABLE;
    HIP_TRY(hipSetDevice(c->device));
    *n_vertices = 0; *n_faces = 0; *n_components = 0; *n_kept = 0;
    indexed_mesh_dev m;
    if (int rc = indexed_mesh_count(c, iso, tri_table, "gsdf_extract_mesh_indexed_filtered", m)) return rc;
    if (m.nt == 0) return GSDF_OK;
    const bool sizing = max_vertices == 0 && max_faces == 0;
    if (int rc = indexed_mesh_weld(c, normals_out != nullptr && !sizing, m)) return rc;
    mesh_components_dev cc;
    if (int rc = mesh_components_label(c, m, false, cc)) return rc;
    const size_t nv = m.nv, nt = m.nt;
    /* the mask over the components, then per vertex and per face; the exclusive scans of the two are the new ids */
    gsdf_dev<uint32_t> d_keep, d_kept, d_vbefore, d_fflags, d_fbefore;
    HIP_TRY(d_keep.alloc(cc.n_comp));
    HIP_TRY(d_kept.alloc(1));
    HIP_TRY(d_vbefore.alloc(nv));
    HIP_TRY(d_fflags.alloc(nt));
    HIP_TRY(d_fbefore.alloc(nt));
    uint32_t* d_vflags = cc.flags;                                              /* the root flags have been scanned: reuse */
    gsdf_launch_cc_keep(c->stream, cc.counts, cc.n_comp, (long long)min_faces, d_keep, d_kept);
    gsdf_launch_cc_keep_flags(c->stream, cc.vcomp, d_keep, nv, d_vflags);
    gsdf_launch_cc_keep_flags(c->stream, cc.fcomp, d_keep, nt, d_fflags);
    HIP_TRY(gsdf_scan_u32(cc.tmp, d_vflags, d_vbefore, nv, c->stream));
    HIP_TRY(gsdf_scan_u32(cc.tmp, d_fflags, d_fbefore, nt, c->stream));
    uint32_t h[5] = { 0u, 0u, 0u, 0u, 0u };
    HIP_TRY(hipMemcpyAsync(&h[0], d_kept, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(gsdf_scan_total_read(c->stream, d_vbefore, d_vflags, nv, &h[1]));
    HIP_TRY(gsdf_scan_total_read(c->stream, d_fbefore, d_fflags, nt, &h[3]));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    const size_t kv = (size_t)h[1] + h[2], kf = (size_t)h[3] + h[4];
    *n_vertices = (int64_t)kv; *n_faces = (int64_t)kf; *n_components = (int64_t)cc.n_comp; *n_kept = (int64_t)h[0];
    if (sizing) return GSDF_OK;
    if ((int64_t)kv > max_vertices || (int64_t)kf > max_faces)
        return fail(GSDF_ERR_INVALID,
                    "gsdf_extract_mesh_indexed_filtered: max_vertices or max_faces too small (n_vertices / n_faces hold the need)");
    if (kf == 0) return GSDF_OK;
    gsdf_dev<float> d_vo, d_no;
    gsdf_dev<int32_t> d_fo;
    HIP_TRY(d_vo.alloc(kv * 3));
    if (normals_out) HIP_TRY(d_no.alloc(kv * 3));
    HIP_TRY(d_fo.alloc(kf * 3));
    gsdf_launch_cc_compact(c->stream, m.v, normals_out ? m.n.get() : nullptr, m.faces, d_vflags, d_vbefore, d_fflags, d_fbefore, nv, nt, d_vo,
                           normals_out ? d_no.get() : nullptr, d_fo);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(vertices_out, d_vo, kv * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(faces_out, d_fo, kf * 3 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (normals_out) HIP_TRY(hipMemcpyAsync(normals_out, d_no, kv * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

int gsdf_block_keys_dev(gsdf_ctx* c, uint64_t* keys_dev, int64_t max_n, int64_t* n) {
    GSDF_FLUSH(c);
    if (!c || !n || (max_n > 0 && !keys_dev)) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long cnt = 0;
    HIP_TRY(gsdf_counted(c, [&] { gsdf_launch_block_keys(c->stream, c->tab, c->n_slots / GSDF_BLOCK_VOX, (unsigned long long*)keys_dev, c->counter, max_n); }, &cnt));
    *n = (int64_t)cnt;
    return GSDF_OK;
}
int gsdf_pack_blocks_dev(gsdf_ctx* c, const uint64_t* block_keys_dev, int64_t n, float* dense_dev) {
    GSDF_FLUSH(c);
    if (!c || (n > 0 && (!block_keys_dev || !dense_dev))) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    gsdf_launch_pack_blocks(c->stream, c->tab, (const unsigned long long*)block_keys_dev, n, dense_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}
int gsdf_unpack_blocks_dev(gsdf_ctx* c, const uint64_t* block_keys_dev, int64_t n, const float* dense_dev) {
    GSDF_FLUSH(c);
    if (!c || (n > 0 && (!block_keys_dev || !dense_dev))) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    c->occ_dirty = true;
    gsdf_launch_unpack_blocks(c->stream, c->tab, (const unsigned long long*)block_keys_dev, n, dense_dev, c->st);
    HIP_TRY(hipGetLastError());
    return gsdf_sync(c);
}

int gsdf_dev_alloc(gsdf_ctx* c, void** dev_ptr, int64_t bytes) {
    if (!c || !dev_ptr || bytes <= 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMalloc(dev_ptr, (size_t)bytes));
    return GSDF_OK;
}
int gsdf_dev_free(gsdf_ctx* c, void* dev_ptr) {
    GSDF_FLUSH(c);
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (dev_ptr) {
        /* a hinted frame or one whose normals were computed ahead (gsdf_hint_next_depth_dev) inside the freed allocation: the
         * allocator may hand the same address out again with other contents, which the normals would not belong to */
        size_t bytes = 0;
        void* base = nullptr;
        if (hipMemGetAddressRange((hipDeviceptr_t*)&base, &bytes, (hipDeviceptr_t)dev_ptr) != hipSuccess || !base) {
            (void)hipGetLastError();
            base = dev_ptr; bytes = 1;
        }
        (void)c->ahead.range_changes(base, bytes, c->frame_bytes());   /* (a waiting fusion was launched above) */
    }
    HIP_TRY(hipFree(dev_ptr));
    return GSDF_OK;
}
int gsdf_dev_download(gsdf_ctx* c, void* host_dst, const void* dev_src, int64_t bytes) {
    GSDF_FLUSH(c);
    if (!c || !host_dst || !dev_src || bytes < 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(host_dst, dev_src, (size_t)bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}
int gsdf_dev_upload(gsdf_ctx* c, void* dev_dst, const void* host_src, int64_t bytes) {
    if (!c || !dev_dst || !host_src || bytes < 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = flush_if_overlaps(c, dev_dst, bytes); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(dev_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GSDF_OK;
}

/* ---- asynchronous frame staging (Scan3D: decode on host threads -> pinned buffer -> HBM, overlapped with the GPU) ---- */
int gsdf_host_alloc(gsdf_ctx* c, void** host_ptr, int64_t bytes) {
    if (!c || !host_ptr || bytes <= 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostMalloc(host_ptr, (size_t)bytes, hipHostMallocDefault));
    return GSDF_OK;
}
int gsdf_host_free(gsdf_ctx* c, void* host_ptr) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipHostFree(host_ptr));
    return GSDF_OK;
}
int gsdf_dev_upload_async(gsdf_ctx* c, void* dev_dst, const void* host_src, int64_t bytes) {
    if (!c || !dev_dst || !host_src || bytes < 0) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = flush_if_overlaps(c, dev_dst, bytes); if (rc) return rc; }
    HIP_TRY(hipMemcpyAsync(dev_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    return GSDF_OK;
}
int gsdf_mark(gsdf_ctx* c, int64_t* mark) {
    GSDF_FLUSH(c);
    if (!c || !mark) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    /* a mark says "the stream has passed this point" -- what a staging slot's recycling needs -- and nothing about device
     * memory being visible to the host (the download entries synchronise for that): no system-scope fence, which would write
     * back and invalidate the caches between the frame's fusion and the next frame's first tracker pass */
    hipEvent_t e = nullptr;
    if (!c->mark_pool.empty()) { e = c->mark_pool.back(); c->mark_pool.pop_back(); }
    else HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence));
    HIP_TRY(hipEventRecord(e, c->stream));
    c->marks.push_back({ ++c->mark_serial, e });
    *mark = c->mark_serial;
    return GSDF_OK;
}
/* retire the marks up to `mark` (they complete in stream order); wait != 0 blocks until then */
static int marks_reached(gsdf_ctx* c, int64_t mark, int wait, int* reached) {
    *reached = 1;
    while (!c->marks.empty() && c->marks.front().first <= mark) {
        hipEvent_t e = c->marks.front().second;
        hipError_t q = wait ? hipEventSynchronize(e) : hipEventQuery(e);
        if (q == hipErrorNotReady) { *reached = 0; return GSDF_OK; }
        if (q != hipSuccess) return fail(GSDF_ERR_HIP, std::string("gsdf mark: ") + hipGetErrorString(q));
        c->mark_pool.push_back(e);
        c->marks.pop_front();
    }
    return GSDF_OK;
}
int gsdf_mark_wait(gsdf_ctx* c, int64_t mark) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    int r = 0;
    return marks_reached(c, mark, 1, &r);
}
int gsdf_mark_reached(gsdf_ctx* c, int64_t mark, int* reached) {
    if (!c || !reached) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    return marks_reached(c, mark, 0, reached);
}

int gsdf_dev_upload_ahead(gsdf_ctx* c, void* dev_dst, const void* host_src, int64_t bytes, int64_t* upload) {
    if (!c || !dev_dst || !host_src || bytes < 0 || !upload) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    /* (a caller that keeps to the contract -- dev_dst is out of the stream's reach: its last reader passed a gsdf_mark, which
     * launched any waiting fusion -- never gets here with an overlap; the copy stream is not ordered behind the kernels) */
    if (c->ahead.range_changes(dev_dst, (size_t)bytes, c->frame_bytes()))   /* new contents: normals computed ahead are the old frame's */
        return fail(GSDF_ERR_INVALID, "gsdf_dev_upload_ahead into the depth image of a fusion that has not run yet (record a gsdf_mark "
                                      "behind its gsdf_update_dev and wait for it first)");
    if (!c->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    HIP_TRY(hipMemcpyAsync(dev_dst, host_src, (size_t)bytes, hipMemcpyHostToDevice, c->copy_stream));
    hipEvent_t e = nullptr;                                      /* (a pool of their own: these keep the default fences) */
    if (!c->upload_pool.empty()) { e = c->upload_pool.back(); c->upload_pool.pop_back(); }
    else HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(e, c->copy_stream));
    c->uploads.push_back({ ++c->upload_serial, e });
    *upload = c->upload_serial;
    return GSDF_OK;
}
int gsdf_upload_wait(gsdf_ctx* c, int64_t upload) {
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    while (!c->uploads.empty() && c->uploads.front().first <= upload) {
        hipEvent_t e = c->uploads.front().second;
        const hipError_t q = hipEventSynchronize(e);
        if (q != hipSuccess) return fail(GSDF_ERR_HIP, std::string("gsdf upload: ") + hipGetErrorString(q));
        c->upload_pool.push_back(e);
        c->uploads.pop_front();
    }
    return GSDF_OK;
}

int gsdf_timer_start(gsdf_ctx* c) {
    GSDF_FLUSH(c);
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev0, c->stream));
    return GSDF_OK;
}
int gsdf_timer_stop_ms(gsdf_ctx* c, float* ms) {
    GSDF_FLUSH(c);
    if (!c || !ms) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventRecord(c->ev1, c->stream));
    HIP_TRY(hipEventSynchronize(c->ev1));
    HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
    return GSDF_OK;
}

int gsdf_profile(gsdf_ctx* c, int enable) {
    GSDF_FLUSH(c);
    if (!c) return fail(GSDF_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_collect(c);
    c->profiling = enable != 0;
    if (enable) for (int k = 0; k < GSDF_PROF_SLOTS; ++k) { c->prof_ms[k] = 0; c->prof_n[k] = 0; c->prof_each[k].clear(); }
    return GSDF_OK;
}
int gsdf_profile_read_launches(gsdf_ctx* c, int slot, float* ms, int64_t max_n, int64_t* n) {
    if (!c || !n || slot < 0 || slot >= GSDF_PROF_SLOTS || max_n < 0 || (max_n > 0 && !ms)) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_collect(c);
    const std::vector<float>& v = c->prof_each[slot];
    *n = (int64_t)v.size();
    for (int64_t i = 0; i < std::min<int64_t>(max_n, *n); ++i) ms[i] = v[i];
    return GSDF_OK;
}
int gsdf_profile_read(gsdf_ctx* c, double ms[3], int64_t launches[3]) {
    if (!c || !ms || !launches) return fail(GSDF_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int k = 0; k < 3; ++k) { ms[k] = c->prof_ms[k]; launches[k] = c->prof_n[k]; }
    return GSDF_OK;
}
int gsdf_profile_read_n(gsdf_ctx* c, int n, double* ms, int64_t* launches) {
    if (!c || !ms || !launches || n < 0 || n > GSDF_PROF_SLOTS) return fail(GSDF_ERR_INVALID, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    prof_collect(c);
    for (int k = 0; k < n; ++k) { ms[k] = c->prof_ms[k]; launches[k] = c->prof_n[k]; }
    return GSDF_OK;
}

} // extern "C"
