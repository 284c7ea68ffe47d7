/*
 * gsdf.h -- C-ABI of the MI355X-native Gradient-SDF engine (libgsdf.so).
 *
 * This is the drop-in boundary for the hot path of c-sommer/gradient-sdf
 * (cpp/depth_scanning): per-voxel TSDF+gradient fusion, the voxel-hash point
 * query and the 6-DoF SDF-tracking normal-equation reduction.  The reference has
 * no FFI / plugin layer: its seam is two C++ virtual interfaces and one POD
 * (SURVEY.md 8b).  Every entry point below names the reference interface it
 * replaces (paths relative to /root/reference/cpp/include/).  The C++ facade in
 * gradient-sdf_amd/host/ (MapGradPixelSdf, RigidPointOptimizer, SdfVoxel) calls
 * only these functions; INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions (identical to the reference's):
 *   depth  : float32, row-major H x W, continuous, metres, 0 = invalid
 *            (cv::Mat CV_32FC1, img_loader/ImageLoader.h:159-175)
 *   K      : row-major 3x3 float  fx 0 cx; 0 fy cy; 0 0 1
 *   R, t   : camera->world, p_w = R p_c + t, R row-major (MapGradPixelSdf.cpp:62-64,103)
 *   pose7  : tx ty tz qx qy qz qw  (Sophus SE3 state; TUM file order, main_scan_3d.cpp:274-280)
 *   keys   : int32 x,y,z voxel indices (Eigen::Vector3i, MapGradPixelSdf.h:65-68)
 *   payload: float dist, gx, gy, gz, weight (struct SdfVoxel, sdf_voxel/SdfVoxel.h:45-57)
 *
 * Plain C types only, caller-owned buffers, no exceptions across the ABI.
 * One context = one GPU; a context is not thread-safe (the reference has a
 * single caller thread).  All functions return GSDF_OK (0) or a GSDF_ERR_* code;
 * gsdf_last_error() gives the message.  *_dev variants take DEVICE pointers and
 * only enqueue work on the context's HIP stream (no host synchronisation).
 */
#ifndef GSDF_H_
#define GSDF_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSDF_OK               0
#define GSDF_ERR_TABLE_FULL   1   /* the block table (or the deferred list) ran out of room (new failure mode) */
#define GSDF_ERR_KEY_RANGE    2   /* voxel index outside the packable +-2^20 range */
#define GSDF_ERR_INVALID      3   /* bad argument / call order */
#define GSDF_ERR_HIP          4   /* HIP runtime error (message in gsdf_last_error) */
#define GSDF_ERR_NO_DEVICE    5   /* no gfx950 device visible: the engine has NO CPU fallback */

typedef struct gsdf_ctx gsdf_ctx;

/* counters of the fusion / tracking launches (for algorithmic-bytes accounting: callers take differences) */
typedef struct gsdf_stats {
    int64_t n_upd;        /* (pixel,k) samples with w>0, summed over every update() since create/reset   */
    int64_t n_valid;      /* pixels that passed the z-range and both normal gates, summed likewise       */
    int64_t n_hit;        /* sum over executed tracker passes of pixels with w0>0       */
    int32_t track_passes; /* tracker reduction passes executed in the last optimize()   */
    int32_t converged;    /* result of the last optimize()                              */
    int64_t frames;       /* Sdf::counter_ (Sdf.h:65)                                   */
    int64_t n_deferred;   /* voxel contributions that took the deferred (float-atomic) route of the fusion flush
                             since create/reset: near tiles, LDS overflow, timed-out waits (0 in steady state)  */
    int64_t fuse_timeouts;/* fusion tiles whose bounded wait for a neighbouring tile expired (they deferred)     */
    int64_t far_tiles;    /* tiles of the last fusion that did not fit the small LDS table in one band; while more than
                             fuse_blocks / 16 of them, the frame entries choose the fusion kernel with the larger table  */
    int64_t fuse_blocks;  /* fusion tiles of a frame                                                             */
    int64_t fuse_launches;      /* fusion launches since create/reset (a tracked frame queues one per batch)        */
    int64_t far_table_launches; /* of those, the ones with the larger LDS table                                     */
} gsdf_stats;

const char* gsdf_last_error(void);
const char* gsdf_version(void);

/* MapGradPixelSdf(voxel_size, T) + table allocation -- MapGradPixelSdf.h:99-103, Sdf.h:103-107.
 * capacity_log2 in [10, 30]: 2^capacity_log2 32-byte voxel records, organised as 2^(capacity_log2-6) blocks of
 * 4x4x4 voxels (BASELINE configs: 22 and 25).  A surface map fills its blocks to ~70 %, so it holds about
 * 0.6 * 2^capacity_log2 voxels before GSDF_ERR_TABLE_FULL.
 * trunc_dist (T) must be below 2 m: the fusion kernel accumulates a tile's w * sdf sums in 51-bit fixed point (2^-40).
 * device: HIP device ordinal.  Fails with GSDF_ERR_NO_DEVICE when no GPU is present. */
int gsdf_create(gsdf_ctx** out, float voxel_size, float trunc_dist, int capacity_log2, int device);
/* delete tSDF -- main_scan_3d.cpp:314 */
void gsdf_destroy(gsdf_ctx* c);
/* drop all voxels, frame counter := 0 (new: lets one context be reused by bench/tests) */
int gsdf_reset(gsdf_ctx* c);
/* The reference's tsdf_ grows without bound (a node hash map, MapGradPixelSdf.h:65-68); this table has a capacity.  gsdf_grow
 * moves every block into a table of 2^new_capacity_log2 records (synchronous; the map -- voxels, vis_ bit-vectors, frame counter
 * -- is unchanged, only the room differs; on failure the old table stays; a sticky GSDF_ERR_TABLE_FULL from an earlier fusion
 * does not stop it, but stays reported: that fusion's samples were dropped).  gsdf_set_auto_grow lets the frame entries
 * (gsdf_update_dev / gsdf_update / gsdf_track_and_fuse_dev) do that by themselves: the table is doubled when ~45 % of its block
 * entries are in use, up to max_capacity_log2; 0 switches it off, which is the default -- then GSDF_ERR_TABLE_FULL reports a map
 * that outgrew its table, as before.  The load is counted on the device behind every frame and read without waiting; the
 * library knows how old the count it sees is and how fast the map grew lately, and an entry waits by itself (for the device to
 * come within 8 frames, or for an exact count) when count + lag x growth comes near the limit -- callers need not
 * synchronise.  What auto-grow cannot absorb: ONE frame that needs more new blocks than the table has left (more than half
 * its entries): that frame still ends in GSDF_ERR_TABLE_FULL.  Size the initial table for at least two frames' blocks.
 * gsdf_capacity reports the present capacity_log2. */
int gsdf_grow(gsdf_ctx* c, int new_capacity_log2);
int gsdf_set_auto_grow(gsdf_ctx* c, int max_capacity_log2);
int gsdf_capacity(gsdf_ctx* c, int* capacity_log2);

/* Map type -- main_scan_3d.cpp:226-233 (--scan-type): GSDF_MAP_GRAD is MapGradPixelSdf (the default, the Gradient-SDF map),
 * GSDF_MAP_BASE is MapPixelSdf (sdf_tracker/MapPixelSdf.h:52-157), the plain voxel-hash SDF the paper compares against.  Both
 * fuse the same voxels with the same weight / truncation / running mean (MapPixelSdfOmp.cpp:163-186 = MapGradPixelSdf.cpp:86-118),
 * so gsdf_update[_dev], gsdf_export, gsdf_get_voxels, gsdf_raycast*, gsdf_extract_mesh, grow and the next-frame hint are the same
 * on both.  On a base context the tracker entries (gsdf_track, gsdf_track_sampled, gsdf_track_and_fuse_dev,
 * gsdf_track_and_fuse_ahead_dev) and gsdf_query use MapPixelSdf::weights / ::tsdf (MapPixelSdf.h:108-143, interp3 at
 * MapPixelSdf.cpp:43-111): trilinear interpolation of the 8 voxels around floor(p / vs); phi = -T and grad = 0 where none of them
 * exists, phi = 0 and grad = 0 where some do, and w is the weight of the round(p / vs) voxel only when all 8 exist (else 0).
 * gsdf_ba_setup (PhotoBA needs the gradient) and gsdf_merge_from between contexts of different type are GSDF_ERR_INVALID on a
 * base context.  gsdf_merge_raw* and the multi-device merge take raw sums without a type; callers keep them to one type.
 * gsdf_set_map_type is allowed only while the map is empty (gsdf_count == 0), else GSDF_ERR_INVALID and the type stays as it
 * was; gsdf_reset keeps the type. */
#define GSDF_MAP_GRAD 0
#define GSDF_MAP_BASE 1
int gsdf_set_map_type(gsdf_ctx* c, int type);
int gsdf_get_map_type(gsdf_ctx* c, int* type);

/* Sdf::set_zmin / Sdf::set_zmax -- Sdf.h:123-129 (defaults 0.5 / 3.5).  Both bounds finite and zmin < zmax, else
 * GSDF_ERR_INVALID and the range stays as it was.  A change of range withdraws a next-frame hint (gsdf_hint_next_depth_dev):
 * normals computed ahead carry tile statistics taken under the old range. */
int gsdf_set_zrange(gsdf_ctx* c, float zmin, float zmax);

/* new cv::NormalEstimator<float>(W, H, K, Size(win,win)) -> cache() -- normals/NormalEstimator.h:81-165,
 * main_scan_3d.cpp:183.  Also fixes the frame size all later calls must use.
 * win: the side of the box window, odd, 1 .. 15 (the reference's scanner passes 11); a frame may be smaller than the window
 * (BORDER_REFLECT_101 folds it over as often as needed).  win = 1 is accepted and is what the reference computes: the moment
 * matrix of one pixel is singular and most normals are not finite.  An even, non-positive or larger win (or W, H <= 0, K null)
 * is GSDF_ERR_INVALID; the arguments are checked before anything is released, so the context keeps the frame set-up it had. */
int gsdf_normals_init(gsdf_ctx* c, int W, int H, const float K[9], int win);
/* the 11 cached planes (x0,y0,x0/n2,y0/n2,1/n2,Q11,Q12,Q13,Q22,Q23,Q33) copied to the host */
int gsdf_normals_cache(gsdf_ctx* c, float* planes11_host);
/* NormalEstimator::compute(depth, nx, ny, nz) -- NormalEstimator.h:179-204 (host in, host out) */
int gsdf_normals_compute(gsdf_ctx* c, const float* depth_host, float* nx, float* ny, float* nz);

/* Sdf::update(color, depth, K, pose, NEst) -- Sdf.h:117, MapGradPixelSdf.cpp:43-122.
 * color is ignored by the reference and is not part of this ABI.  Synchronous; returns
 * GSDF_ERR_TABLE_FULL / GSDF_ERR_KEY_RANGE if the launch reported one.
 * GSDF_ERR_KEY_RANGE: voxel indices are packed into 21 biased bits per axis, -2^20 <= index < 2^20 (+-20971.52 m at 2 cm voxels).
 * A frame with samples beyond that is fused as if those samples' voxels did not exist: every packable voxel receives exactly
 * what it would have received, the others are dropped, the frame is counted (gsdf_stats::frames, its vis_ bit), and n_valid /
 * n_upd count every valid pixel and every sample with a positive weight, the dropped ones included.  The status is sticky: it
 * is returned by this call, by gsdf_sync and by gsdf_track / gsdf_track_sampled until gsdf_reset, which clears it with the
 * map; exports, queries and gsdf_get_stats keep working meanwhile.  gsdf_merge_raw[_dev] treat rows beyond the range the same
 * way (refused, the other rows of the call merged); the readers (gsdf_query, gsdf_get_voxels, the raycaster, the mesh, the
 * tracker) take a voxel beyond the range as missing, without an error.
 * Depth values: a pixel is fused iff zmin < z < zmax holds as the reference writes it (`z <= zmin || z >= zmax` skips it), so
 * 0, negative, +-inf and denormal depths are skipped -- but all of them enter the normals of the pixels around them as the
 * reference's `z != 0 ? 1 / z : 0` gives them (a denormal: inf, i.e. no finite normal in its window).  A valid pixel whose
 * normal is not finite passes the reference's gates (`<` comparisons) and is fused: distance and weight as usual, the gradient
 * sum of its voxels NaN -- here as there (also most of a frame at win = 1).  A NaN depth passes the range gate in the reference
 * and reaches a float -> int conversion of NaN (undefined behaviour): depth images must not hold NaN. */
int gsdf_update(gsdf_ctx* c, const float* depth_host, const float R[9], const float t[3]);
/* same with depth already resident in HBM; enqueue only.
 * Runs of this call are pipelined: the fusion of a frame is launched when the NEXT frame arrives (that launch's last workgroups
 * compute the next frame's normals in its otherwise idle tail) or when any other entry point of this header that touches the
 * map, the stream or the frame is called on the context -- every one of them launches a waiting fusion first, so results never
 * depend on it.  The staging entries (gsdf_dev_upload, gsdf_dev_upload_async) do so when their destination overlaps the waiting
 * fusion's depth image, so one staging buffer may be reused frame after frame (upload -> update_dev -> upload -> ...) exactly as
 * before; gsdf_dev_alloc / gsdf_host_alloc / gsdf_host_free / gsdf_mark_wait / gsdf_mark_reached / gsdf_upload_wait do not
 * touch it.  The caller's contract is the old one: depth_dev must stay valid and unchanged until the fusion has RUN, i.e. until
 * a mark recorded after this call (gsdf_mark) has been reached, or gsdf_sync has returned.
 * Error reporting lags with the launch: a launch error of frame i's fusion is returned by the call that launches it -- the
 * gsdf_update_dev of frame i + 1 (which is then NOT queued: call it again after handling the error) or whichever entry point
 * flushed it; device-side failures (GSDF_ERR_TABLE_FULL, GSDF_ERR_KEY_RANGE) are sticky and reported by gsdf_sync as before. */
int gsdf_update_dev(gsdf_ctx* c, const float* depth_dev, const float R[9], const float t[3]);

/* RigidOptimizer::optimize(depth, K) -- RigidOptimizer.h:106, RigidPointOptimizer.cpp:40-99.
 * pose7 in/out replaces RigidOptimizer::pose()/set_pose (RigidOptimizer.h:99-103);
 * num_iterations/conv_threshold/damping replace the setters (RigidOptimizer.h:85-97).
 * *converged receives the bool the reference returns; *passes the reduction passes executed. */
int gsdf_track(gsdf_ctx* c, const float* depth_host, const float K[9], float pose7[7],
               int num_iterations, float conv_threshold, float damping,
               int* converged, int* passes);

/* RigidPointOptimizer::optimize_sampled(depth, K, sampling) -- RigidPointOptimizer.h:65, the public member optimize() forwards to
 * with sampling 1 (.h:69-72).  sampling >= 1 is the pixel stride of RigidPointOptimizer.cpp:62 (`y += sampling`, `x += sampling`:
 * the pixels (i * sampling, j * sampling)); a stride beyond the image leaves pixel (0, 0), as there; sampling < 1 (the
 * reference's size_t 0 never leaves its loop) is GSDF_ERR_INVALID.  gsdf_track == gsdf_track_sampled(..., 1, ...).  The frame
 * loop entry below has no such argument because the reference's loop calls optimize() (main_scan_3d.cpp:258). */
int gsdf_track_sampled(gsdf_ctx* c, const float* depth_host, const float K[9], float pose7[7],
                       int num_iterations, float conv_threshold, float damping, int sampling,
                       int* converged, int* passes);

/* The Scan3D loop body without host round trips -- main_scan_3d.cpp:255-266:
 *   conv = pOpt->optimize(depth, K);  if (conv) tSDF->update(color, depth, K, pOpt->pose(), NEst);
 * The pose persists on the device between frames (RigidOptimizer::pose_, RigidOptimizer.h:64);
 * set it with gsdf_set_pose.  Enqueue only; per-frame results are appended to a device log that
 * gsdf_read_frame_log returns (pose7 + converged + passes per frame). */
int gsdf_set_pose(gsdf_ctx* c, const float pose7[7]);
int gsdf_get_pose(gsdf_ctx* c, float pose7[7]);          /* synchronises */
int gsdf_track_and_fuse_dev(gsdf_ctx* c, const float* depth_dev, const float K[9],
                            int num_iterations, float conv_threshold, float damping);
/* Optional, time only: names the frame the NEXT gsdf_track_and_fuse_dev will be called with, before the call for the CURRENT
 * frame.  The current frame's fusion launch then computes NormalEstimator::compute of that next frame in its tail (its last
 * workgroups: the fusion leaves a third of the chip's workgroup slots idle there) -- when that fusion runs, i.e. the current
 * frame converged; it leaves a token, and the next frame's tracker launches, which carry the normals tiles as ever, skip them
 * when they find it.  The same launch also performs the closing head of the current frame's optimize() (reduce, solve, stop
 * test of the first batch's last pass) instead of a tracker launch of its own.
 * The normals and the fusion's tile statistics depend on the depth image and the depth range alone (MapGradPixelSdf.cpp:60,
 * gsdf_set_zrange), so results do not: same poses, same map (tests/test_gpu_parity.py::
 * test_next_depth_hint_is_invisible_except_in_time).  Contract: next_depth_dev already holds the next frame when the CURRENT
 * frame's gsdf_track_and_fuse_dev is called, and stays unchanged until the next frame's call; a copy into it through
 * gsdf_dev_upload* in between withdraws the hint, as do a gsdf_dev_free of its allocation, a gsdf_set_zrange that changes the
 * range, and any other frame entry; a hint that does not match the
 * next call's depth_dev is ignored.  One hint per frame; NULL withdraws it.  No device work, never an error for a mismatch. */
int gsdf_hint_next_depth_dev(gsdf_ctx* c, const float* next_depth_dev);
/* both in one call: gsdf_hint_next_depth_dev(c, next_depth_dev) + gsdf_track_and_fuse_dev(c, depth_dev, ...) -- for hosts whose
 * calls are not free (a ctypes call is ~1.5 us, 1 % of a frame, and the host is in the loop while a frame needs further batches
 * of passes).  next_depth_dev may be NULL. */
int gsdf_track_and_fuse_ahead_dev(gsdf_ctx* c, const float* depth_dev, const float* next_depth_dev, const float K[9],
                                  int num_iterations, float conv_threshold, float damping);
/* log rows = float[10]: pose7, converged, passes, n_hit (of the last pass) */
int gsdf_read_frame_log(gsdf_ctx* c, float* rows10, int64_t max_rows, int64_t* n_rows);

/* wait for all enqueued work; returns the sticky launch status (table full / key range) */
int gsdf_sync(gsdf_ctx* c);
int gsdf_get_stats(gsdf_ctx* c, gsdf_stats* out);        /* synchronises */

/* tsdf_.size() -- number of occupied voxels */
int gsdf_count(gsdf_ctx* c, int64_t* n);
/* get_tsdf() -- MapGradPixelSdf.h:133-138: all (key, SdfVoxel) pairs.  sorted!=0 orders rows by
 * (z,y,x) so exports are diffable.  raw_sums!=0 returns the additive accumulators
 * (sum w*d, sum w*Rn, sum w) instead of (dist, grad, weight) -- the merge wire format. */
int gsdf_export(gsdf_ctx* c, int32_t* keys, float* payload, int64_t max_n, int64_t* n,
                int sorted, int raw_sums);
/* vis_ -- MapGradPixelSdf.h:70, MapGradPixelSdf.cpp:113-115: per voxel, bit f set <=> the voxel was updated by
 * integrated frame f (f = Sdf::counter_ at the time).  The reference always maintains it (PhotoBA reads it
 * through get_vis(), MapGradPixelSdf.h:140-142); here it is opt-in because it costs one more atomic per
 * touched voxel: call gsdf_enable_vis once (before fusing) with the number of frames to keep.
 * gsdf_export_vis returns ceil(max_frames/32) uint32 words per voxel, rows in the (z,y,x) order of
 * gsdf_export(sorted=1); keys may be NULL. */
int gsdf_enable_vis(gsdf_ctx* c, int max_frames);
int gsdf_export_vis(gsdf_ctx* c, int32_t* keys, uint32_t* words, int words_per_voxel, int64_t max_n, int64_t* n);

/* PhotoBA -- class PhotometricOptimizer (ps_optimizer/PhotometricOptimizer.h:68-186, .cpp), coarse photometric
 * bundle adjustment of keyframe poses and voxel distances on the fused map.  Needs gsdf_enable_vis.
 * images: float32 BGR in [0,1], n x H x W x 3 (setImages, cv::Mat CV_32FC3); poses16: n row-major 4x4
 * camera->world (setPoses); frame_idx: integrated-frame index of each keyframe (setKeyframes).
 * LIMIT: 1 <= n <= 64 keyframes per set (GSDF_ERR_INVALID beyond).  The reference's frame_idx_ / poses_ / images_ are
 * unbounded std::vectors (PhotometricOptimizer.h:68-186); here the pose sweep keeps one visibility bit per keyframe in a 64-bit
 * word per voxel and its per-wave LDS accumulators are sized by n.  BASELINE configs[4] (50 keyframes) fits; a larger keyframe
 * set has to be optimised in windows of <= 64 keyframes (the energy is a sum over voxels of terms that couple only the keyframes
 * that see the voxel, so windows of neighbouring keyframes are the usual bundle-adjustment practice -- but it is NOT what the
 * reference computes for n > 64, and no such windowing is done inside the library).
 * Also GSDF_ERR_INVALID, checked before anything is allocated or launched (an earlier setup stays as it is): a negative
 * frame_idx[i] (an id is a bit position of vis_), and a context whose frames have W < 2 or H < 2 (computeImageGradient, :80-140,
 * reads a neighbouring column / row; the reference reads outside such an image).  An id at or beyond the frames of
 * gsdf_enable_vis, or one that was never fused, is legal: that keyframe sees no voxel and its pose stays.
 * gsdf_ba_energy = getEnergy (:273-321), gsdf_ba_solve_pose = solvePose (:499-590), gsdf_ba_solve_dist =
 * solveDist (:326-388), gsdf_ba_optimize = optimize (:611-662): energies receives E0 and E after every pose
 * and distance step (<= 2*max_it+1 values), *converged = relative change < 5e-4. */
int gsdf_ba_setup(gsdf_ctx* c, int n, const float* images_bgr_host, const float* poses16_host, const int* frame_idx,
                  float reg_weight);
/* OptSettings::loss and OptSettings::lambda (PhotometricOptimizer.h:54-57; LossFunction, loss.h:39-46: 0 L2, 1 CAUCHY -- the
 * default --, 2 HUBER, 3 TUKEY, 4 TRUNC_L2).  As in the reference only TRUNC_L2 changes the computation: solveDist (:364) and
 * solvePose (:542) then leave out a keyframe whose intensity residual exceeds lambda^2 in any channel.  Default: CAUCHY, 0.5. */
int gsdf_ba_set_loss(gsdf_ctx* c, int loss, float lambda);
int gsdf_ba_energy(gsdf_ctx* c, float* E);
int gsdf_ba_solve_pose(gsdf_ctx* c, float damping);
int gsdf_ba_solve_dist(gsdf_ctx* c, float damping);
int gsdf_ba_optimize(gsdf_ctx* c, int max_it, float* energies, int* n_energies, int* converged);
int gsdf_ba_get_poses(gsdf_ctx* c, float* poses16_host);
/* The coupled pose step -- solvePoseFull (PhotometricOptimizer.cpp:392-496, public at PhotometricOptimizer.h:180; optimize()
 * names it as the alternative of solvePose at :627-628).  One 6n x 6n system over all keyframes instead of n systems of 6 x 6.
 * For every voxel with |dist| <= voxel size (:406) the observations are collected exactly as in solvePose: the same visibility
 * test, getIntensity, computeJc, the TRUNC_L2 rule (:435), A_ij, the 3 x 6 J_ij, N_j, inv_Nj = (float)(1. / (float)N_j), mean_j,
 * r_ij = A_ij - mean_j.  Then
 *     b[6i .. 6i+5]  += sum_c r_ij[c] * J_ij[c, :]                          (:461-462)
 *     H[i, i]        += (1 - inv_Nj) * J_ij^T J_ij                          (:464-466)
 *     H[i1, i2]      += (-inv_Nj) * J_i1j^T J_i2j,  i1 < i2 both counted by voxel j, and its transpose into H[i2, i1]   (:475-479)
 * so the diagonal blocks and b are the decoupled step's sums (bit for bit what gsdf_ba_solve_pose solves) and only the
 * off-diagonal blocks are new.  delta = H.ldlt().solve(b) (:483) is Eigen's LDLT: symmetric pivoting on the largest remaining
 * |diagonal|, a zero pivot gives a zero component.  If any component of delta is NaN no pose moves (:488-490); otherwise
 * t_i -= delta[6i .. 6i+2], R_i = R_i * SO3::exp(-delta[6i+3 .. 6i+5]) for every keyframe (:491-494).  damping is unused, as in
 * the reference.  n is 1..64 as everywhere in gsdf_ba_*.
 * gsdf_ba_pose_system assembles the system at the current state and changes nothing (poses, map, ColorUpsampler snapshot): H is
 * (6n)^2 floats row-major, full and exactly symmetric, b is 6n floats; either may be NULL, both NULL is GSDF_ERR_INVALID.
 * gsdf_ba_solve_pose_full assembles, solves and updates the poses; synchronous like gsdf_ba_solve_pose.
 * gsdf_ba_set_pose_step chooses the pose step gsdf_ba_optimize runs at :627: 0 = solvePose (the default), 1 = solvePoseFull.
 * It needs a gsdf_ba_setup (GSDF_ERR_INVALID otherwise, or for another value) and lasts until the next gsdf_ba_setup, which
 * sets it back to 0. */
int gsdf_ba_pose_system(gsdf_ctx* c, float* H, float* b);
int gsdf_ba_solve_pose_full(gsdf_ctx* c, float damping);
int gsdf_ba_set_pose_step(gsdf_ctx* c, int mode);
/* what the last gsdf_ba_energy / gsdf_ba_solve_dist call (or the last energy sweep of gsdf_ba_optimize) counted: voxels that took
 * part (energy: |dist| <= voxel size, :285, seen by at least one keyframe; distance sweep: every voxel with an observation) and
 * observations (voxel x keyframe pairs that project into the image, :238-260) -- the units of the sweeps' algorithmic bytes
 * (measurement only; the reference has no counterpart) */
int gsdf_ba_counters(gsdf_ctx* c, int64_t* voxels, int64_t* observations);

/* ColorUpsampler (ps_optimizer/ColorUpsampler.h/.cpp with SdfVoxelHr, sdf_voxel/SdfVoxel.h:61-112): sub-voxel albedo of the
 * voxels near the surface, averaged over the keyframes that see them, and the coloured point cloud.  main_photo_ba.cpp:300-311
 * runs it after PhotoBA.
 *
 * gsdf_color_compute builds the result from the table as it is now, a SNAPSHOT like the reference's SdfHrMap copy: later
 * fusion, BA steps or table growth leave it as it is until the next compute; gsdf_reset drops it.  The table is only read.
 *  - selection (init :143-146): a voxel is kept iff it exists and fabsf(dist) < (float)(sqrt(3.0) * vs), strict, in float; dist is
 *    s / w as the BA sweeps read it, so distances refined by gsdf_ba_solve_dist / gsdf_ba_optimize are used.
 *  - Hr voxel (SdfVoxel.h:83-101): grad = normalized(g); d[i] = dist + vs4 * (+-g0 +- g1 +- g2) in the order of :92-99,
 *    vs4 = 0.25f * vs; sub-voxel i takes x from bit 0, y from bit 1, z from bit 2; its centre is vs * (0.25f * corner_i + idx)
 *    (getSubvoxelFloat :208-212).
 *  - per keyframe (computeColor :334-377, getIntensity :168-204): it counts only if the voxel's vis_ bit frame_idx[i] is set
 *    (PhotoBA's rule: ids past the vectors are unset).  Point = R^T ((centre_i - grad d[i]) - t); m = (fx x) / z + cx,
 *    n = (fy y) / z + cy (a true division).  The keyframe is skipped for all 8 sub-voxels if any m or n is NaN or any sub-voxel
 *    falls outside [0,W) x [0,H); otherwise interpolateImage(n, m) -- PhotoBA's sampling -- is added to per-channel float
 *    sums, and the voxel's one observation count grows by one.  The reference's vis_ resize to frame_idx.back() + 1 (:159) makes
 *    a frame_idx that is not ascending undefined behaviour there; here any order of ids >= 0 is accepted.
 *  - albedo (:369-373, setAlbedo :217-235): c = (1.f / (float)count) * sum clamped to [0, 1]; count 0 gives NaN, which stays NaN
 *    through the clamp.
 * images_bgr_host: n x H x W x 3 floats (BGR, [0,1]) or NULL = the images of gsdf_ba_setup (no second upload).
 * poses16_host: n row-major 4x4 camera-to-world poses, or NULL = PhotoBA's CURRENT poses (gsdf_ba_get_poses).  The reference
 *   colours with the pre-BA key poses (setPoses copies them, PhotometricOptimizer.h:148-151, main_photo_ba.cpp:295,300) while
 *   the distances are the refined ones: pass those poses to reproduce it.
 * frame_idx: n keyframe ids (vis_ bits), or NULL = those of gsdf_ba_setup.
 * Any NULL needs an earlier gsdf_ba_setup with the same n.  GSDF_ERR_INVALID: a base-sdf context, no gsdf_enable_vis, n outside
 * 1..64, a NULL without gsdf_ba_setup, a negative keyframe id.  *n_voxels (nullable) = Hr voxels (getVoxelNumber). */
int gsdf_color_compute(gsdf_ctx* c, int n, const float* images_bgr_host, const float* poses16_host, const int* frame_idx,
                       int64_t* n_voxels);
/* the snapshot in (z, y, x) key order (gsdf_export(sorted = 1)): keys n x 3, rows n x 37 = dist, weight, grad[3] (normalised),
 * d[8], r[8], g[8], b[8].  *n = Hr voxels; NULL keys and rows only report it.  GSDF_ERR_INVALID before a compute. */
int gsdf_color_export(gsdf_ctx* c, int32_t* keys, float* rows, int64_t max_n, int64_t* n);
/* extractCloud (:251-330): one row of 9 floats -- point centre_i + dvec, normal, colour in [0,1] -- per sub-voxel of a voxel
 * seen by a keyframe with weight >= 5, where n = -normalized(grad) (normalised again, as the reference does), dvec = n * d[i],
 * all three |dvec| < vs4 and no colour channel NaN.  Rows follow the snapshot's voxel order, then the sub-voxel index (the
 * reference's order is its hash map's).  *n = rows; NULL rows9 only reports it.  GSDF_ERR_INVALID before a compute. */
int gsdf_color_cloud(gsdf_ctx* c, float* rows9, int64_t max_n, int64_t* n);
/* Hr voxels and observations (voxel x keyframe pairs that counted) of the snapshot (measurement only) */
int gsdf_color_counters(gsdf_ctx* c, int64_t* voxels, int64_t* observations);
/* ColorUpsampler::extractMesh -- HrLayeredMarchingCubes::computeIsoSurface (mesh/HrLayeredMarchingCubes.cpp:359-822)
 * over the snapshot of the last gsdf_color_compute.
 * Marching cubes over the FINE grid of the snapshot: 2 x 2 x 2 cells per Hr voxel, cell 2 (X - min) + bit per axis holding d[i]
 * and the colour of sub-voxel i as bytes ((unsigned char)(c * 255); a NaN colour -- no keyframe counted -- is 0).  min / max are
 * the bounding box of ALL snapshot keys; the sweep visits the cubes anchored at x < dim - 2 per axis (dim = 2 extent, :410-417),
 * so no cube is anchored inside a voxel of the box's maximal coarse layer.  A cube is skipped when one of its 8 cells lies in
 * a voxel the snapshot does not hold or has weight 0.  Cube index (tsdf > iso), corner / edge numbering, interpolate and the
 * triangle table are those of gsdf_extract_mesh (the Hr triTable equals include/gsdf_mc_tables.h entry for entry).  Vertices
 * are 0.5f * ((float)i * vs) - origin with origin = -(float)min * vs (voxelToWorld :817-821): sub-voxel 0 sits on the voxel
 * centre and sub-voxel 1 half a voxel further, NOT at -+ 1/4 voxel as in gsdf_color_cloud -- the reference's mesh, kept.  Vertex
 * colours are getColor's (:756-773): bytes / 255 in float, interpolate with the endpoints in the order of the getColor calls
 * (for edges 2, 3, 6 and 7 the reverse of the vertex's), * 255 truncated to a byte.
 * ONE deliberate deviation: the reference reads green at idx + 1 and blue at idx + 2 (:764-766, its own TODO "seems wrong"),
 * bytes of neighbouring cells of its 4-layer window that are stale or past the buffer -- not a function of the map; here red,
 * green and blue are read at the cell's own index.
 * Conventions of gsdf_extract_mesh: max_tris = 0 sizes the buffer; a buffer too small gives GSDF_ERR_INVALID with the need in
 * *n_tris; no vertex de-duplication; degenerate triangles are dropped (:789); output in the reference's sweep order (fine z,
 * then y, then x, then the triangle number within the cube).  colors_out is nullable.  Only the snapshot is read; table,
 * snapshot and cloud stay as they are.  GSDF_ERR_INVALID before a compute, and for a bounding box of more than 2^19 voxels on
 * an axis (the 64-bit sweep key holds 20 bits per fine coordinate). */
int gsdf_color_mesh(gsdf_ctx* c, float iso, float* triangles_out /* 9 per triangle */,
                    uint8_t* colors_out /* 9 per triangle: r,g,b per vertex; nullable */,
                    int64_t max_tris, int64_t* n_tris);

/* additive merge of raw sums into this table (frame-sharded fusion) */
int gsdf_merge_raw(gsdf_ctx* c, const int32_t* keys, const float* payload_raw, int64_t n);

/* dst += src for two contexts on the SAME device ("G logical shards on 1 GPU"; the GT-pose branch,
 * main_scan_3d.cpp:250-254): a GPU can fuse two frame shards at once, each context on its own stream -- a fusion launch leaves
 * a third of the chip's workgroup slots idle in its tail, which the other context's launch fills -- and adds them up locally
 * before the exchange between devices.  Voxel sums are added, Sdf::counter_ becomes the frames of both, vis_ bit-vectors of the
 * source (if enabled, alike on both) are OR-ed in shifted by dst's frame count (dst's frames come first).  Synchronous; src is
 * left unchanged.  Room: the union holds at most blocks(dst) + blocks(src); if that passes 45 % of dst's block entries dst is
 * doubled first when gsdf_set_auto_grow allows it, and if it would pass 90 % of them (no growth allowed, or not enough) the call
 * returns GSDF_ERR_TABLE_FULL with dst UNCHANGED.  Should the kernel itself still report a full table, dst holds part of src,
 * Sdf::counter_ is not advanced and dst is to be reset (gsdf_reset). */
int gsdf_merge_from(gsdf_ctx* dst, gsdf_ctx* src);

/* dst += src RESAMPLED on dst's voxel grid under a rigid pose: the step behind gsdf_surface_cloud + gsdf_align_points, for two
 * maps that were NOT fused in one frame (a second session, a map of another run, a tracked shard).  The reference has one map
 * and one session and no such function; like the raycaster this is defined on top of Sdf::weights / Sdf::tsdf
 * (MapGradPixelSdf.h:109-125).
 * pose7 = tx ty tz qx qy qz qw, src frame -> dst frame, exactly what gsdf_align_points leaves in its pose7.
 * R = Eigen's toRotationMatrix of (qx qy qz qw) as it comes, NOT renormalised (the bits of the tracker's R); t = pose7[0..3);
 * vs the common voxel size, T the common truncation distance.  For every voxel index K = (i, j, k) of dst's grid inside the
 * packable key range, in float, without FMA, in this order:
 *   1. c = (vs * (float)i, vs * (float)j, vs * (float)k)                       vox2float
 *   2. d = c - t, per component
 *   3. q = R^T d, each component x0 + (x1 + x2): q.x = R00 d.x + (R10 d.y + R20 d.z), ...
 *   4. a component of q that is not finite: K gets nothing (tested before any float -> int conversion)
 *   5. (w, phi) = what gsdf_query returns at q: weights() and tsdf() of the voxel V = float2vox(q) of src, phi = dist_V +
 *      1.2 g^_V . (c_V - q) rounded once from double; w == 0 (V missing, beyond the key range, weight 0): K gets nothing
 *   6. otherwise, with (S_w, S_s, S_gx, S_gy, S_gz) the stored sums of V, K receives
 *        w' = S_w,   s' = S_w * truncate(phi, T) (one float product),   g' = R (S_gx, S_gy, S_gz), rows as x0 + (x1 + x2)
 *   7. dst's sums at K become (w + w', s + s', g + g'), one float addition per field; a missing voxel or block counts as
 *      zeros and is created.
 * phi is tsdf() with its factor 1.2 and not a plain Taylor step because that IS the map's value off a voxel centre: tracker,
 * raycaster, registration and extract_pc share it, so a surface point of the merged map lies where src's own extract_pc puts
 * it, moved by the pose.  The raw gradient sum is rotated, not w g^: it keeps the magnitude gsdf_merge_from keeps and is linear.
 * The clamp keeps |dist| <= T in dst.  With the identity pose the result differs from gsdf_merge_from's only in s, by the
 * round trip S_w * (S_s / S_w).
 * The result is a function of (dst, src, pose) alone: a key gets at most one contribution, there are no floating-point
 * atomics and no order left to the scheduler; the same call on the same state gives the same bytes, also across gsdf_grow
 * of either context.
 * Sdf::counter_ of dst becomes the frames of both.  *n_voxels (nullable) = keys that received a contribution, *n_blocks
 * (nullable) = dst blocks they lie in; both are 0 on every refusal.  Synchronous; a waiting pipelined fusion of either context is launched
 * first; src is only read.
 * GSDF_ERR_INVALID, nothing touched: a NULL context or pose, dst == src, different devices, different voxel size or
 * truncation, either context of type GSDF_MAP_BASE (no stored gradient), either context with gsdf_enable_vis on (carrying the
 * vis_ bit-vectors across a resampling is not built, and with it PhotoBA on a posed-merged map), a pose entry that is not
 * finite, | qx^2 + qy^2 + qz^2 + qw^2 - 1 | > 1e-4.
 * GSDF_ERR_TABLE_FULL, nothing touched: src's status holds a full table (as gsdf_merge_from).
 * Room: the number B of dst blocks that receive something is known exactly before dst is written.  If blocks(dst) + B passes
 * 45 % of dst's block entries dst is doubled first when gsdf_set_auto_grow allows it; if it would pass 90 % of them the call
 * returns GSDF_ERR_TABLE_FULL with dst UNCHANGED.  A failed allocation (GSDF_ERR_HIP) leaves dst unchanged as well.  Scratch:
 * 1280 B per candidate block of dst (about twice the blocks that receive).
 * GSDF_ERR_KEY_RANGE: a key beyond the packable +-2^20 range would have received a contribution (evaluated up to +-2^22
 * voxels; an image farther out counts as such).  Those keys are left out, the rest IS merged and counted, Sdf::counter_
 * advances -- as gsdf_update reports samples it dropped. */
int gsdf_merge_from_posed(gsdf_ctx* dst, gsdf_ctx* src, const float pose7[7],
                          int64_t* n_voxels /* nullable */, int64_t* n_blocks /* nullable */);
/* What the last gsdf_merge_from_posed into dst did, for tools: counts[2] = candidate blocks before / after de-duplication;
 * ms[4] = event times of the candidate list's filling pass, sort + unique, the sampling kernel, the adding kernel.  Either may
 * be NULL; zeros before the first call and for stages that did not run. */
int gsdf_merge_posed_last(gsdf_ctx* dst, int64_t counts[2], float ms[4]);
/* n (1..4) contexts for n frame shards on ONE device, like gsdf_create each -- but their streams are guaranteed to sit in n
 * different hardware queues (created at the device's highest stream priority: the runtime pools its queues per priority, and
 * nothing else uses that pool), so that their launches overlap.  Streams of the default priority share queues as soon as the
 * process holds more streams than the runtime has queues (4), and then two contexts fuse no faster than one.
 * Side effects, stated: the shard streams run at the HIGHEST priority, so their launches are scheduled ahead of default-priority
 * work on the same GPU (other gsdf contexts, PyTorch) -- meant for a process whose GPU work at that moment IS the shard fusion;
 * and the guarantee holds only while nothing else in the process creates highest-priority streams.  A device without a stream
 * priority range makes the call fail (GSDF_ERR_HIP) instead of handing out default-priority streams. */
int gsdf_create_shards(gsdf_ctx** out, int n, float voxel_size, float trunc_dist, int capacity_log2, int device);

/* device-buffer variants for the multi-GPU exchange (RCCL works on device memory): unsorted
 * compaction of (key, raw sums) into caller-provided DEVICE buffers / additive merge from them.
 * These are the pack / unpack steps either side of the all-gather. */
int gsdf_export_raw_dev(gsdf_ctx* c, int32_t* keys_dev, float* payload_raw_dev, int64_t max_n, int64_t* n);
int gsdf_merge_raw_dev(gsdf_ctx* c, const int32_t* keys_dev, const float* payload_raw_dev, int64_t n);

/* Dense variant of the exchange: the all-reduce of per-voxel (weight, weighted distance, weighted gradient) named in
 * BASELINE.json's north_star.  The map is a hash of 4x4x4 voxel blocks; block ids are opaque 64-bit words, identical
 * across contexts.  (1) gsdf_block_keys_dev lists this map's block ids (*n = count, also when > max_n); the ranks
 * all-gather and unique them; (2) gsdf_pack_blocks_dev writes 64 x 5 raw sums (w, s, gx, gy, gz; zeros for voxels or
 * blocks this map lacks) per listed block into a DEVICE buffer, which RCCL all-reduces (sum); (3)
 * gsdf_unpack_blocks_dev stores the reduced sums (inserting missing blocks).  All pointers are device pointers. */
int gsdf_block_keys_dev(gsdf_ctx* c, uint64_t* block_keys_dev, int64_t max_n, int64_t* n);
int gsdf_pack_blocks_dev(gsdf_ctx* c, const uint64_t* block_keys_dev, int64_t n, float* dense_dev);
int gsdf_unpack_blocks_dev(gsdf_ctx* c, const uint64_t* block_keys_dev, int64_t n, const float* dense_dev);

/* The exchange step as ONE call, for C++ hosts (BASELINE.json north_star: "frames shard naturally across the
 * 8 GPUs of one node with a RCCL-over-xGMI all-reduce of per-voxel (weight, weighted-distance, weighted-gradient) before
 * mesh extraction").  Collective: every rank of the communicator calls it with the map it fused from its own frames (the
 * GT-pose branch, main_scan_3d.cpp:250-254); on return every rank's map is the sum of all maps (and every rank's table has the
 * capacity of the largest one: ranks whose tables are smaller grow first, gsdf_grow).  Steps: all-gather of the block-key arrays, sorted union on the device, gsdf pack, ONE ncclAllReduce (sum, float32, 1280 B per block of the union) on the context's own
 * stream, gsdf unpack.  nccl_comm: an ncclComm_t of the RCCL already in the process (RCCL is resolved at run time, it is
 * not a link dependency of libgsdf.so).  n_blocks / bytes (nullable): size of the union / of the all-reduced buffers.
 * Also exchanged: Sdf::counter_ (Sdf.h:65) -- afterwards the frames integrated by ALL ranks -- and, when gsdf_enable_vis was
 * called (on every rank, with the frame count of the WHOLE job), the vis_ bit-vectors (MapGradPixelSdf.cpp:113-115): the
 * frame shards are contiguous in rank order, so frame f of rank r becomes integrated frame (frames of the ranks < r) + f and
 * the ranks' shifted vectors are OR-ed (a second all-reduce, unsigned words): the merged map is what PhotoBA needs (C4 -> C5).
 * ONE-SHOT: after the call every map IS the sum, so a second exchange over more than one rank is refused (GSDF_ERR_INVALID)
 * until gsdf_reset.  Failures are collective: a rank that cannot prepare its part reports that through the first all-gather
 * and every rank returns the error, none is left waiting inside a collective -- with ONE exception: the two header buffers
 * of a few hundred bytes are needed to talk at all, and a rank whose hipMalloc fails for THEM returns before the first
 * all-gather; its peers then wait in it (treat that as fatal for the job, as an out-of-memory device is).
 * Memory: the key arrays are gathered WHOLE (8 B per block entry of the table, occupied or not, from every rank) and sorted on
 * the device: three buffers of nranks x 2^(capacity_log2 - 6) x 8 B plus the sort's scratch -- 3 x 4 MB at 8 ranks and 2^22
 * records, 3 x 268 MB at 2^28 (auto-grow's CLI limit), 3 x 1 GB at 2^30.  Growing to the largest rank's capacity also happens
 * inside this call (and inside a timed exchange). */
int gsdf_merge_allreduce(gsdf_ctx* c, void* nccl_comm, int64_t* n_blocks, int64_t* bytes);
/* Optional set-up of the exchange outside a timed region (like the communicator): the scratch buffers for `nranks` ranks and one
 * run of the union's sort kernels, whose code is loaded on first use (~10 ms in the first exchange of a process otherwise).
 * Not collective. */
int gsdf_merge_prepare(gsdf_ctx* c, int nranks);
/* communicator plumbing for hosts that do not link RCCL themselves (the Scan3D CLI): ncclGetUniqueId / ncclCommInitRank
 * (on `device`) / ncclCommDestroy.  Create the communicator once, outside any timed region. */
int gsdf_rccl_unique_id(char id128[128]);
int gsdf_rccl_comm_init(void** nccl_comm, int nranks, const char id128[128], int rank, int device);
int gsdf_rccl_comm_count(void* nccl_comm, int* nranks);       /* ncclCommCount: ranks of the communicator */
int gsdf_rccl_comm_destroy(void* nccl_comm);
/* The same exchange over a caller-provided transport: two collectives on HOST buffers (libgsdf stages the device data).
 * Used where RCCL cannot run (two ranks on one GPU in the tests) or where the host has its own communication layer.
 * Both callbacks return 0 on success. */
typedef struct gsdf_collective {
    /* recv[r * bytes .. (r + 1) * bytes) := rank r's `send` (bytes per rank are equal on all ranks) */
    int (*allgather)(void* user, const void* send, void* recv, int64_t bytes);
    /* buf[i] := sum over the ranks of buf[i], i < n */
    int (*allreduce_sum_f32)(void* user, float* buf, int64_t n);
    void* user;
    int nranks;
} gsdf_collective;
int gsdf_merge_allreduce_with(gsdf_ctx* c, const gsdf_collective* ops, int64_t* n_blocks, int64_t* bytes);

/* Sdf::weights(point) and Sdf::tsdf(point, &grad) at n points -- MapGradPixelSdf.h:109-125.
 * w[i]==0 marks a missing voxel (dist/grad are then 0; the reference's .at() would throw). */
int gsdf_query(gsdf_ctx* c, const float* pts_host, int64_t n, float* dist, float* grad, float* w);

/* MapGradPixelSdf::getSdf(idx) = tsdf_.at(idx) -- MapGradPixelSdf.h:127-129, for n voxel indices at once: the STORED voxel,
 * payload = dist, gx, gy, gz (the raw weighted gradient sum, not the normalised one gsdf_query returns), weight.
 * found[i] == 0 marks a missing voxel (payload zeros; the reference's .at() would throw). */
int gsdf_get_voxels(gsdf_ctx* c, const int32_t* keys_host, int64_t n, float* payload, int32_t* found);

/* REGISTRATION OF A POINT SET against the map -- the loop of RigidPointOptimizer::optimize_sampled
 * (RigidPointOptimizer.cpp:51-96) over n points the caller brings instead of the back-projected pixels of :62-69: from :70 on
 * the reference's tracker never looks at the depth image again.  A second session's cloud, a LiDAR sweep, the vertices of a CAD
 * part: anything that is to be brought into the map's frame (e.g. in front of gsdf_merge_from_posed, which takes the pose found here; gsdf_merge_from needs both
 * maps in one frame).
 * pts: n rows x y z (float32) in the source frame; every coordinate must be finite.  pose7 in/out (tx ty tz qx qy qz qw, unit
 * quaternion): source -> map.  The context's persistent pose (gsdf_set_pose / gsdf_get_pose), the frame log and gsdf_stats are
 * neither read nor written.
 * One pass, per point: R = rotationMatrix() (:53); p = R x + t (:70); then exactly what gsdf_query returns for p -- weights() and
 * tsdf() of MapGradPixelSdf.h:109-125 -- and, where w > 0, the terms phi^2, phi J[i], J[i] J[j] with J = (g, p x g) (:76-80) and
 * the count (:81).  A point whose voxel is missing, beyond the key range or of weight 0 contributes nothing; a point that is not
 * finite after the transform is skipped before the float -> int conversion of float2vox (the reference would convert it, which
 * is undefined).  The float terms are widened to double and added in an order that depends on n alone (no floating-point
 * atomics: the same call gives the same bytes, run to run and across gsdf_grow); each of the 29 sums is rounded to float once.
 * Then xi = damping * H.llt().solve(g) (:86) with correctly rounded roots and divisions, |xi|^2 = (x0 + (x1 + x2)) + (x3 + (x4 +
 * x5)); |xi|^2 < conv_threshold^2 ends the run converged without applying xi (:88-91); otherwise, unless a component is NaN,
 * pose = SE3::exp(-xi) * pose (:94-95).
 * *converged receives the bool the reference returns, *passes the reduction passes executed (k + 1 when converged at k, else
 * num_iterations), as gsdf_track counts them.  trace36 (nullable, num_iterations x 36 floats) receives one row per executed
 * pass: E, g[6], H upper triangle[21] row-major, count, xi[6] (damped), |xi|^2.
 * n == 0 (pts may be NULL) behaves like an empty map: H = 0, xi NaN, not converged, *passes = num_iterations, pose7 unchanged.
 * num_iterations == 0: *converged = 0, *passes = 0.  GSDF_ERR_INVALID: n < 0, num_iterations < 0, a NULL pose7 / converged /
 * passes, NULL pts with n > 0, and a base-sdf context (the trilinear gather of MapPixelSdf is not built for point sets).
 * Synchronous; a waiting pipelined fusion is launched first.  The _dev variant reads n x 3 contiguous floats of DEVICE memory in place (any
 * buffer of gsdf_dev_alloc of a context on the same device, this one or another); the buffer must stay unchanged until the
 * call returns.  Multi-GPU: not built -- the points and the map live on one device. */
int gsdf_align_points(gsdf_ctx* c, const float* pts_host, int64_t n, float pose7[7],
                      int num_iterations, float conv_threshold, float damping,
                      int* converged, int* passes, float* trace36 /* nullable */);
int gsdf_align_points_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float pose7[7],
                          int num_iterations, float conv_threshold, float damping,
                          int* converged, int* passes, float* trace36 /* nullable */);

/* gsdf_align_points from m starting poses at once: one Gauss-Newton run per row of poses7 (m x 7, in / out), all over the same n
 * points, every pass of every run that has not ended in ONE launch pair (k_align_pass_multi with gsdf_align_grid(n) x live
 * workgroups, k_align_head_multi with one workgroup per live run).  A single run finds the answer only from inside its basin (about
 * 2 degrees / 15 cm on the 320x240 test pair); a grid of starts (gsdf_align_starts) and the pick among the runs
 * (gsdf_align_best) widen it.
 * For every h the outputs poses7[h], converged[h], passes[h] and the trace rows [0, passes[h]) are equal in BYTES to what
 * gsdf_align_points returns for (pts, n, poses7[h], the same arguments) on the same map: both run the same device functions
 * over the same launch geometry per run, the sums in the same order, no floating-point atomics.  The result of run h does not
 * depend on m, on its position in the batch or on when the other runs end.
 * trace36 (nullable, m x num_iterations x 36): run h's rows at [h][0 .. passes[h]), zeros from there on.  last36 (nullable,
 * m x 36): trace row passes[h] - 1, zeros when passes[h] == 0.
 * n == 0 and num_iterations == 0 behave per run as in the single call.  GSDF_ERR_INVALID with every output untouched: m < 1,
 * m > GSDF_ALIGN_MAX_STARTS, and what the single call refuses (NULL c / poses7 / converged / passes, NULL pts with n > 0, n < 0,
 * num_iterations < 0, a base-sdf context).
 * Synchronous; a waiting pipelined fusion is launched first.  The context's persistent pose, frame log and gsdf_stats are
 * neither read nor written.  Scratch: m x (256 + gsdf_align_grid(n) x 256) bytes of device memory, kept by the context; a failed
 * allocation returns GSDF_ERR_HIP with nothing changed.  The host reads the m run states once per batch of launch pairs (the
 * batches of the single call) and queues the next batch for the runs that have not ended only.  The _dev variant reads the points
 * in place, as gsdf_align_points_dev. */
#define GSDF_ALIGN_MAX_STARTS 1024
int gsdf_align_points_multi(gsdf_ctx* c, const float* pts_host, int64_t n, float* poses7 /* m x 7, in/out */, int m,
                            int num_iterations, float conv_threshold, float damping,
                            int* converged /* m */, int* passes /* m */,
                            float* last36 /* m x 36, nullable */, float* trace36 /* m x num_iterations x 36, nullable */);
int gsdf_align_points_multi_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float* poses7 /* m x 7, in/out */, int m,
                                int num_iterations, float conv_threshold, float damping,
                                int* converged /* m */, int* passes /* m */,
                                float* last36 /* m x 36, nullable */, float* trace36 /* m x num_iterations x 36, nullable */);

/* A grid of starting poses around center7 (tx ty tz qx qy qz qw, source -> map).  Host only: no context, no GPU.
 * Rn = 2 rot_k + 1, Tn = 2 trans_k + 1, *m = Rn^3 Tn^3, always reported (2^31 - 1 if it would pass that).  Start
 * h = ((((a Rn + b) Rn + c) Tn + d) Tn + e) Tn + f has the rotation vector r = rot_step_rad (a - rot_k, b - rot_k, c - rot_k) and
 * the offset o = trans_step (d - trans_k, e - trans_k, f - trans_k) in the MAP frame: the source is rotated by r about `pivot`
 * (source frame; pass the cloud's centroid), then the centre pose is applied, then the offset.  All in double from the float
 * inputs: qc = the centre's quaternion normalised, Rc its matrix; theta = |r|, qd = (sin(theta / 2) r / theta, cos(theta / 2)) or
 * the identity when theta == 0, dR its matrix; q_h = qc (x) qd normalised, its sign such that w >= 0;
 * t_h = Rc (pivot - dR pivot) + tc + o; each of the 7 values rounded to float once.  The middle index (*m - 1) / 2 is the centre
 * pose itself.  poses7_out == NULL or max_m == 0 is the sizing call; a max_m below *m writes nothing and returns
 * GSDF_ERR_INVALID.  GSDF_ERR_INVALID also: a NULL centre / pivot / m, negative rot_k / trans_k / max_m, an input that is not
 * finite, a centre quaternion whose norm is off 1 by more than 1e-4 (*m not written in these cases), *m > GSDF_ALIGN_MAX_STARTS. */
int gsdf_align_starts(const float center7[7], const float pivot[3], float rot_step_rad, int rot_k, float trans_step, int trans_k,
                      float* poses7_out, int max_m, int* m);

/* The pick among the m runs of gsdf_align_points_multi.  Host only.  Run h is eligible if passes[h] > 0, converged[h] (unless
 * !require_converged), count = last36[h][28] >= min_count and > 0, and E = last36[h][0] is finite; its score is (double)E /
 * (double)count, the mean squared distance of the points that hit.  *best = the eligible run of the smallest score, the lowest
 * index on a tie, or -1 (still GSDF_OK) if none is eligible.  E is the energy at the pose BEFORE the step of the last executed
 * pass: for a converged run, whose last step is not applied, that is the returned pose exactly; for one that ran out of passes
 * it is the pose one step earlier.  GSDF_ERR_INVALID: m < 1 or a NULL argument. */
int gsdf_align_best(int m, const int* converged, const int* passes, const float* last36, int64_t min_count,
                    int require_converged, int* best);

/* ROBUST REGISTRATION.  gsdf_align_points minimises the plain sum of squares of RigidPointOptimizer.cpp:76-81: right for a depth
 * frame against the map it was tracked on, wrong for two sessions of a scene in which something moved or that overlap in part --
 * the points that do not belong pull the pose.  The entries below multiply every term of a point by the weight a robust loss
 * gives its distance (iteratively reweighted least squares with a constant scale).  The loss family is the reference's
 * ps_optimizer/loss.h:41-48 and the integers are those of gsdf_ba_set_loss.
 *
 * The weight of one point.  Host only: no context, no GPU; it is the inline function the kernel calls (csrc/gsdf_align_loss.h).
 * All float, no contraction, correctly rounded divisions.  With a = |phi|, k = scale, r = phi / k, rr = r * r:
 *     0 L2        1 (scale ignored)
 *     1 CAUCHY    1 / (1 + rr)
 *     2 HUBER     a <= k ? 1 : k / a
 *     3 TUKEY     a < k ? (1 - rr) * (1 - rr) : 0
 *     4 TRUNC_L2  a < k ? 1 : 0
 * GSDF_ERR_INVALID: loss outside 0..4, a NULL w, and for loss != 0 a scale that is not finite or not > 0. */
int gsdf_align_loss_weight(int loss, float scale, float phi, float* w);

/* gsdf_align_points / _dev / _multi / _multi_dev with a loss.  Per point everything up to the map values (w0, phi, g) is the plain
 * pass; where w0 > 0, with one float operation per step: rw = the weight above of phi, wphi = rw * phi, wJ[a] = rw * J[a]; the
 * terms are wphi * phi, wphi * J[a] and wJ[a] * J[b] (a <= b); the count is raised by 1 as before; two more sums: wsum += rw and
 * n_in += 1 where rw > 0.  The 31 sums are widened, ordered and rounded exactly as the 29 of the plain pass.  Head, stop rule, pose
 * update, batching and scratch are the plain call's (the partial rows had the room).
 * The trace rows are 38 floats wide: [0..35] as in gsdf_align_points with the weighted E, g and H, [36] = wsum, [37] = n_in.
 * trace38: num_iterations x 38 (m x num_iterations x 38 for the multi entries), last38: m x 38; both nullable.
 * With loss = 0 every output is equal in BYTES to the plain entry's for the same call (pose, flags, passes, floats [0..35] of
 * every row), and [36] == [37] == [28].  Run h of a multi call is equal in bytes to the single robust call from poses7[h].
 * GSDF_ERR_INVALID with every output untouched: what the plain entry refuses (a base-sdf context included), a loss outside 0..4
 * and, for loss != 0, a scale that is not finite or not > 0.  The context's persistent pose, frame log and gsdf_stats are
 * neither read nor written.  Not built: a normal-compatibility gate, an annealed or automatic scale, base maps, multi-GPU. */
int gsdf_align_points_robust(gsdf_ctx* c, const float* pts_host, int64_t n, float pose7[7],
                             int num_iterations, float conv_threshold, float damping, int loss, float scale,
                             int* converged, int* passes, float* trace38 /* nullable */);
int gsdf_align_points_robust_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float pose7[7],
                                 int num_iterations, float conv_threshold, float damping, int loss, float scale,
                                 int* converged, int* passes, float* trace38 /* nullable */);
int gsdf_align_points_multi_robust(gsdf_ctx* c, const float* pts_host, int64_t n, float* poses7 /* m x 7, in/out */, int m,
                                   int num_iterations, float conv_threshold, float damping, int loss, float scale,
                                   int* converged /* m */, int* passes /* m */,
                                   float* last38 /* m x 38, nullable */, float* trace38 /* m x num_iterations x 38, nullable */);
int gsdf_align_points_multi_robust_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, float* poses7 /* m x 7, in/out */, int m,
                                       int num_iterations, float conv_threshold, float damping, int loss, float scale,
                                       int* converged /* m */, int* passes /* m */,
                                       float* last38 /* m x 38, nullable */, float* trace38 /* m x num_iterations x 38, nullable */);

/* gsdf_align_best for the runs of gsdf_align_points_multi_robust.  Host only.  Run h is eligible if passes[h] > 0, converged[h]
 * (unless !require_converged), wsum = last38[h][36] >= min_wsum and > 0, and E = last38[h][0] is finite; its score is (double)E /
 * (double)wsum, the weighted mean squared distance.  *best = the eligible run of the smallest score, the lowest index on a tie,
 * or -1 (still GSDF_OK) if none is eligible.  GSDF_ERR_INVALID: m < 1 or a NULL argument. */
int gsdf_align_best_robust(int m, const int* converged, const int* passes, const float* last38, float min_wsum,
                           int require_converged, int* best);

/* What a pass from pose7 (tx ty tz qx qy qz qw, source -> map) sees per point: p = R x + t exactly as the pass forms it, then the
 * map values at p as gsdf_query returns them.  w_out[i] = the voxel's weight, 0 for a missing voxel or a point that is not finite
 * after the transform; phi_out[i] = the distance, 0 where w_out[i] == 0.  With the pose a registration returned, |phi_out| splits
 * the cloud into the part that registered and the part that moved.  phi_out and w_out are HOST buffers of n floats in both
 * variants; the _dev variant reads n x 3 floats of device memory in place.  One lane per point (k_align_residuals).
 * n == 0: nothing is written (the pointers may be NULL).  GSDF_ERR_INVALID: a NULL c / pose7, n < 0, NULL points or outputs with
 * n > 0, a base-sdf context.  Synchronous; a waiting pipelined fusion is launched first; the table is only read, and the
 * persistent pose, the frame log and gsdf_stats are untouched. */
int gsdf_align_residuals(gsdf_ctx* c, const float* pts_host, int64_t n, const float pose7[7], float* phi_out, float* w_out);
int gsdf_align_residuals_dev(gsdf_ctx* c, const float* pts_dev, int64_t n, const float pose7[7], float* phi_out, float* w_out);

/* MapGradPixelSdf::extract_pc (MapGradPixelSdf.cpp:177-195) in memory instead of an ASCII PLY: one row x y z nx ny nz per voxel
 * with weight >= 5 (:184) and |dist * 1.2 g^| < voxel_size / 2 on every axis (:186-188), point = vox2float(idx) - dist * 1.2 g^
 * (:191), normal = -1.2 g^ (:192), all in float; g^ the normalised stored gradient sum.  The reference's row order is its hash
 * map's; here rows follow the (z, y, x) key order of gsdf_export(sorted = 1).
 * *n = rows of the cloud, always reported.  rows6 == NULL or max_n == 0 is the sizing call (nothing written, GSDF_OK); a max_n
 * below the count writes nothing and returns GSDF_ERR_INVALID with the need in *n.  The _dev variant leaves the rows in the
 * caller's DEVICE buffer (max_n x 6 floats), so that another context on the same device can read them without a host copy.
 * Synchronous; the table is only read; a waiting pipelined fusion is launched first.  GSDF_ERR_INVALID on a base-sdf context. */
int gsdf_surface_cloud(gsdf_ctx* c, float* rows6_host, int64_t max_n, int64_t* n);
int gsdf_surface_cloud_dev(gsdf_ctx* c, float* rows6_dev, int64_t max_n, int64_t* n);

/* REMOVING VOXELS: a selection on the device, its consumers, erase and compact.  The reference's map only grows (tsdf_ is never
 * erased from); a multi-session engine needs the opposite as well: take out what moved between sessions before
 * gsdf_merge_from_posed, drop speckle of weight below the extraction threshold, crop to a region, take a region out and put it
 * back later (gsdf_select_export + gsdf_merge_raw).
 *
 * A context owns at most one selection S: a set of voxel SLOTS of the present table, one 64-bit word per block entry, bit =
 * the voxel's index in its 4x4x4 block (8 B per block entry: 512 KB at 2^22 records; allocated by the first select call).
 * Membership is by slot, whether or not the voxel exists; every consumer (count, export, erase) acts on the members with w > 0
 * at the time it runs, and the *n a select call reports (nullable) is that count at its return.
 * States: none, valid, lost.  gsdf_reset, gsdf_select_clear, gsdf_erase_selected and gsdf_compact leave none.  Any rehash leaves
 * a valid selection lost, because slots move: gsdf_grow, auto-grow, and the grows inside gsdf_merge_from, gsdf_merge_from_posed
 * and gsdf_merge_allreduce.  On a lost selection the consumers, gsdf_select_invert and the combining ops (ADD, INTERSECT,
 * SUBTRACT) return GSDF_ERR_INVALID with a message that says so; GSDF_SEL_REPLACE and gsdf_select_clear start over.  On none the
 * consumers report zero and GSDF_OK, and the combining ops start from the empty set.
 * op: S := P (REPLACE), S | P (ADD), S & P (INTERSECT), S & ~P (SUBTRACT), P the call's predicate set.
 *
 * Predicates: float, without FMA, in the order written.
 *   centre  of voxel index (i, j, k): c = (vs * (float)i, vs * (float)j, vs * (float)k)          -- step 1 of gsdf_merge_from_posed
 *   box     member iff lo[a] <= c[a] && c[a] <= hi[a] on all three axes.  lo > hi on an axis: the empty set.  A NaN bound:
 *           GSDF_ERR_INVALID; infinities are allowed.  The kernel reads block keys only, no voxel records.
 *   weight  member iff w_min <= w && w < w_max, w the stored weight sum.  w_max = +inf is allowed; a NaN: GSDF_ERR_INVALID.
 *   points  p = x when pose7 == NULL, else p = R x + t exactly as gsdf_align_points and gsdf_align_residuals form it (R = Eigen's
 *           toRotationMatrix of the quaternion as it comes, rows as x0 + (x1 + x2), then + t).  A point with a component of p
 *           that is not finite is skipped.  A voxel is a member iff for some point, with d = c - p per component,
 *               dx * dx + (dy * dy + dz * dz) <= radius * radius              (one float product on the right)
 *           The set is defined over ALL voxels of the map; the kernel enumerates, per point and axis, the integer range
 *           [ceil((p - radius) / vs) - 1, floor((p + radius) / vs) + 1] taken in double -- one index wider on each side than exact
 *           arithmetic needs --, tests the predicate above on every candidate and leaves out candidates beyond the packable
 *           +-2^20 range before any packing (a point farther than 2^21 voxels from the origin on an axis has none).
 *           GSDF_ERR_INVALID: a negative or non-finite radius, radius > 16 * vs (at most 35^3 candidates per point), a pose that
 *           gsdf_merge_from_posed would refuse (not finite, | |q|^2 - 1 | > 1e-4), n_pts < 0, NULL points with n_pts > 0.
 *           n_pts == 0 is the empty predicate set.  The _dev variant reads n_pts x 3 floats of
 *           DEVICE memory in place.  Bits are set with integer atomic OR: the result is a set, nothing depends on an order.
 * gsdf_select_invert complements S over the slots of existing blocks (on none: everything).
 * gsdf_select_count: members with w > 0, and the blocks that hold at least one (either pointer may be NULL).
 * gsdf_select_export: the members with w > 0 in (z, y, x) key order, payload as gsdf_export (raw_sums selects sums or means).
 * Sizing conventions of gsdf_surface_cloud: *n is always reported; keys and payload NULL or max_n == 0 is the sizing call; a
 * max_n below the count writes nothing and returns GSDF_ERR_INVALID with the need in *n.  gsdf_select_export_raw_dev writes each
 * member exactly once, in no stated order, as raw sums into DEVICE buffers like gsdf_export_raw_dev.  vis_ words are NOT
 * carried by either export: a region taken out and merged back comes back without them.
 *
 * gsdf_erase_selected zeroes all 32 bytes of every member record, and its vis_ words when gsdf_enable_vis is on: exactly what
 * the table clear leaves, so a later fusion into that key starts from nothing.  Block keys STAY: the lookup's "an empty entry
 * ends the chain" rule holds because no entry is ever emptied.  *n_voxels = members that existed, *n_blocks_emptied = blocks
 * that lost at least one voxel and hold none afterwards (both nullable).  It allocates nothing, so it cannot fail half-way.
 * PhotoBA's gate list and mean cache are dropped as gsdf_grow drops them; a ColorUpsampler snapshot is a copy and stays.
 * gsdf_compact rebuilds the table without the blocks that hold no voxel with w > 0 -- the rebuild of gsdf_grow with dead blocks
 * left behind.  new_capacity_log2 0 keeps the capacity; otherwise 10..30, smaller than the present one included, as long as the
 * live blocks stay at or below 45 % of the new block entries (the room rule of gsdf_merge_from): beyond that
 * GSDF_ERR_TABLE_FULL with the map unchanged.  A failed allocation leaves the map unchanged.  *n_blocks_dropped is nullable.
 * The map's exported bytes (gsdf_export, gsdf_export_vis) are unchanged.
 *
 * All entries are synchronous and launch a waiting pipelined fusion first.  Pose, frame log, Sdf::counter_ and gsdf_stats are
 * left as they are.  Both map types.  Not built: carrying vis_ through an export, erasing across ranks. */
#define GSDF_SEL_REPLACE   0
#define GSDF_SEL_ADD       1
#define GSDF_SEL_INTERSECT 2
#define GSDF_SEL_SUBTRACT  3
int gsdf_select_box(gsdf_ctx* c, const float lo[3], const float hi[3], int op, int64_t* n);
int gsdf_select_weight(gsdf_ctx* c, float w_min, float w_max, int op, int64_t* n);
int gsdf_select_points(gsdf_ctx* c, const float* pts_host, int64_t n_pts, const float pose7[7] /* nullable */, float radius,
                       int op, int64_t* n);
int gsdf_select_points_dev(gsdf_ctx* c, const float* pts_dev, int64_t n_pts, const float pose7[7] /* nullable */, float radius,
                           int op, int64_t* n);
int gsdf_select_invert(gsdf_ctx* c, int64_t* n);
int gsdf_select_clear(gsdf_ctx* c);
int gsdf_select_count(gsdf_ctx* c, int64_t* n_voxels, int64_t* n_blocks);
int gsdf_select_export(gsdf_ctx* c, int32_t* keys, float* payload, int64_t max_n, int64_t* n, int raw_sums);
int gsdf_select_export_raw_dev(gsdf_ctx* c, int32_t* keys_dev, float* payload_raw_dev, int64_t max_n, int64_t* n);
int gsdf_erase_selected(gsdf_ctx* c, int64_t* n_voxels, int64_t* n_blocks_emptied);
int gsdf_compact(gsdf_ctx* c, int new_capacity_log2 /* 0 = keep */, int64_t* n_blocks_dropped);

/* Voxel-hash raycaster: depth (camera z, 0 = no hit) and camera-frame normals (3 planes, nullable) of the
 * fused map seen from pose (R, t) through K.  Named in BASELINE.json's north_star but ABSENT from the
 * reference: it is defined on top of Sdf::weights / Sdf::tsdf (MapGradPixelSdf.h:109-125) and the
 * tracker's back-projection (RigidPointOptimizer.cpp:46-47,67-70); DESIGN.md states the definition. */
int gsdf_raycast(gsdf_ctx* c, const float K[9], const float R[9], const float t[3], int W, int H, float zmin, float zmax,
                 float* depth_out, float* normals_out);

/* the same with DEVICE output buffers (depth W*H floats, normals 3*W*H floats or NULL); enqueue only */
int gsdf_raycast_dev(gsdf_ctx* c, const float K[9], const float R[9], const float t[3], int W, int H, float zmin, float zmax,
                     float* depth_dev, float* normals_dev);
/* what the raycasts since the last reset did: samples their definition evaluated (one block-key probe each) and voxel records
 * read -- the algorithmic bytes of the raycaster's roofline entry are 8 B per sample + 32 B per record + 16 B per pixel.
 * Synchronises; reset != 0 clears the counters. */
int gsdf_raycast_counters(gsdf_ctx* c, int64_t* samples, int64_t* records, int reset);

/* Iso-surface of the map on the device -- LayeredMarchingCubesNoColor::computeIsoSurface + computeLutIndex + interpolate +
 * computeTriangles (mesh/LayeredMarchingCubesNoColor.cpp:354-712), called by MapGradPixelSdf::extract_mesh
 * (MapGradPixelSdf.cpp:124-175).  tri_table: NULL = the reference's triTable (:96-352, the classic marching-cubes
 * cases, constant data in include/gsdf_mc_tables.h), which gives the reference's mesh triangle for triangle; or a
 * caller's 256 x 16 table (edge ids, 3 per triangle, -1 ends a row; corner / edge numbering of :599-606, :410-549).
 * triangles_out: 9 floats per triangle, in the reference's z-y-x sweep order, no vertex de-duplication, degenerate
 * triangles dropped.  *n_tris = triangles found; call with max_tris = 0 to size the buffer. */
int gsdf_extract_mesh(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16], float* triangles_out, int64_t max_tris,
                      int64_t* n_tris);

/* The same iso-surface as an INDEXED mesh: one vertex per crossed grid edge, faces as vertex ids, a normal per vertex from the
 * stored gradients.  Not in the reference (its meshes are triangle soups, computeTriangles :686-712 pushes three fresh vertices
 * per face); defined on top of gsdf_extract_mesh (computeIsoSurface / computeLutIndex / interpolate,
 * mesh/LayeredMarchingCubesNoColor.cpp:354-712) and of the cloud export's normal (extract_pc, MapGradPixelSdf.cpp:186-192:
 * normal = -g^).
 *  - Faces: exactly the triangles of gsdf_extract_mesh(iso, tri_table), in its order (z-y-x sweep, table order within a cube)
 *    and with its corner order.  The degenerate-triangle rule is the soup's (:686-712: position equality of the cube's own three
 *    interpolations); nothing is filtered again after welding.  The three ids of a face are distinct (a table triangle names
 *    three different cube edges).
 *  - Vertex identity: the GRID EDGE a corner lies on -- its lower endpoint voxel relative to the bounding-box minimum (z, then
 *    y, then x, 20 bits each, as the sweep order's key) followed by the axis (0 x, 1 y, 2 z) in 2 bits.  Position bits are not
 *    the identity: neighbouring cubes walk a grid edge in opposite directions (cube edge 0 runs -y, edge 2 +y: getVertex
 *    :410-549) and interpolate (:642-662) need not give the same bits from both ends.  Vertex ids are the ranks of the distinct
 *    edge keys in ascending order.
 *  - Position: that of the vertex's CANONICAL corner, the first soup corner on the edge in sweep order (face index, then corner
 *    0..2): interpolate's result for that cube, unchanged.  So vertices[faces[f][k]] differs from the soup's corner only where the
 *    other direction of the walk rounds differently.
 *  - Normal (normals_out, nullable): from the same canonical corner, with its endpoints a -> b as its cube walks the edge and
 *    interpolate's mu (0, 1, 0 on the three 1e-7 guard returns :645-650, else the clamped quotient):
 *    n = -normalized((1 - mu) g^_a + mu g^_b) in float, g^ the normalised stored gradient sum of the endpoint voxel as gsdf_query
 *    and the cloud export normalise it; (0, 0, 0) when the blend's norm is 0 or not finite.  Base contexts store the same sums.
 * Conventions of gsdf_extract_mesh: tri_table NULL = the reference's table; max_vertices = max_faces = 0 sizes the buffers;
 * *n_vertices and *n_faces are always reported; if either maximum is too small nothing is written to any buffer and the call
 * returns GSDF_ERR_INVALID; an empty map gives 0 / 0 and GSDF_OK; the table is only read; coordinates relative to the
 * bounding-box minimum are taken at 20 bits per axis, as in gsdf_extract_mesh's sweep key -- an edge's lower endpoint may lie one
 * voxel beyond a cube's anchor, so the keys are distinct for a bounding box of up to 2^20 - 1 voxels per axis (the sweep key's
 * limit is 2^20).  At most (2^31 - 1) / 3 faces.
 * Deterministic: the same map gives the same bytes, run to run and across gsdf_grow. */
int gsdf_extract_mesh_indexed(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16],
                              float* vertices_out /* 3 per vertex */, float* normals_out /* 3 per vertex, nullable */,
                              int32_t* faces_out /* 3 per face */, int64_t max_vertices, int64_t max_faces,
                              int64_t* n_vertices, int64_t* n_faces);

/* CONNECTED COMPONENTS of the indexed mesh, and the mesh without its small fragments.  Not in the reference (a triangle soup has
 * no neighbours to find).  Noise at depth edges leaves isolated voxels in a fused map, and marching cubes turns them into islands
 * of a face or two beside the scanned surface.
 *  - Mesh and graph: the mesh is that of gsdf_extract_mesh_indexed(iso, tri_table) -- the same vertices, ids, faces and order.
 *    Two vertices are adjacent iff some face names both; a component is a connected component of that graph.  Faces that share
 *    only a vertex are therefore connected.  Every vertex lies in a face, so every component has at least one face.
 *  - Component ids: 0 .. C-1 in ascending order of the component's smallest vertex id (component 0 holds vertex 0).  A function
 *    of the mesh alone, not of any order of execution.
 * gsdf_mesh_components: vertex_comp[v] the id per vertex; face_comp[f] the id per face (the component of its vertices);
 * comp_counts 2 int32 per component: faces, vertices; comp_bbox 6 floats per component: min x, y, z then max x, y, z of its vertex
 * positions (the floats of vertices_out; where a component holds both zeros, either sign of zero may be reported).  Each of the
 * four arrays may be NULL.  max_vertices belongs to vertex_comp, max_faces to face_comp, max_components to comp_counts and
 * comp_bbox.  Conventions of gsdf_extract_mesh_indexed: all three maxima 0 sizes the outputs; the three counts are always
 * reported; if a maximum that belongs to a non-NULL array is too small nothing is written to any array and the call returns
 * GSDF_ERR_INVALID; an empty map gives 0 / 0 / 0 and GSDF_OK; the table is only read; base contexts are accepted.
 * Deterministic: the same map gives the same bytes, run to run and across gsdf_grow. */
int gsdf_mesh_components(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16],
                         int32_t* vertex_comp /* 1 per vertex, nullable */, int32_t* face_comp /* 1 per face, nullable */,
                         int64_t max_vertices, int64_t max_faces,
                         int32_t* comp_counts /* 2 per component, nullable */, float* comp_bbox /* 6 per component, nullable */,
                         int64_t max_components, int64_t* n_vertices, int64_t* n_faces, int64_t* n_components);

/* gsdf_extract_mesh_indexed restricted to the components that are kept:
 *  - min_faces >= 1 keeps the components with at least that many faces; min_faces == GSDF_MESH_KEEP_LARGEST keeps the one
 *    component with the most faces, among equals the one with the lowest id; any other value is GSDF_ERR_INVALID.
 *  - Output vertices are the kept vertices in ascending original id, position and normal bytes unchanged; a vertex's new id is
 *    its rank among the kept.  Output faces are the kept faces in their original order with the ids remapped.
 *  - *n_vertices and *n_faces are the FILTERED counts, which is also what the sizing call (both maxima 0) reports;
 *    *n_components counts all components, *n_kept the kept ones.  All four are always reported.
 *  - min_faces = 1 returns the bytes of gsdf_extract_mesh_indexed.  A threshold above every component gives 0 / 0 and GSDF_OK.
 * Otherwise the conventions of gsdf_extract_mesh_indexed (normals_out nullable; a maximum that is too small: nothing is written,
 * GSDF_ERR_INVALID).  Deterministic in the same sense. */
#define GSDF_MESH_KEEP_LARGEST (-1)
int gsdf_extract_mesh_indexed_filtered(gsdf_ctx* c, float iso, const int8_t tri_table[256 * 16], int64_t min_faces,
                                       float* vertices_out /* 3 per vertex */, float* normals_out /* 3 per vertex, nullable */,
                                       int32_t* faces_out /* 3 per face */, int64_t max_vertices, int64_t max_faces,
                                       int64_t* n_vertices, int64_t* n_faces, int64_t* n_components, int64_t* n_kept);

/* GRADIENT ACCURACY on a sphere scene: the angle between a voxel's gradient and the analytic one, for the gradient the map
 * STORES and for finite differences of the stored distances, and its statistics over the voxels near the surface -- the paper's
 * central measurement (matlab/GradientAnalysisSpheres.m, matlab/phi_statistics.m), on the map in HBM instead of save_sdf's text
 * files.  All arithmetic is DOUBLE unless stated; its inputs are the floats the map holds.
 *  - Voxels and grid: a voxel exists iff w > 0.  dist is bit for bit gsdf_export(raw_sums = 0)'s; g^_1 is the stored gradient
 *    sum, normalised (:59-75).  D(v) = dist of an existing voxel, else the context's trunc_dist (D = vs*T*ones(sz), :55); a
 *    neighbour outside the packable key range is missing.  The grid is the bounding box of all existing voxels (save_sdf's
 *    `voxel min` / `voxel max`, copied in :48-50).
 *  - Estimators, per existing voxel, each normalised (a zero or non-finite vector: NaN):
 *      0 stored    g^_1 (:59-75)
 *      1 central   gradient(D, vs) (:81-87), per axis (D[i+1] - D[i-1]) / (2 vs) inside the box, (D[i+1] - D[i]) / vs on the box's
 *                  minimal face, (D[i] - D[i-1]) / vs on its maximal face, 0 where the box is one voxel thick on that axis
 *      2 forward   vs_inv (D[i+1] - D[i]), 0 on the maximal face (:117-130)
 *      3 backward  vs_inv (D[i] - D[i-1]), 0 on the minimal face (:136-149)
 *    with vs the context's voxel size widened to double and vs_inv = 1 / vs.
 *  - Ground truth (:96-111): the voxel centre c = vs * (float)idx, a float product as the project forms voxel centres, widened
 *    to double; n_spheres rows cx cy cz R; the sphere maximising R - |c - centre| (the first among equals) gives
 *    g = normalized(c - centre) (NaN for a voxel centre on a sphere centre: all four angles undefined).
 *  - Angle (:162-163): phi_e = acosd(min(|g^_e . g|, 1)), stored as float32 degrees; NaN marks an undefined estimator.
 *  - Statistics (phi_statistics.m:69-73) for ascending thresholds d[0..n_thr): over the voxels with fabsf(dist) < d[k] (a float
 *    compare) and phi_e not NaN: count, mean, rmse = sqrt(mean(phi^2)), median and 95th percentile of the float32 phi values,
 *    in double.  Percentiles are MATLAB's prctile: for sorted x[1..n] the position n p / 100 + 0.5, clamped to [1, n], linear in
 *    between (numpy's method="hazen").  An empty subset gives count 0 and NaN for the rest.
 * Stated deviations: the script reads 6-digit text and takes vs*T in double, here the map's own floats and trunc_dist are used;
 * phi_statistics' hist2d output and the plots are not part of this.
 * Conventions: max_n = 0 (keys and rows5 may be NULL) sizes the output; a buffer that is too small: nothing is written,
 * GSDF_ERR_INVALID, the need in *n; an empty map gives *n = 0 / count 0 with NaN, GSDF_OK.  GSDF_ERR_INVALID with nothing
 * written: n_spheres outside 1..64, n_thr outside 1..256, thresholds that are not finite, not positive or not strictly
 * ascending, a sphere row that is not finite or has R <= 0, NULL inputs.  Synchronous.  The table is only read: the map, a
 * ColorUpsampler snapshot and PhotoBA state stay as they are; a waiting pipelined fusion is launched first.  Base-sdf contexts
 * are accepted (they store the same sums).  At most 2^31 - 1 voxels.
 * Deterministic: no floating-point atomics, every sum taken in one fixed order over sorted arrays -- the same map gives the
 * same bytes, run to run and across gsdf_grow. */
/* rows5 per voxel: dist, phi[4] (degrees; NaN = undefined); rows and keys in the order of gsdf_export(sorted = 1) */
int gsdf_gradient_angles(gsdf_ctx* c, const float* spheres4_host, int n_spheres,
                         int32_t* keys, float* rows5, int64_t max_n, int64_t* n);
/* stats: 4 x n_thr x 5 doubles = count, mean, median, rmse, p95; estimator order as above */
int gsdf_gradient_stats(gsdf_ctx* c, const float* spheres4_host, int n_spheres,
                        const float* thresholds, int n_thr, double* stats);

/* device-memory plumbing so callers can stage frames in HBM without another runtime */
int gsdf_dev_alloc(gsdf_ctx* c, void** dev_ptr, int64_t bytes);
int gsdf_dev_free(gsdf_ctx* c, void* dev_ptr);          /* withdraws a next-frame hint that lies in the freed allocation */
int gsdf_dev_upload(gsdf_ctx* c, void* dev_dst, const void* host_src, int64_t bytes);
int gsdf_dev_download(gsdf_ctx* c, void* host_dst, const void* dev_src, int64_t bytes);
/* Asynchronous frame staging for a host loop that keeps the GPU fed (the Scan3D CLI): page-locked host
 * buffers, an upload that is only ENQUEUED on the context's stream (host_src must stay untouched until a later mark is
 * reached), and marks: gsdf_mark records a point in the stream, gsdf_mark_wait blocks until the stream has passed it,
 * gsdf_mark_reached polls.  Marks complete in the order they were recorded.  A reached mark orders STREAM PROGRESS only (the
 * kernels and copies queued before it have run: a staging slot may be reused); its event carries no system-scope fence, so it
 * does NOT make device writes visible to the host -- read results through gsdf_sync or the download / export entries. */
int gsdf_host_alloc(gsdf_ctx* c, void** host_ptr, int64_t bytes);
int gsdf_host_free(gsdf_ctx* c, void* host_ptr);
int gsdf_dev_upload_async(gsdf_ctx* c, void* dev_dst, const void* host_src, int64_t bytes);
int gsdf_mark(gsdf_ctx* c, int64_t* mark);
int gsdf_mark_wait(gsdf_ctx* c, int64_t mark);
int gsdf_mark_reached(gsdf_ctx* c, int64_t mark, int* reached);
/* Staging AHEAD of the stream: the copy runs on the context's copy stream -- a DMA engine beside the kernels of the frames
 * before it, where gsdf_dev_upload_async queues behind them and makes the stream change engines twice per frame --
 * and gsdf_upload_wait blocks the HOST until that copy has arrived; after it returned, dev_dst may be handed to any _dev entry.
 * The caller keeps dev_dst out of the stream's reach meanwhile (a buffer whose last reader passed a mark) and host_src
 * untouched until the wait returned.  Uploads complete in the order they were started. */
int gsdf_dev_upload_ahead(gsdf_ctx* c, void* dev_dst, const void* host_src, int64_t bytes, int64_t* upload);
int gsdf_upload_wait(gsdf_ctx* c, int64_t upload);
/* HIP-event timing on the context's stream: t0/t1 bracket whatever is enqueued between them */
int gsdf_timer_start(gsdf_ctx* c);
int gsdf_timer_stop_ms(gsdf_ctx* c, float* ms);          /* synchronises */
/* accumulated per-kernel HIP-event time (ms) and launch counts since the last reset:
 * index 0 normals, 1 fusion, 2 tracking pass.  Enabled by gsdf_profile(c, 1). */
int gsdf_profile(gsdf_ctx* c, int enable);
int gsdf_profile_read(gsdf_ctx* c, double ms[3], int64_t launches[3]);
/* the first n <= 5 slots: 0 normals, 1 fusion, 2 tracking pass launches, 3 raycast, 4 reserved */
int gsdf_profile_read_n(gsdf_ctx* c, int n, double* ms, int64_t* launches);
/* every launch of one slot by itself, in launch order (ms each; at most 2^20 kept): *n = launches recorded since the last
 * gsdf_profile(c, 1), the first min(max_n, *n) durations in ms[].  Lets a caller tell the tracker launches that ran a pass from
 * the head-only ones and those that found optimize() already ended (bench.py: roofline.tracker per executed pass). */
int gsdf_profile_read_launches(gsdf_ctx* c, int slot, float* ms, int64_t max_n, int64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* GSDF_H_ */
