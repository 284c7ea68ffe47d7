#!/usr/bin/env python3
"""Map-to-map registration at bench scale -- measured, not gated.

Fuses the two halves of the 640x480 S-tum stream (1 cm voxels, trunc 10) into two maps A and B at their ground-truth poses, takes
B's surface cloud on the device (gsdf_surface_cloud_dev), moves it into a source frame by 1 degree about (0.3, -0.5, 0.8) and
(0.01, -0.008, 0.006) m, and registers it against A from the identity (gsdf_align_points_dev).  Reports points, hits, passes, the
final E / hits, the recovered pose's error, the wall time of the call (median of `--reps` after one warm call), and the HIP-event
time of one batch of 5 pass + head pairs divided by 5 (conv_threshold = 0, so all five run) next to the event time of
k_track_pass's launches on map A for a frame of the stream.  One JSON line, also written to profiles/align_points.json (or --out).
--merge goes on to the merge under the recovered pose instead (merge_main): profiles/merge_posed.json.
--multi measures the multi-start registration instead (multi_main): profiles/align_multi.json.
--robust measures the registration with a robust loss beside the plain one (robust_main): profiles/align_robust.json.
--erase-moved erases what moved between two sessions before merging them, and times the selection entries (erase_main):
profiles/erase.json."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def quat_to_R(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    """the unit quaternion x y z w of a rotation matrix with positive trace (the stream's camera poses)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    w = 0.5 * np.sqrt(1.0 + np.trace(R))
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w], np.float32)


def merge_main(args):
    """--merge: B is fused in a frame of its OWN (every pose of its half premultiplied by the inverse of the displacement), its
    cloud registered against A as it is, and B merged into a copy of A under the recovered pose and under the true one
    (gsdf_merge_from_posed).  Reports the counts, the candidate blocks before / after unique, the wall time of the call (median of
    --reps, each into a fresh copy of A), the event times of its stages, the wall time of gsdf_merge_from on the same two maps for
    scale, and the median / 95th percentile of |phi| that A alone and the two merged maps return at the surface-cloud points of a
    map fused from ALL frames at their ground-truth poses.  One JSON line, also written to profiles/merge_posed.json (or --out)."""
    import __graft_entry__ as graft
    import align_points_ref as ref
    pkg = graft.package()
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    vs = np.float32(0.01); T = np.float32(10) * vs
    new = lambda: pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    a, b, full = new(), new(), new()
    frames = [seq.frame(i) for i in range(n)]
    _, Rd, td = ref.displace(np.zeros((1, 3)))
    for i in range(n):
        d, R, t = frames[i]
        full.update(d, R, t)
        if i < n // 2:
            a.update(d, R, t)
        else:                                           # B's own frame: x_b = Rd^T (x - td)
            b.update(d, (Rd.T @ np.asarray(R, np.float64).reshape(3, 3)).astype(np.float32), (Rd.T @ (np.asarray(t, np.float64) - td)).astype(np.float32))
    cloud_b = b.surface_cloud()
    conv, pose, passes, trace = a.align_points(cloud_b[:, :3], ref.IDENTITY)
    true = np.concatenate([td.astype(np.float32), R_to_quat(Rd)]).astype(np.float32)
    Rg = quat_to_R(pose[3:])
    ang = float(np.rad2deg(np.arccos(np.clip((np.trace(Rg.T @ Rd) - 1) / 2, -1, 1))))
    terr = float(np.abs(pose[:3].astype(np.float64) - td).max())
    probe = full.surface_cloud()[:, :3]

    hit_a = a.query(probe)[2] > 0

    def phi_stats(g):
        """over the points the map answers, and over those of them that A alone answers too (the same set for every map)"""
        phi, _, w = g.query(probe)
        out = {}
        for name, hit in (("", w > 0), ("_where_a_hits", (w > 0) & hit_a)):
            v = np.abs(phi[hit].astype(np.float64))
            out.update({"points_hit" + name: int(hit.sum()), "median_mm" + name: round(1e3 * float(np.median(v)), 4),
                        "p95_mm" + name: round(1e3 * float(np.percentile(v, 95)), 4)})
        return out

    def copy_of_a():
        g = new()
        g.merge_from(a)
        return g
    res = {}
    for name, p in (("true_pose", true), ("recovered_pose", pose)):
        g = copy_of_a()
        nv, nb = g.merge_from_posed(b, p)
        (cand, uniq), ms = g.merge_posed_last()
        res[name] = {"n_voxels": nv, "n_blocks": nb, "candidate_blocks": int(cand), "candidate_blocks_unique": int(uniq),
                     "event_ms": {"candidates_fill": round(float(ms[0]), 4), "sort_unique": round(float(ms[1]), 4),
                                  "k_posed_sample": round(float(ms[2]), 4), "k_posed_add": round(float(ms[3]), 4)},
                     "voxels_after": g.count(), "abs_phi_at_full_map_cloud": phi_stats(g)}
        g.close()
    ts, tm = [], []
    for _ in range(args.reps + 1):                      # the first one warm
        g = copy_of_a()
        t0 = time.perf_counter(); g.merge_from_posed(b, pose); ts.append(time.perf_counter() - t0)
        g.close()
        g = copy_of_a()
        t0 = time.perf_counter(); g.merge_from(b); tm.append(time.perf_counter() - t0)
        g.close()
    out = {"map": "S-tum %dx%d, %d frames (A = first half, B = second half in a frame of its own), voxel %.3g m" % (W, H, n, float(vs)),
           "voxels_a": a.count(), "voxels_b": b.count(), "blocks_b": int(len(np.unique(b.export()[0] >> 2, axis=0))),
           "registration": {"points": int(len(cloud_b)), "converged": bool(conv), "passes": int(passes),
                            "rotation_error_deg": round(ang, 4), "translation_error_mm": round(1e3 * terr, 3)},
           "merge": res, "reps": args.reps,
           "merge_from_posed_wall_ms": round(float(np.median(ts[1:])) * 1e3, 3),
           "merge_from_wall_ms_same_maps_for_scale": round(float(np.median(tm[1:])) * 1e3, 3),
           "abs_phi_at_full_map_cloud_a_alone": phi_stats(a), "full_map_cloud_points": int(len(probe))}
    a.close(); b.close(); full.close()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


def multi_main(args):
    """--multi: the same two maps; B's cloud displaced by 2 degrees about (0.3, -0.5, 0.8) and 0.2 m along (1, 1, -1) / sqrt(3),
    registered from m = 27 (offsets on the 0.1 m grid, k = 1) and m = 125 (k = 2) starts around the identity with the cloud's
    centroid as pivot.  Per m: the wall time of ONE gsdf_align_points_multi_dev call next to the wall time of the same starts as m
    sequential gsdf_align_points_dev calls (both the median of --reps after a warm call, same process), the runs still live at
    the start of every batch of launch pairs (from the pass counts: a run is queued in a batch iff it has not ended before it),
    and the HIP-event time of a pass + head pair with all m runs live (a 5-pair batch with conv_threshold = 0, divided by 5).
    Then the basin: initial errors of 1, 2, 5, 10, 20 degrees crossed with 1, 5, 10, 20, 30 cm, per cell the final error of the
    single start from the identity and of the picks among the 27 and the 125 starts (converged, at least half the points
    hitting).  One JSON line, also written to profiles/align_multi.json (or --out)."""
    import __graft_entry__ as graft
    import align_points_ref as ref
    pkg = graft.package()
    B = pkg.binding
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    vs = np.float32(0.01); T = np.float32(10) * vs
    a = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    b = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    frames = [seq.frame(i) for i in range(n)]
    for i in range(n // 2):
        a.update(*frames[i])
    for i in range(n // 2, n):
        b.update(*frames[i])
    cloud = b.surface_cloud()[:, :3]
    npts = len(cloud)
    u = np.array([1.0, 1.0, -1.0]) / np.sqrt(3.0)

    def errors(pose, Rd, td):
        Rg = quat_to_R(pose[3:])
        return (round(float(np.rad2deg(np.arccos(np.clip((np.trace(Rg.T @ Rd) - 1) / 2, -1, 1)))), 4),
                round(1e3 * float(np.abs(pose[:3].astype(np.float64) - td).max()), 3))

    def grids(src):
        piv = src.astype(np.float64).mean(axis=0)
        return {27: B.align_starts(ref.IDENTITY, piv, 0.0, 0, 0.1, 1), 125: B.align_starts(ref.IDENTITY, piv, 0.0, 0, 0.1, 2)}

    def pick(dev, starts, Rd, td):
        fl, poses, ps, last, _ = a.align_points_multi_dev(dev, npts, starts)
        best = B.align_best(fl, ps, last, npts // 2, True)
        if best < 0:
            return {"pick": -1}
        ang, terr = errors(poses[best], Rd, td)
        return {"pick": int(best), "passes": int(ps[best]), "hits": int(last[best, 28]), "rotation_error_deg": ang, "translation_error_mm": terr}

    src, Rd, td = ref.displace(cloud, rot_deg=2.0, tr=tuple(0.2 * u))
    dev = a.upload(src)
    timing = {}
    for m, starts in grids(src).items():
        fl, poses, ps, last, _ = a.align_points_multi_dev(dev, npts, starts)             # warm, and the pass counts
        for s in starts[:2]:
            a.align_points_dev(dev, npts, s)
        tm, tq = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); a.align_points_multi_dev(dev, npts, starts); tm.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for s in starts:
                a.align_points_dev(dev, npts, s)
            tq.append(time.perf_counter() - t0)
        a.timer_start()
        a.align_points_multi_dev(dev, npts, starts, iters=5, conv=0.0)
        pair_ms = a.timer_stop_ms() / 5
        edges, q = [], 0
        while q < 25:                                   # the batches of the call: first_batch = 5, then next_batch = 8
            edges.append(q)
            q += 5 if q == 0 else 8
        best = B.align_best(fl, ps, last, npts // 2, True)
        ang, terr = errors(poses[best], Rd, td) if best >= 0 else (None, None)
        timing[str(m)] = {"multi_call_wall_ms": round(float(np.median(tm)) * 1e3, 3),
                          "sequential_single_calls_wall_ms": round(float(np.median(tq)) * 1e3, 3),
                          "ratio_sequential_over_multi": round(float(np.median(tq) / np.median(tm)), 2),
                          "passes": [int(v) for v in ps], "converged": int(fl.sum()),
                          "live_at_batch_start": {str(e): int((ps > e).sum()) for e in edges},
                          "pass_plus_head_pair_event_us_all_live": round(float(pair_ms) * 1e3, 2),
                          "workgroups_per_pass_all_live": int(min(max((npts + 255) // 256, 1), 512)) * m,
                          "pick": int(best), "rotation_error_deg": ang, "translation_error_mm": terr}
    a.timer_start()
    a.align_points_dev(dev, npts, ref.IDENTITY, iters=5, conv=0.0)
    single_pair_us = round(a.timer_stop_ms() * 1e3 / 5, 2)
    basin = []
    for deg in (1, 2, 5, 10, 20):
        for cm in (1, 5, 10, 20, 30):
            src, Rd, td = ref.displace(cloud, rot_deg=float(deg), tr=tuple(0.01 * cm * u))
            d = a.upload(src)
            c1, p1, u1, _ = a.align_points_dev(d, npts, ref.IDENTITY)
            ang1, terr1 = errors(p1, Rd, td)
            g = grids(src)
            basin.append({"deg": deg, "cm": cm,
                          "single": {"converged": bool(c1), "passes": int(u1), "rotation_error_deg": ang1, "translation_error_mm": terr1},
                          "pick_of_27": pick(d, g[27], Rd, td), "pick_of_125": pick(d, g[125], Rd, td)})
    out = {"map": "S-tum %dx%d, %d frames (A = first half, B = second half), voxel %.3g m" % (W, H, n, float(vs)),
           "points": int(npts), "reps": args.reps, "displacement": "2 deg about (0.3, -0.5, 0.8), 0.2 m along (1, 1, -1) / sqrt(3)",
           "starts": {"27": "offsets {-0.1, 0, 0.1} m per axis", "125": "offsets {-0.2 .. 0.2} m per axis, step 0.1 m"},
           "timing": timing, "single_pass_plus_head_pair_event_us": single_pair_us, "basin": basin}
    a.close(); b.close()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


def robust_main(args):
    """--robust: the registration with a robust loss (gsdf_align_points_robust, Tukey at 2 cm) beside the plain one, on two scenes.
    (1) The demonstration scene of tests/test_gpu_align_robust.py: 320x240 spheres, 1 cm voxels, trunc 10, sessions A (frames 0..7)
    and B (frames 4..11), the third sphere of B moved by (0.04, -0.02, 0.012) m.  (2) The bench-stream pair of the other modes with
    a block of B's cloud displaced: the points inside a 0.5 m cube about the cloud's centroid are shifted by (0.05, -0.03, 0.02) m.
    Per scene: the pose errors of the plain and of the robust run from the identity, and from gsdf_align_residuals under either
    pose the hit points with |phi| >= 2 cm, and how many of them belong to the part that moved.  On the bench pair also the
    HIP-event time of a robust pass + head pair beside the plain pair (a 5-pair batch with conv_threshold = 0, divided by 5, median
    of --reps) and the wall time of a 27-start robust call beside the plain 27-start call, all in this process.  One JSON line,
    also written to profiles/align_robust.json (or --out)."""
    import __graft_entry__ as graft
    import align_points_ref as ref
    pkg = graft.package()
    B = pkg.binding
    LOSS, SCALE = B.LOSS_TUKEY, np.float32(0.02)

    def errors(pose, Rd, td):
        Rg = quat_to_R(pose[3:])
        return (round(float(np.rad2deg(np.arccos(np.clip((np.trace(Rg.T @ Rd) - 1) / 2, -1, 1)))), 4),
                round(1e3 * float(np.abs(pose[:3].astype(np.float64) - td).max()), 3))

    def compare(a, dev, npts, Rd, td, moved):
        """the plain and the robust run from the identity; `moved`: bool [npts], the points that do not belong"""
        res = {}
        for name, run in (("l2", lambda: a.align_points_dev(dev, npts, ref.IDENTITY)),
                          ("tukey_2cm", lambda: a.align_points_robust_dev(dev, npts, ref.IDENTITY, LOSS, SCALE))):
            conv, pose, passes, trace = run()
            ang, terr = errors(pose, Rd, td)
            phi, w = a.align_residuals_dev(dev, npts, pose)
            off = (w > 0) & (np.abs(phi) >= SCALE)
            res[name] = {"converged": bool(conv), "passes": int(passes), "rotation_error_deg": ang, "translation_error_mm": terr,
                         "hits": int((w > 0).sum()), "hits_2cm_or_more_off": int(off.sum()), "of_which_moved": int((off & moved).sum()),
                         "inliers": int(((w > 0) & ~off).sum())}
            if name != "l2":
                res[name]["wsum_last_pass"] = float(trace[-1, 36]) if passes else None
                res[name]["n_in_last_pass"] = int(trace[-1, 37]) if passes else None
        return res

    # (1) the demonstration scene
    W, H = 320, 240
    kw = dict(n_frames=12, seed=1, step_deg=0.5)
    sa, sb = pkg.synth.Sequence("spheres", W, H, **kw), pkg.synth.Sequence("spheres", W, H, **kw)
    sb.spheres = np.array(sb.spheres, np.float64).copy()
    sb.spheres[2, :3] += (0.04, -0.02, 0.012)
    vs = np.float32(0.01); T = np.float32(10) * vs
    a = pkg.GradSdf(vs, T, W, H, sa.K, capacity_log2=21)
    b = pkg.GradSdf(vs, T, W, H, sa.K, capacity_log2=21)
    for i in range(8):
        a.update(*sa.frame(i))
    for i in range(4, 12):
        b.update(*sb.frame(i))
    cloud = b.surface_cloud()[:, :3]
    c, r = sb.spheres[2, :3], float(sb.spheres[2, 3])
    on_moved = np.abs(np.linalg.norm(cloud.astype(np.float64) - c, axis=1) - r) < 2.0 * float(vs)
    src, Rd, td = ref.displace(cloud)
    demo = {"scene": "spheres %dx%d, A = frames 0..7, B = frames 4..11 with sphere 2 moved by (0.04, -0.02, 0.012) m, voxel %.3g m" % (W, H, float(vs)),
            "points": int(len(src)), "points_on_the_moved_sphere": int(on_moved.sum())}
    demo.update(compare(a, a.upload(src), len(src), Rd, td, on_moved))
    a.close(); b.close()

    # (2) the bench-stream pair with a block of B's cloud displaced
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    a = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    b = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    frames = [seq.frame(i) for i in range(n)]
    for i in range(n // 2):
        a.update(*frames[i])
    for i in range(n // 2, n):
        b.update(*frames[i])
    cloud = b.surface_cloud()[:, :3].copy()
    npts = len(cloud)
    block = (np.abs(cloud.astype(np.float64) - cloud.astype(np.float64).mean(axis=0)) < 0.25).all(axis=1)
    cloud[block] += np.array([0.05, -0.03, 0.02], np.float32)
    src, Rd, td = ref.displace(cloud)
    dev = a.upload(src)
    bench = {"scene": "S-tum %dx%d, %d frames (A = first half, B = second half), voxel %.3g m; B's points within 0.25 m of the centroid per axis moved by (0.05, -0.03, 0.02) m" % (W, H, n, float(vs)),
             "points": int(npts), "points_in_the_moved_block": int(block.sum())}
    bench.update(compare(a, dev, npts, Rd, td, block))
    # timings, the plain kernels and the robust ones side by side in this process
    starts = B.align_starts(ref.IDENTITY, src.astype(np.float64).mean(axis=0), 0.0, 0, 0.1, 1)
    pair_l2, pair_rb, call_l2, call_rb, multi_l2, multi_rb = [], [], [], [], [], []
    a.align_points_dev(dev, npts, ref.IDENTITY); a.align_points_robust_dev(dev, npts, ref.IDENTITY, LOSS, SCALE)       # warm
    a.align_points_multi_dev(dev, npts, starts); a.align_points_multi_robust_dev(dev, npts, starts, LOSS, SCALE)
    for _ in range(args.reps):
        a.timer_start(); a.align_points_dev(dev, npts, ref.IDENTITY, iters=5, conv=0.0); pair_l2.append(a.timer_stop_ms() / 5)
        a.timer_start(); a.align_points_robust_dev(dev, npts, ref.IDENTITY, LOSS, SCALE, iters=5, conv=0.0); pair_rb.append(a.timer_stop_ms() / 5)
        t0 = time.perf_counter(); a.align_points_dev(dev, npts, ref.IDENTITY, conv=0.0); call_l2.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); a.align_points_robust_dev(dev, npts, ref.IDENTITY, LOSS, SCALE, conv=0.0); call_rb.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); a.align_points_multi_dev(dev, npts, starts, conv=0.0); multi_l2.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); a.align_points_multi_robust_dev(dev, npts, starts, LOSS, SCALE, conv=0.0); multi_rb.append(time.perf_counter() - t0)
    t0 = time.perf_counter(); a.align_residuals_dev(dev, npts, ref.IDENTITY); t_res = time.perf_counter() - t0
    med = lambda v, k: round(float(np.median(v)) * k, 3)                   # noqa: E731
    bench["timing"] = {"note": "conv_threshold = 0: every call runs all its passes, so both losses do the same number of launches",
                       "pass_plus_head_pair_event_us": {"l2": med(pair_l2, 1e3), "tukey_2cm": med(pair_rb, 1e3)},
                       "call_25_passes_wall_ms": {"l2": med(call_l2, 1e3), "tukey_2cm": med(call_rb, 1e3)},
                       "call_27_starts_25_passes_wall_ms": {"l2": med(multi_l2, 1e3), "tukey_2cm": med(multi_rb, 1e3)},
                       "residuals_call_wall_ms": round(t_res * 1e3, 3),
                       "workgroups": int(min(max((npts + 255) // 256, 1), 512)), "reps": args.reps}
    a.close(); b.close()
    out = {"loss": "TUKEY", "scale_m": float(SCALE), "demonstration": demo, "bench_pair": bench}
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


def erase_main(args):
    """--erase-moved: the scene of --robust (320x240 spheres, session B with its third sphere moved, B fused in a frame of its
    own) taken to a merged map that holds the moved object once.  (1) B's surface cloud is registered against A with Tukey at
    2 cm.  (2) gsdf_align_residuals of each map's cloud against the OTHER map: B's under the recovered pose, A's under its inverse.
    (3) The points that hit and lie 2 cm or more off the other map are what moved.  (4) gsdf_select_points with radius = the
    truncation distance on the map the points come from.  (5) Both maps erased, then gsdf_merge_from_posed.  Reports the triangle
    and component counts of the merged map (gsdf_mesh_components) with and without the erase.  Then, on the bench-stream map
    (S-tum 640x480, --frames frames, 1 cm voxels), the wall time of every new entry (median of --reps) beside gsdf_count, a
    whole-table sweep; erase and compact run on a fresh copy of the map each time.  Nothing is gated.  One JSON line, also
    written to profiles/erase.json (or --out)."""
    import __graft_entry__ as graft
    import align_points_ref as ref
    pkg = graft.package()
    B = pkg.binding
    LOSS, SCALE = B.LOSS_TUKEY, np.float32(0.02)
    W, H = 320, 240
    kw = dict(n_frames=12, seed=1, step_deg=0.5)
    sa, sb = pkg.synth.Sequence("spheres", W, H, **kw), pkg.synth.Sequence("spheres", W, H, **kw)
    sb.spheres = np.array(sb.spheres, np.float64).copy()
    sb.spheres[2, :3] += (0.04, -0.02, 0.012)
    vs = np.float32(0.01); T = np.float32(10) * vs
    new = lambda: pkg.GradSdf(vs, T, W, H, sa.K, capacity_log2=21)   # noqa: E731
    a, b = new(), new()
    _, Rd, td = ref.displace(np.zeros((1, 3)))
    for i in range(8):
        a.update(*sa.frame(i))
    for i in range(4, 12):                              # B's own frame: x_b = Rd^T (x - td)
        d, R, t = sb.frame(i)
        b.update(d, (Rd.T @ np.asarray(R, np.float64).reshape(3, 3)).astype(np.float32), (Rd.T @ (np.asarray(t, np.float64) - td)).astype(np.float32))
    cloud_a, cloud_b = a.surface_cloud()[:, :3].copy(), b.surface_cloud()[:, :3].copy()
    conv, pose, passes, _ = a.align_points_robust(cloud_b, ref.IDENTITY, LOSS, SCALE)
    Rg = quat_to_R(pose[3:])
    inv = np.concatenate([-(Rg.T @ pose[:3].astype(np.float64)), [-pose[3], -pose[4], -pose[5], pose[6]]]).astype(np.float32)
    phi_b, w_b = a.align_residuals(cloud_b, pose)
    phi_a, w_a = b.align_residuals(cloud_a, inv)
    off_b, off_a = (w_b > 0) & (np.abs(phi_b) >= SCALE), (w_a > 0) & (np.abs(phi_a) >= SCALE)

    def copy_of(g):
        c = new()
        c.merge_from(g)
        return c

    def merged(erase):
        a2, b2 = copy_of(a), copy_of(b)
        info = {}
        if erase:
            na = a2.select_points(cloud_a[off_a], T)
            nb = b2.select_points(cloud_b[off_b], T)
            info = {"selected_in_a": int(na), "selected_in_b": int(nb), "erased_in_a": list(a2.erase_selected()), "erased_in_b": list(b2.erase_selected())}
        nv, nbk = a2.merge_from_posed(b2, pose)
        _, fc, counts, _ = a2.mesh_components()
        info.update({"merge_n_voxels": int(nv), "merge_n_blocks": int(nbk), "voxels": a2.count(), "triangles": int(len(fc)), "components": int(len(counts)),
                     "components_of_100_faces_or_more": int((counts[:, 0] >= 100).sum()) if len(counts) else 0})
        a2.close(); b2.close()
        return info
    demo = {"scene": "spheres %dx%d, A = frames 0..7, B = frames 4..11 in a frame of its own with sphere 2 moved by (0.04, -0.02, 0.012) m, voxel %.3g m" % (W, H, float(vs)),
            "registration": {"loss": "TUKEY", "scale_m": float(SCALE), "converged": bool(conv), "passes": int(passes),
                             "rotation_error_deg": round(float(np.rad2deg(np.arccos(np.clip((np.trace(Rg.T @ Rd) - 1) / 2, -1, 1)))), 4),
                             "translation_error_mm": round(1e3 * float(np.abs(pose[:3].astype(np.float64) - td).max()), 3)},
            "cloud_points": {"a": int(len(cloud_a)), "b": int(len(cloud_b))},
            "hit_and_2cm_or_more_off_the_other_map": {"a": int(off_a.sum()), "b": int(off_b.sum())},
            "select_radius_m": float(T), "merged_without_erase": merged(False), "merged_with_erase": merged(True)}
    a.close(); b.close()

    # the time of every new entry on the bench map, beside gsdf_count
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    for i in range(n):
        g.update(*seq.frame(i))
    keys, _ = g.export()
    cloud = g.surface_cloud()[:, :3].copy()
    pts = cloud[::max(1, len(cloud) // 20000)]
    dev = g.upload(pts)
    nvox = g.count()
    mid = (vs * np.median(keys, axis=0)).astype(np.float32)
    lo, hi = mid - np.float32(0.5), mid + np.float32(0.5)
    kd, pd = g.upload(np.zeros((nvox, 3), np.int32)), g.upload(np.zeros((nvox, 5), np.float32))

    def timed(fn, reps=args.reps):
        fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter(); r = fn(); ts.append(time.perf_counter() - t0)
        return round(float(np.median(ts)) * 1e3, 3), r
    tm = {}
    tm["gsdf_count"], _ = timed(g.count)
    tm["gsdf_select_box"], n_box = timed(lambda: g.select_box(lo, hi))
    tm["gsdf_select_weight"], n_w = timed(lambda: g.select_weight(0, 5))
    tm["gsdf_select_points"], n_p = timed(lambda: g.select_points(pts, T))
    tm["gsdf_select_points_dev"], _ = timed(lambda: g.select_points_dev(dev, len(pts), T))
    tm["gsdf_select_points_dev_radius_2_voxels"], n_p2 = timed(lambda: g.select_points_dev(dev, len(pts), np.float32(2) * vs))
    tm["gsdf_select_invert"], _ = timed(g.select_invert)
    g.select_box(lo, hi)
    tm["gsdf_select_count"], _ = timed(g.select_count)
    tm["gsdf_select_export"], _ = timed(lambda: g.select_export(raw=True))
    tm["gsdf_select_export_raw_dev"], _ = timed(lambda: g.select_export_raw_dev(kd.value, pd.value, nvox))
    tm["gsdf_select_clear"], _ = timed(g.select_clear)
    te, tc, tcs, counts = [], [], [], None
    inside = ((vs * keys.astype(np.float32) >= lo) & (vs * keys.astype(np.float32) <= hi)).all(axis=1)
    live = int(len(np.unique(keys[inside] >> 2, axis=0)))   # blocks the crop keeps; the smallest capacity the 45 % rule admits for them
    small = 10
    while live * 100 > ((1 << small) // 64) * 45:
        small += 1
    for _ in range(args.reps + 1):                      # the first one warm; each on a fresh copy of the map
        c = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
        c.merge_from(g)
        c.select_box(lo, hi)
        c.select_invert()
        t0 = time.perf_counter(); ev = c.erase_selected(); te.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); dropped = c.compact(); tc.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); c.compact(small); tcs.append(time.perf_counter() - t0)
        counts = {"erased_voxels": int(ev[0]), "blocks_emptied": int(ev[1]), "blocks_dropped": int(dropped), "voxels_left": c.count(),
                  "live_blocks": live, "smallest_capacity_log2_admitted": small}
        c.close()
    tm["gsdf_erase_selected"] = round(float(np.median(te[1:])) * 1e3, 3)
    tm["gsdf_compact_same_capacity"] = round(float(np.median(tc[1:])) * 1e3, 3)
    tm["gsdf_compact_to_the_smallest_capacity_after_it"] = round(float(np.median(tcs[1:])) * 1e3, 3)
    bench = {"map": "S-tum %dx%d, %d frames, voxel %.3g m, capacity 2^22" % (W, H, n, float(vs)), "voxels": int(nvox),
             "blocks": int(len(np.unique(keys >> 2, axis=0))), "reps": args.reps, "points": int(len(pts)), "select_radius_m": float(T),
             "selected": {"box_1m": int(n_box), "weight_0_5": int(n_w), "points_radius_T": int(n_p), "points_radius_2_voxels": int(n_p2)},
             "crop_to_the_box": counts, "wall_ms": tm,
             "note": "wall time of the synchronous call from Python, median of reps after one warm call; gsdf_count is the whole-table sweep the engine already had"}
    g.close()
    out = {"erase_moved": demo, "bench_map": bench}
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--merge", action="store_true", help="also merge B into A under the recovered pose (gsdf_merge_from_posed); writes profiles/merge_posed.json")
    ap.add_argument("--multi", action="store_true", help="multi-start registration (gsdf_align_points_multi) against sequential single calls, and the basin sweep; writes profiles/align_multi.json")
    ap.add_argument("--robust", action="store_true", help="robust registration (gsdf_align_points_robust, Tukey at 2 cm) beside the plain one on a scene with a moved object, residual counts and timings; writes profiles/align_robust.json")
    ap.add_argument("--erase-moved", action="store_true", help="erase what moved between the two sessions of the --robust scene before merging them (gsdf_select_points, gsdf_erase_selected), and time the selection entries on the bench map; writes profiles/erase.json")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "merge_posed.json" if args.merge else "align_multi.json" if args.multi else
                                "align_robust.json" if args.robust else "erase.json" if args.erase_moved else "align_points.json")
    if args.erase_moved:
        return erase_main(args)
    if args.merge:
        return merge_main(args)
    if args.multi:
        return multi_main(args)
    if args.robust:
        return robust_main(args)
    import __graft_entry__ as graft
    import align_points_ref as ref
    pkg = graft.package()
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    vs = np.float32(0.01); T = np.float32(10) * vs
    a = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    b = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    frames = [seq.frame(i) for i in range(n)]
    for i in range(n // 2):
        a.update(*frames[i])
    for i in range(n // 2, n):
        b.update(*frames[i])
    m = b.surface_cloud_dev(None, 0)
    rows_dev = b.upload(np.zeros((m, 6), np.float32))
    t0 = time.perf_counter(); b.surface_cloud_dev(rows_dev, m); t_cloud = time.perf_counter() - t0
    rows = b.download(rows_dev, (m, 6), np.float32)
    src, Rd, td = ref.displace(rows[:, :3])
    dev = a.upload(src)
    conv, pose, passes, trace = a.align_points_dev(dev, m, ref.IDENTITY)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); a.align_points_dev(dev, m, ref.IDENTITY); ts.append(time.perf_counter() - t0)
    a.timer_start()
    a.align_points_dev(dev, m, ref.IDENTITY, iters=5, conv=0.0)
    batch_ms = a.timer_stop_ms()
    # the tracker's pass on the same map: frame n/2 from frame n/2 - 1's pose, every launch timed by events
    d, _, _ = frames[n // 2]
    _, R1, t1 = frames[n // 2 - 1]
    p0 = np.concatenate([np.asarray(t1, np.float32), R_to_quat(R1)]).astype(np.float32)
    a.track(d, p0, iters=5, conv=0.0)
    a.profile(1)
    a.track(d, p0, iters=5, conv=0.0)
    trk = a.profile_launches(2)
    a.profile(0)
    Rg = quat_to_R(pose[3:])
    ang = float(np.rad2deg(np.arccos(np.clip((np.trace(Rg.T @ Rd) - 1) / 2, -1, 1))))
    terr = float(np.abs(pose[:3].astype(np.float64) - td).max())
    hits = int(trace[-1, 28]) if passes else 0
    out = {"map": "S-tum %dx%d, %d frames (A = first half, B = second half), voxel %.3g m" % (W, H, n, float(vs)),
           "voxels_a": a.count(), "voxels_b": b.count(), "points": int(m), "hits_last_pass": hits, "converged": bool(conv),
           "passes": int(passes), "E_over_hits_last_pass": float(trace[-1, 0] / max(hits, 1)) if passes else None,
           "xi_sq_per_pass": [float(v) for v in trace[:, 35]], "rotation_error_deg": round(ang, 4), "translation_error_mm": round(1e3 * terr, 3),
           "surface_cloud_dev_ms": round(t_cloud * 1e3, 3), "align_call_wall_ms": round(float(np.median(ts)) * 1e3, 3), "reps": args.reps,
           "align_pass_plus_head_event_us": round(batch_ms * 1e3 / 5, 2),
           "k_track_pass_launch_event_us": {"median": round(float(np.median(trk)) * 1e3, 2) if len(trk) else None, "launches": int(len(trk)),
                                            "pixels": W * H},
           "workgroups": int(min(max((m + 255) // 256, 1), 512))}
    a.close(); b.close()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
