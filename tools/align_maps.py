#!/usr/bin/env python3
"""Map-to-map registration at bench scale -- measured, not gated.

Fuses the two halves of the 640x480 S-tum stream (1 cm voxels, trunc 10) into two maps A and B at their ground-truth poses, takes
B's surface cloud on the device (gsdf_surface_cloud_dev), moves it into a source frame by 1 degree about (0.3, -0.5, 0.8) and
(0.01, -0.008, 0.006) m, and registers it against A from the identity (gsdf_align_points_dev).  Reports points, hits, passes, the
final E / hits, the recovered pose's error, the wall time of the call (median of `--reps` after one warm call), and the HIP-event
time of one batch of 5 pass + head pairs divided by 5 (conv_threshold = 0, so all five run) next to the event time of
k_track_pass's launches on map A for a frame of the stream.  One JSON line, also written to profiles/align_points.json (or --out)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_points.json"))
    args = ap.parse_args()
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
