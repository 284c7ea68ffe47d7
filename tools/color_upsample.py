#!/usr/bin/env python3
"""ColorUpsampler at BASELINE config C5 (ps_optimizer/ColorUpsampler.cpp, the step main_photo_ba.cpp:300-311 runs after PhotoBA):
150 frames of the 640x480 S-tum stream fused at 1 cm (trunc 10, vis_ on), 50 keyframes, a few PhotoBA iterations from perturbed
key poses, then the colour pass with the pre-BA poses (as the reference does).  Prints one JSON line:
  * the median wall time of gsdf_color_compute and of gsdf_color_cloud (each entry synchronises; the cloud is timed on a fresh
    snapshot, so it includes its predicate / scan / compaction),
  * Hr voxels, observations (voxel x keyframe pairs that counted) and cloud points,
  * the algorithmic bytes: per observation 8 sub-voxels x 4 taps x 12 B; per Hr voxel its 32 B record, its vis_ words and the
    37-float row it writes,
  * the numpy restatement (tests/color_upsampler_ref.py) on the same state, 1 core, as the CPU figure,
  * with --mesh PATH: the coloured sub-voxel mesh of the snapshot (gsdf_color_mesh, ColorUpsampler::extractMesh) written to PATH
    as the reference's PLY, its triangle count and the median wall time of gsdf_color_mesh (sizing call + exact-size call, as
    GradSdf.color_mesh makes them); for scale, in the same process, gsdf_extract_mesh on the same map (it visits every voxel
    record, the Hr sweep only the shell) and, unless --cpu 0, the numpy restatement tests/hr_mesh_ref.py on the same snapshot.
Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/color_upsample.py` run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--keyframes", type=int, default=50)
    ap.add_argument("--ba-it", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", type=int, default=1, help="also time the numpy restatement on the same state (0 = skip)")
    ap.add_argument("--mesh", metavar="PATH", help="also extract the coloured sub-voxel mesh and write it to PATH (PLY)")
    args = ap.parse_args()
    import __graft_entry__ as graft
    import color_upsampler_ref as CU
    pkg = graft.package()
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    vs = np.float32(0.01)
    T = np.float32(10) * vs
    g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    g.enable_vis(n)
    for i in range(n):
        g.update(*seq.frame(i))
    kf = np.linspace(0, n - 1, args.keyframes).astype(np.int32)
    imgs = np.stack([pkg.synth.render_color_bgr(seq, int(i)) for i in kf]).astype(np.float32)
    P = np.stack([pkg.synth.pose16(*seq.pose(int(i))) for i in kf]).astype(np.float32)
    Pp = P.copy()
    Pp[1:, :3, 3] += (0.004 * np.random.default_rng(0).standard_normal((len(kf) - 1, 3))).astype(np.float32)
    g.ba_setup(imgs, Pp, kf)
    g.ba_optimize(args.ba_it)
    nk = len(kf)
    g.color_compute(nk, None, Pp, kf)                                  # warm
    tc, tk = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter(); g.color_compute(nk, None, Pp, kf); tc.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); pts = g.color_cloud(); tk.append(time.perf_counter() - t0)
    nv, obs = g.color_counters()
    vw = (n + 31) // 32
    t_c = float(np.median(tc))
    b = 8 * 4 * 12.0 * obs + (32.0 + 4.0 * vw + 37 * 4.0) * nv
    out = {"config": "C5 ColorUpsampler (after %d PhotoBA iterations)" % args.ba_it, "frame": "%dx%d" % (W, H), "voxel_size_m": float(vs),
           "keyframes": nk, "fused_frames": n, "voxels": g.count(), "hr_voxels": nv, "observations": obs,
           "observations_per_voxel": round(obs / max(nv, 1), 2), "cloud_points": int(len(pts)),
           "compute_ms": round(t_c * 1e3, 3), "cloud_ms": round(float(np.median(tk)) * 1e3, 3),
           "compute_algorithmic_bytes": round(b), "compute_achieved_GBs": round(b / t_c / 1e9, 1),
           "compute_frac_of_hbm_peak": round(b / t_c / 1e9 / HBM_PEAK_GBS, 4),
           "note": "wall times around synchronous C-ABI entries (selection, sort, colour kernel, read-backs); the taps of the 8 "
                   "sub-voxels of a voxel hit neighbouring pixels, so the byte figure is an L2-side rate, not HBM traffic"}
    if args.cpu:
        keys, pay = g.export(sorted=True)
        _, vis = g.export_vis()
        t0 = time.perf_counter()
        sel, rows, _ = CU.compute(keys, pay, vis, imgs, Pp, kf, np.asarray(seq.K, np.float32), vs)
        CU.cloud(keys[sel], rows, vis[sel], kf, vs)
        t_cpu = time.perf_counter() - t0
        out["cpu_restatement"] = {"kind": "numpy float32 restatement, vectorised over voxels", "cores": 1, "wall_s": round(t_cpu, 3),
                                  "speedup": round(t_cpu / t_c, 1)}
    if args.mesh:
        import hr_mesh_ref as HR
        tris, rgb = g.color_mesh()                                       # warm
        tm, tx = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter(); tris, rgb = g.color_mesh(); tm.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); plain = g.extract_mesh(); tx.append(time.perf_counter() - t0)
        with open(args.mesh, "w") as f:
            f.write(HR.ply_text(tris, rgb))
        out["mesh"] = {"path": args.mesh, "triangles": int(len(tris)), "color_mesh_ms": round(float(np.median(tm)) * 1e3, 3),
                       "extract_mesh_ms": round(float(np.median(tx)) * 1e3, 3), "extract_mesh_triangles": int(len(plain)),
                       "note": "wall times of the sizing call plus the exact-size call (two kernel sweeps, one sort, one copy)"}
        if args.cpu:
            keys, rows = g.color_export()
            t0 = time.perf_counter()
            rt, rc = HR.compute(keys, rows, vs)
            t_cpu = time.perf_counter() - t0
            out["mesh"]["cpu_restatement"] = {"kind": "numpy restatement of the layered sweep, vectorised over one z-layer", "cores": 1,
                                              "wall_s": round(t_cpu, 3), "speedup": round(t_cpu / float(np.median(tm)), 1),
                                              "identical": bool(np.array_equal(rt.view(np.uint32), tris.view(np.uint32)) and np.array_equal(rc, rgb))}
    print(json.dumps(out))
    g.close()


if __name__ == "__main__":
    main()
