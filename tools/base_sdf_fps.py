"""Frames per second of the plain-SDF baseline (MapPixelSdf, --scan-type base-sdf) next to the Gradient-SDF map, in one process,
on bench.py's tracked workload: the S-tum stream at 640x480, 1 cm voxels, trunc 10, 2^22 records; frame 0 fused at its GT pose,
frames 1..5 untimed, frames 6..25 timed (gsdf_track_and_fuse_ahead_dev with the next-frame hint), median of 5 windows.  Then a
replay of the timed frames with HIP events around every tracker launch (gsdf_profile): the per-launch median of the base
k_track_pass, passes per frame, and the algorithmic bytes of a base pass -- 4 B of depth per pixel, and per pixel with a hit its
8 corner records' (w, s) = 64 B -- over the median launch, as a fraction of the HBM peak.
Prints one JSON line.  usage: python tools/base_sdf_fps.py [--repeats 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G  # noqa: E402

HBM_PEAK_GBS = 8000.0       # MI355X HBM3E spec peak
W, H, WM, K = 640, 480, 5, 20


def windows(g, dev, p0, R0, t0, repeats):
    def start():
        g.reset()
        g.update_dev(dev[0], R0, t0)
        g.set_pose(p0)
        for i in range(1, 1 + WM):
            g.track_and_fuse_ahead_dev(dev[i], dev[i + 1])
    runs = []
    for rep in range(1 + repeats):
        start()
        g.sync()
        t = time.perf_counter()
        for i in range(1 + WM, 1 + WM + K):
            g.track_and_fuse_ahead_dev(dev[i], dev[i + 1] if i < WM + K else None)
        g.sync()
        if rep:
            runs.append(time.perf_counter() - t)
    return float(np.median(runs))


def replay(g, dev, p0, R0, t0):
    """the timed frames again, every tracker launch timed by itself"""
    g.reset()
    g.update_dev(dev[0], R0, t0)
    g.set_pose(p0)
    for i in range(1, 1 + WM):
        g.track_and_fuse_dev(dev[i])
    g.sync()
    st0 = g.stats()
    g.profile(1)
    for i in range(1 + WM, 1 + WM + K):
        g.track_and_fuse_dev(dev[i])
    g.sync()
    each = g.profile_launches(2)
    g.profile(0)
    st1 = g.stats()
    log = g.frame_log()[WM:WM + K]
    passes = float(log[:, 8].sum())
    return {"launch_median_us": round(float(np.median(each)) * 1e3, 2), "launches": int(each.size),
            "passes_per_frame": round(passes / K, 2), "hits_per_pass": (st1["n_hit"] - st0["n_hit"]) / max(passes, 1.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    pkg = G.package()
    seq = pkg.synth.Sequence("tum", W, H, seed=0)
    frames = [seq.frame(i) for i in range(2 + WM + K)]
    vs = np.float32(0.01)
    T = np.float32(10) * vs
    out = {"workload": "S-tum 640x480, 1 cm, trunc 10, frames %d..%d, median of %d windows" % (1 + WM, WM + K, a.repeats)}
    for name, mt in (("grad", pkg.MAP_GRAD), ("base", pkg.MAP_BASE)):
        g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22, map_type=mt)
        dev = [g.upload(f[0]) for f in frames]
        d0, R0, t0 = frames[0]
        q = G.oracle_module().R_to_quat(R0)
        p0 = np.concatenate([t0, q]).astype(np.float32)
        R0q = G.oracle_module().quat_to_R(q)
        s = windows(g, dev, p0, R0q, t0, a.repeats)
        r = replay(g, dev, p0, R0q, t0)
        out[name + "_fps"] = round(K / s, 1)
        out[name + "_track_launch_median_us"] = r["launch_median_us"]
        out[name + "_passes_per_frame"] = r["passes_per_frame"]
        if name == "base":
            alg = 4.0 * W * H + 64.0 * r["hits_per_pass"]
            gbs = alg / (r["launch_median_us"] * 1e-6) / 1e9 if r["launch_median_us"] > 0 else 0.0
            out["base_pass_alg_bytes"] = int(alg)
            out["base_pass_hbm_frac"] = round(gbs / HBM_PEAK_GBS, 4)
        g.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
