#!/usr/bin/env python3
"""The gradient-accuracy analysis (gsdf_gradient_angles / gsdf_gradient_stats; matlab/GradientAnalysisSpheres.m) on the C1
stream, measured: synth.Sequence("spheres", 640, 480, n_frames=30, seed=0) fused at its ground-truth poses (1 cm voxels,
trunc 10), the ladder d = 0.001 : 0.001 : trunc.

Prints the table (median and 95th percentile per estimator at a few d) and writes profiles/gradient_analysis.json: the four
estimators' curves, voxel and block counts, the wall time of both calls (median of `--reps` synchronous calls) with the HIP-event
time of the same calls (gsdf_timer_*), and the numpy restatement's time (tests/gradient_analysis_ref.py) on the same export.
Per-kernel times come from a kernel trace of this command:

    rocprofv3 --kernel-trace --output-format csv -d DIR -o ga -- python tools/gradient_analysis.py --no-json
    python tools/gradient_analysis.py --kernel-trace DIR

(the second run reads DIR/**/*kernel_trace.csv and adds the median duration of every kernel of the two calls).  The times are
reported, not gated; the JSON says which box they come from."""
import argparse, collections, csv, glob, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def med_event(g, f, reps):
    ts = []
    for _ in range(reps):
        g.timer_start(); f(); ts.append(g.timer_stop_ms())
    return float(np.median(ts))


def kernel_medians(root):
    files = glob.glob(root + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no kernel_trace.csv under " + root)
    d = collections.defaultdict(list)
    for r in csv.DictReader(open(files[0])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "")
        if "k_grad" in name or "radix" in name.lower() or "k_iota" in name or "k_export" in name:
            d[name[:64]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"launches": len(v), "median_us": round(float(np.median(v)), 2)} for k, v in sorted(d.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-json", action="store_true", help="print only (the run under the profiler)")
    ap.add_argument("--kernel-trace", default=None, help="directory of a rocprofv3 --kernel-trace run of this command")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gradient_analysis.json"))
    args = ap.parse_args()
    import __graft_entry__ as graft
    import gradient_analysis_ref as G
    pkg = graft.package()
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=0)
    vs = np.float32(0.01); T = np.float32(10) * vs
    g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    for i in range(n):
        g.update(*seq.frame(i))
    sph = np.asarray(seq.spheres, np.float32).reshape(-1, 4)
    thr = G.ladder(T)
    keys, pay = g.export(sorted=True)
    blocks = len(np.unique((keys >> 2), axis=0))
    st = g.gradient_stats(sph, thr)                                            # warm
    g.gradient_angles(sph)
    t_stats, t_angles = med(lambda: g.gradient_stats(sph, thr), args.reps), med(lambda: g.gradient_angles(sph), args.reps)
    e_stats, e_angles = med_event(g, lambda: g.gradient_stats(sph, thr), args.reps), med_event(g, lambda: g.gradient_angles(sph), args.reps)
    t0 = time.perf_counter(); ref_rows = G.angles(keys, pay, sph, vs, T); t_ref_a = time.perf_counter() - t0
    t0 = time.perf_counter(); ref = G.stats(ref_rows, thr); t_ref_s = time.perf_counter() - t0
    dev = float(np.nanmax(np.abs(st[:, :, 1:] - ref[:, :, 1:])))
    print("voxels %d blocks %d thresholds %d; device against restatement: counts equal %s, statistics |d|max %.2e deg"
          % (len(keys), blocks, len(thr), np.array_equal(st[:, :, 0], ref[:, :, 0]), dev))
    print("%-9s %8s | %s" % ("estimator", "d [m]", "count   mean  median   rmse    p95  [deg]"))
    for e, name in enumerate(G.ESTIMATORS):
        for k in (4, 9, 19, 49, len(thr) - 1):
            if k < len(thr):
                print("%-9s %8.3f | %6d %6.2f %7.2f %6.2f %6.2f" % ((name, thr[k], int(st[e, k, 0])) + tuple(st[e, k, 1:])))
    print("gsdf_gradient_stats %.3f ms wall (%.3f ms on the stream), gsdf_gradient_angles %.3f ms (%.3f); numpy restatement %.1f + %.1f ms"
          % (t_stats * 1e3, e_stats, t_angles * 1e3, e_angles, t_ref_a * 1e3, t_ref_s * 1e3))
    out = {"workload": "C1 stream: synth.Sequence('spheres', 640, 480, n_frames=%d, seed=0), GT poses, 1 cm voxels, trunc 10" % n,
           "measured_on": "the builder's MI355X box; reported, not gated", "voxels": int(len(keys)), "blocks": int(blocks),
           "thresholds": [float(t) for t in thr], "stat_columns": list(G.STAT_NAMES),
           "curves": {name: [[None if np.isnan(v) else float(v) for v in row] for row in st[e]] for e, name in enumerate(G.ESTIMATORS)},
           "device_vs_restatement": {"counts_equal": bool(np.array_equal(st[:, :, 0], ref[:, :, 0])), "statistics_max_abs_deg": dev},
           "wall_ms": {"gsdf_gradient_stats": round(t_stats * 1e3, 3), "gsdf_gradient_angles": round(t_angles * 1e3, 3), "reps": args.reps,
                       "note": "median of synchronous calls through the Python binding: allocation, kernels, sorts, download"},
           "stream_ms": {"gsdf_gradient_stats": round(e_stats, 3), "gsdf_gradient_angles": round(e_angles, 3),
                         "note": "HIP events around the same calls (gsdf_timer_start / gsdf_timer_stop_ms)"},
           "numpy_restatement_ms": {"angles": round(t_ref_a * 1e3, 1), "stats": round(t_ref_s * 1e3, 1), "note": "one core, same export"}}
    if args.kernel_trace:
        out["kernel_median_us"] = kernel_medians(args.kernel_trace)
        for k, v in out["kernel_median_us"].items():
            print("  %-64s %5d launches, median %8.2f us" % (k, v["launches"], v["median_us"]))
    if not args.no_json:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", args.out)
    g.close()


if __name__ == "__main__":
    main()
