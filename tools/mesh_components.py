#!/usr/bin/env python3
"""Connected components of the indexed mesh, and the filtered mesh, on the C5 map -- measured, not gated.

Fuses the 640x480 S-tum stream of BASELINE config C5 at its ground-truth poses (1 cm voxels, trunc 10) and times, as wall clock
around the synchronous entries (median of `--reps` after one warm call, sizing call included as a caller pays it):
  * gsdf_extract_mesh_indexed (GradSdf.extract_mesh_indexed), the mesh both new entries start from,
  * gsdf_mesh_components (GradSdf.mesh_components),
  * gsdf_extract_mesh_indexed_filtered at min_faces = 10 and at MESH_KEEP_LARGEST,
  * the numpy restatement (tests/mesh_components_ref.py) of the components and of the filter on the same arrays, 1 core,
and checks the device's labels, counts and filtered arrays against the restatement bit for bit.  One JSON line, also written to
profiles/mesh_components.json (or --out)."""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_components.json"))
    args = ap.parse_args()
    import __graft_entry__ as graft
    import mesh_components_ref as MC
    pkg = graft.package()
    W, H, n = 640, 480, args.frames
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    vs = np.float32(0.01); T = np.float32(10) * vs
    g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=22)
    for i in range(n):
        g.update(*seq.frame(i))
    V, N, F = g.extract_mesh_indexed()
    vc, fc, counts, bbox = g.mesh_components()
    t0 = time.perf_counter(); ref = MC.compute(V, F); t_ref = time.perf_counter() - t0
    same = lambda a, b: a.shape == b.shape and a.tobytes() == b.tobytes()    # noqa: E731
    ok = same(vc, ref["vertex_comp"]) and same(fc, ref["face_comp"]) and same(counts, ref["counts"]) and np.array_equal(bbox, ref["bbox"])
    out = {"map": "C5 (BASELINE.json configs[4]): S-tum %dx%d, %d frames, voxel %.3g m" % (W, H, n, float(vs)), "voxels": g.count(),
           "vertices": int(len(V)), "faces": int(len(F)), "components": int(len(counts)),
           "largest_face_counts": [int(c) for c in np.sort(counts[:, 0])[::-1][:8]], "components_under_10_faces": int((counts[:, 0] < 10).sum()),
           "union_passes": 1, "restatement_rounds": int(ref["rounds"]), "reps": args.reps,
           "extract_mesh_indexed_ms": round(med(g.extract_mesh_indexed, args.reps) * 1e3, 3),
           "mesh_components_ms": round(med(g.mesh_components, args.reps) * 1e3, 3),
           "numpy_components_ms": round(t_ref * 1e3, 1), "filtered": {}}
    for name, m in (("min_faces_10", 10), ("keep_largest", pkg.MESH_KEEP_LARGEST)):
        Vg, Ng, Fg, nc, kept = g.extract_mesh_indexed_filtered(m)
        t0 = time.perf_counter(); Vr, Nr, Fr, Cr, kr = MC.filter_mesh(V, N, F, m, ref); t_f = time.perf_counter() - t0
        ok = ok and same(Vg, Vr) and same(Ng, Nr) and same(Fg, Fr) and (nc, kept) == (Cr, kr)
        out["filtered"][name] = {"kept_components": int(kept), "faces": int(len(Fg)), "vertices": int(len(Vg)),
                                 "ms": round(med(lambda: g.extract_mesh_indexed_filtered(m), args.reps) * 1e3, 3),
                                 "numpy_filter_ms": round(t_f * 1e3, 1)}
    out["equals_restatement"] = bool(ok)
    g.close()
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
