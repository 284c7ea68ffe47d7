"""The gradient-accuracy analysis on the GPU (gsdf_gradient_angles / gsdf_gradient_stats, GradSdf.gradient_angles /
gradient_stats, the host facade, host/gradient_selftest and Scan3D --gradient-analysis) against the numpy restatement
(tests/gradient_analysis_ref.py) fed with the context's own sorted export.

Per map: keys equal to the export's, the dist column bit-equal to it, identical NaN masks, phi within 1e-4 degrees, counts exactly
equal, mean / median / rmse / p95 within 1e-4 degrees.  The bound is derived, not measured: both sides run the same double
arithmetic on the same floats; the worst conditioning of acos is at cos -> 1, where an error of 1e-15 in the cosine moves the
angle by about 3e-6 degrees; the float32 rounding of phi near 90 degrees is about 4e-6 degrees; every statistic is 1-Lipschitz in
the sup norm of phi."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradient_analysis_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32
pytestmark = pytest.mark.gpu
TOL = 1e-4


def _fixture_map(pkg, name, frames, cap, map_type=None):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    depth = z["depth_u16"].astype(np.float32) * np.float32(z["unit"])
    g = pkg.GradSdf(z["voxel_size"], z["trunc_dist"], int(z["W"]), int(z["H"]), z["K"], capacity_log2=cap, map_type=map_type)
    for i in range(frames):
        g.update(depth[i], z["R"][i], z["t"][i])
    return g, f32(z["voxel_size"]), f32(z["trunc_dist"])


def _threshold_sets(trunc):
    """the script's ladder, n_thr = 1, n_thr = 256 (past trunc_dist: the last ones hold every voxel)"""
    return [G.ladder(trunc), np.array([0.6 * float(trunc)], f32), (np.arange(1, 257) * (1.25 * float(trunc) / 256)).astype(f32)]


def _check(g, spheres, vs, trunc, min_voxels=1):
    """every property of one map; returns (keys, rows)"""
    keys, pay = g.export(sorted=True)
    ref = G.angles(keys, pay, spheres, vs, trunc)
    k2, rows = g.gradient_angles(spheres)
    assert k2.dtype == np.int32 and rows.dtype == np.float32 and len(keys) >= min_voxels
    assert k2.shape == keys.shape and np.array_equal(k2, keys)
    assert rows.shape == ref.shape and np.array_equal(rows[:, 0].view(np.uint32), pay[:, 0].view(np.uint32))
    nan = np.isnan(rows[:, 1:])
    assert np.array_equal(nan, np.isnan(ref[:, 1:]))
    dphi = float(np.nanmax(np.abs(rows[:, 1:].astype(np.float64) - ref[:, 1:].astype(np.float64)))) if (~nan).any() else 0.0
    print("voxels %d, undefined per estimator %s, phi |d|max %.2e deg" % (len(keys), nan.sum(0).tolist(), dphi))
    assert dphi <= TOL
    assert (rows[:, 1:][~nan] >= 0).all() and (rows[:, 1:][~nan] <= 90).all()
    for thr in _threshold_sets(trunc):
        st, want = g.gradient_stats(spheres, thr), G.stats(ref, thr)
        assert st.shape == want.shape == (4, len(thr), 5) and st.dtype == np.float64
        assert np.array_equal(st[:, :, 0], want[:, :, 0])
        assert np.array_equal(np.isnan(st), np.isnan(want))
        dst = float(np.nanmax(np.abs(st[:, :, 1:] - want[:, :, 1:]))) if (want[:, :, 0] > 0).any() else 0.0
        print("  n_thr %d: largest count %d, statistics |d|max %.2e deg" % (len(thr), int(want[:, :, 0].max()), dst))
        assert dst <= TOL
        own = G.stats(rows, thr)                                               # the device's statistics of the device's own angles
        assert np.array_equal(own[:, :, 0], st[:, :, 0]) and np.allclose(own[:, :, [2, 4]], st[:, :, [2, 4]], rtol=0, atol=1e-9, equal_nan=True)
    k3, p3 = g.export(sorted=True)                                             # the map is untouched
    assert k3.tobytes() == keys.tobytes() and p3.tobytes() == pay.tobytes()
    return keys, rows


def test_gpu_gradient_spheres_64x48(pkg):
    g, vs, trunc = _fixture_map(pkg, "spheres_64x48", 2, 14)
    keys, rows = _check(g, pkg.synth.make_spheres(7), vs, trunc)
    assert len(keys) == 96 and (keys.max(0) - keys.min(0) + 1).tolist() == [22, 34, 9]
    g.close()


def test_gpu_gradient_spheres_160x120(pkg):
    g, vs, trunc = _fixture_map(pkg, "spheres_160x120", 2, 16)
    sph = pkg.synth.make_spheres(7)
    keys, rows = _check(g, sph, vs, trunc, min_voxels=8000)
    assert len(keys) == 8324
    st = g.gradient_stats(sph, [0.011, 0.1])
    print("medians at d = 0.011:", st[:, 0, 2].round(2), "at d = 0.1:", st[:, 1, 2].round(2))
    assert (st[0, :, 2] < st[1:, :, 2].min(0)).all()                           # the paper's picture, from the device
    g.close()


@pytest.fixture(scope="module")
def tum(pkg):
    g, vs, trunc = _fixture_map(pkg, "tum_128x96", 3, 16)
    yield g, vs, trunc
    g.close()


def test_gpu_gradient_tum_three_frames(pkg, tum):
    g, vs, trunc = tum
    sph = np.array([[0.2, -0.1, 1.4, 0.5], [-0.6, 0.3, 2.0, 0.25], [0.0, 0.0, 0.0, 0.1]], f32)      # any list serves as ground truth
    _check(g, sph, vs, trunc, min_voxels=20000)


def test_gpu_gradient_analytic_sphere_through_merge_raw(pkg):
    """negative keys and block floor semantics: a neighbour looked up in the wrong block shows as a central angle of degrees"""
    vs, trunc = f32(0.02), f32(0.1)
    keys, pay, sphere = G.sphere_map(12.5, (0.3, -0.2, 0.1), vs, trunc, band_vox=4.0)
    g = pkg.GradSdf(vs, trunc, 64, 48, pkg.synth.intrinsics(64, 48), capacity_log2=17)
    g.merge_raw(keys, pay.copy())                                              # w = 1: the raw sums are the values
    k2, rows = _check(g, sphere, vs, trunc, min_voxels=10000)
    assert (k2.min(0) < 0).all() and (k2.max(0) > 0).all()
    have = {tuple(k) for k in k2.tolist()}
    inner = np.array([all(tuple(np.add(k, o)) in have for o in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
                      for k in k2.tolist()])
    print("sphere: stored max %.2e deg, central max over %d inner voxels %.4f deg" % (np.nanmax(rows[:, 1]), inner.sum(), rows[inner, 2].max()))
    assert np.nanmax(rows[:, 1]) < 1e-3 and rows[inner, 2].max() < 0.1 * (25.0 / 12.5) ** 2      # second order in h / R
    g.close()


def test_gpu_gradient_one_voxel_and_hand_made_maps(pkg):
    vs, trunc = f32(0.02), f32(0.1)
    K = pkg.synth.intrinsics(64, 48)
    raw = np.array([[0.01, 0, 0, 2, 1]], f32)
    g = pkg.GradSdf(vs, trunc, 64, 48, K, capacity_log2=14)
    g.merge_raw(np.array([[3, -2, 5]], np.int32), raw)
    sph = np.array([[0.06, -0.04, -1.0, 1.0]], f32)
    keys, rows = _check(g, sph, vs, trunc)
    assert len(rows) == 1 and rows[0, 1] < 1e-5 and np.isnan(rows[0, 2:]).all()
    st = g.gradient_stats(sph, [0.02])
    assert st[:, 0, 0].tolist() == [1, 0, 0, 0] and np.isnan(st[1:, 0, 1:]).all()
    g.close()
    # a plate with a hole across block boundaries; zero, NaN and infinite gradient sums; a voxel centre ON the sphere centre
    ks = np.array([[x, y, 0] for y in range(-2, 3) for x in range(2, 7) if (x, y) != (4, 0)], np.int32)
    raw = np.zeros((len(ks), 5), f32)
    raw[:, 0] = 0.01 * ks[:, 0] - 0.005 * ks[:, 1]
    raw[:, 1:4] = (1, 0.5, 0)
    raw[0, 1:4] = 0
    raw[1, 1] = np.nan
    raw[2, 2] = np.inf
    raw[:, 4] = 1
    g = pkg.GradSdf(vs, trunc, 64, 48, K, capacity_log2=14)
    g.merge_raw(ks, raw)
    sph = np.array([[float(vs * f32(5)), float(vs * f32(1)), 0.0, 0.3]], f32)
    keys, rows = _check(g, sph, vs, trunc)
    on_centre = (keys == [5, 1, 0]).all(1)
    assert on_centre.sum() == 1 and np.isnan(rows[on_centre, 1:]).all() and np.isnan(rows[:, 1]).sum() == 4
    g.close()


def test_gpu_gradient_base_sdf_context(pkg):
    g, vs, trunc = _fixture_map(pkg, "spheres_160x120", 2, 16, map_type=pkg.MAP_BASE)
    assert g.map_type == pkg.MAP_BASE
    keys, rows = _check(g, pkg.synth.make_spheres(7), vs, trunc, min_voxels=8000)
    assert np.isfinite(rows[:, 1]).mean() > 0.99                               # a base context stores the gradient sums too
    g.close()


def _angles_raw(g, sph, n_spheres, keys, rows, max_n, n_ptr=True):
    n = C.c_int64(-5)
    rc = g.L.gsdf_gradient_angles(g.h, None if sph is None else sph.ctypes.data_as(C.POINTER(C.c_float)), n_spheres,
                                  None if keys is None else keys.ctypes.data_as(C.POINTER(C.c_int32)),
                                  None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_float)), max_n, C.byref(n) if n_ptr else None)
    return rc, n.value


def _stats_raw(g, sph, n_spheres, thr, n_thr, out):
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))           # noqa: E731
    return g.L.gsdf_gradient_stats(g.h, fp(sph), n_spheres, fp(thr), n_thr, None if out is None else out.ctypes.data_as(C.POINTER(C.c_double)))


def test_gpu_gradient_protocol_and_determinism(pkg, tum):
    g, vs, trunc = tum
    INVALID = pkg.binding.ERR_INVALID
    sph = np.array([[0.2, -0.1, 1.4, 0.5], [-0.6, 0.3, 2.0, 0.25]], f32)
    thr = G.ladder(trunc)
    before = g.export(sorted=True)
    k0, r0 = g.gradient_angles(sph)
    s0 = g.gradient_stats(sph, thr)
    nv = len(k0)
    assert _angles_raw(g, sph, 2, None, None, 0) == (0, nv)                    # the sizing call
    keys = np.full((nv, 3), -7, np.int32)
    rows = np.full((nv, 5), 7.5, np.float32)
    rc, need = _angles_raw(g, sph, 2, keys, rows, nv - 1)                      # one too small: nothing written, the need reported
    assert rc == INVALID and need == nv and "too small" in g.L.gsdf_last_error().decode()
    assert (keys == -7).all() and (rows == 7.5).all()
    out = np.full((4, len(thr), 5), 7.5)
    bad_sph = [sph * [1, 1, 1, -1], sph * [1, 1, 1, 0], np.where(np.arange(8).reshape(2, 4) == 5, np.nan, sph).astype(f32),
               np.where(np.arange(8).reshape(2, 4) == 2, np.inf, sph).astype(f32)]
    for s, ns in [(sph, 0), (np.tile(sph, (33, 1))[:65].copy(), 65), (sph, -1), (None, 2)] + [(np.ascontiguousarray(b, f32), 2) for b in bad_sph]:
        assert _angles_raw(g, s, ns, keys, rows, nv) == (INVALID, -5)
        assert _stats_raw(g, s, ns, thr, len(thr), out) == INVALID
    assert _angles_raw(g, sph, 2, keys, rows, nv, n_ptr=False)[0] == INVALID
    assert _angles_raw(g, sph, 2, None, None, nv)[0] == INVALID                # room announced, no buffer
    assert _angles_raw(g, sph, 2, keys, rows, -1)[0] == INVALID
    up = np.arange(1, 258, dtype=f32) * f32(0.001)
    bad_thr = [(thr, 0), (up, 257), (None, 3), (np.array([0.01, 0.01], f32), 2), (np.array([0.02, 0.01], f32), 2), (np.array([0.0, 0.01], f32), 2),
               (np.array([-0.01, 0.01], f32), 2), (np.array([0.01, np.nan], f32), 2), (np.array([0.01, np.inf], f32), 2)]
    for t, nt in bad_thr:
        assert _stats_raw(g, sph, 2, t, nt, out) == INVALID
    assert _stats_raw(g, sph, 2, thr, len(thr), None) == INVALID
    assert (keys == -7).all() and (rows == 7.5).all() and (out == 7.5).all()   # every refusal left the buffers alone
    assert _stats_raw(g, np.tile(sph, (32, 1)).copy(), 64, up[:256].copy(), 256, np.empty((4, 256, 5))) == 0      # the limits themselves
    # keys only / rows only
    assert _angles_raw(g, sph, 2, keys, None, nv) == (0, nv) and keys.tobytes() == k0.tobytes() and (rows == 7.5).all()
    assert _angles_raw(g, sph, 2, None, rows, nv + 3) == (0, nv) and rows.tobytes() == r0.tobytes()
    # a second call, and the map moved into a larger table: the same bytes
    k1, r1 = g.gradient_angles(sph)
    s1 = g.gradient_stats(sph, thr)
    cap = g.capacity_log2()
    g.grow(cap + 1)
    assert g.capacity_log2() == cap + 1
    k2, r2 = g.gradient_angles(sph)
    s2 = g.gradient_stats(sph, thr)
    assert k0.tobytes() == k1.tobytes() == k2.tobytes() and r0.tobytes() == r1.tobytes() == r2.tobytes()
    assert s0.tobytes() == s1.tobytes() == s2.tobytes()
    after = g.export(sorted=True)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    # an empty map
    e = pkg.GradSdf(vs, trunc, 64, 48, pkg.synth.intrinsics(64, 48), capacity_log2=14)
    assert _angles_raw(e, sph, 2, None, None, 0) == (0, 0)
    assert _angles_raw(e, sph, 2, keys, rows, nv) == (0, 0) and rows.tobytes() == r0.tobytes()
    ke, re_ = e.gradient_angles(sph)
    assert ke.shape == (0, 3) and re_.shape == (0, 5)
    se = e.gradient_stats(sph, thr)
    assert (se[:, :, 0] == 0).all() and np.isnan(se[:, :, 1:]).all()
    e.close()


def test_gpu_gradient_sees_the_pending_fusion(pkg):
    """gsdf_update_dev leaves its fusion waiting for the next frame; a map-reading entry launches it first"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "spheres_160x120.npz"))
    depth = z["depth_u16"].astype(np.float32) * np.float32(z["unit"])
    sph = pkg.synth.make_spheres(7)
    thr = G.ladder(z["trunc_dist"])
    mk = lambda: pkg.GradSdf(z["voxel_size"], z["trunc_dist"], int(z["W"]), int(z["H"]), z["K"], capacity_log2=16)      # noqa: E731
    a, b, c = mk(), mk(), mk()
    for i in range(2):
        a.update(depth[i], z["R"][i], z["t"][i])
    ka, ra = a.gradient_angles(sph)
    sa = a.gradient_stats(sph, thr)
    b.update_dev(b.upload(depth[0]), z["R"][0], z["t"][0])
    kb0, rb0 = b.gradient_angles(sph)                                          # between two frames
    b.update_dev(b.upload(depth[1]), z["R"][1], z["t"][1])
    kb, rb = b.gradient_angles(sph)
    for i in range(2):
        c.update_dev(c.upload(depth[i]), z["R"][i], z["t"][i])
    sc = c.gradient_stats(sph, thr)                                            # the statistics entry flushes as well
    assert 0 < len(kb0) < len(ka)
    assert kb.tobytes() == ka.tobytes() and rb.tobytes() == ra.tobytes() and sc.tobytes() == sa.tobytes()
    for g in (a, b, c):
        g.close()


def _parse_table(path):
    blocks, names = [], []
    for line in open(path):
        if line.startswith("# estimator"):
            blocks.append([])
            names.append(line.split()[3])
        elif not line.startswith("#") and line.strip():
            blocks[-1].append([float(v) for v in line.split()])
    return np.array(blocks), names


@pytest.mark.parametrize("kind", ["grad", "base"])
def test_gradient_selftest_binary(pkg, tmp_path, kind):
    """host/gradient_selftest: MapGradPixelSdf / MapPixelSdf::gradient_analysis through the C++ facade; its table, its statistics
    and its per-voxel rows against the restatement of the map it dumps"""
    W, H, n, vs = 160, 120, 3, f32(0.02)
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=4, step_deg=2.0)
    d = tmp_path
    np.asarray(seq.K, np.float32).reshape(9).tofile(d / "K.bin")
    np.stack([seq.frame(i)[0] for i in range(n)]).astype(np.float32).tofile(d / "depth.bin")
    np.stack([pkg.synth.pose16(*seq.pose(i)) for i in range(n)]).astype(np.float32).tofile(d / "poses.bin")
    sph = np.asarray(seq.spheres, f32).reshape(-1, 4)
    sph.tofile(d / "spheres.bin")
    out = subprocess.run([os.path.join(HOST, "gradient_selftest"), str(d), str(W), str(H), str(n), repr(float(vs)), "5"]
                         + (["base"] if kind == "base" else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "gradient_selftest: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    keys = np.fromfile(d / "map_keys.bin", np.int32).reshape(-1, 3)
    pay = np.fromfile(d / "map_payload.bin", np.float32).reshape(-1, 5)
    thr = np.fromfile(d / "thresholds.bin", np.float32)
    trunc = f32(5) * vs
    assert len(keys) > 3000 and np.array_equal(thr, G.ladder(trunc)) and len(thr) == 100
    ref = G.angles(keys, pay, sph, vs, trunc)
    rows = np.fromfile(d / "angle_rows.bin", np.float32).reshape(-1, 5)
    assert np.array_equal(np.fromfile(d / "angle_keys.bin", np.int32).reshape(-1, 3), keys)
    assert np.array_equal(np.isnan(rows), np.isnan(ref)) and np.nanmax(np.abs(rows.astype(np.float64) - ref)) <= TOL
    st = np.fromfile(d / "stats.bin", np.float64).reshape(4, len(thr), 5)
    want = G.stats(ref, thr)
    assert np.array_equal(st[:, :, 0], want[:, :, 0]) and np.nanmax(np.abs(st - want)) <= TOL
    table, names = _parse_table(str(d / "gradient_stats.txt"))
    assert names == list(G.ESTIMATORS) and table.shape == (4, len(thr), 6)
    assert np.array_equal(table[:, :, 0].astype(f32), np.tile(thr, (4, 1)))
    assert np.array_equal(table[:, :, 1:], st, equal_nan=True)                 # %.17g: the table parses back to the statistics


def test_scan3d_gradient_analysis_flag(pkg, O, tmp_path):
    """Scan3D --gradient-analysis: one more file, the others byte for byte as without the flag; the table parses back to
    gradient_stats of a context fused from the same files' content the CLI's way; a ladder of more than 256 thresholds is reported
    and skipped, the other exports still written"""
    W, H, n = 160, 120, 3
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=4, step_deg=2.0)
    ds = pkg.synth.write_dataset(seq, str(tmp_path / "ds"), layout="synth")
    sph = np.asarray(seq.spheres, f32).reshape(-1, 4)
    sfile = str(tmp_path / "spheres.txt")
    np.savetxt(sfile, sph, fmt="%.9g")
    res = {}
    for tag, extra, trunc in (("plain", [], "5"), ("flag", ["--gradient-analysis", sfile], "5"), ("wide", ["--gradient-analysis", sfile], "13")):
        r = str(tmp_path / tag) + "/"
        os.makedirs(r)
        cmd = [os.path.join(HOST, "Scan3D"), "--input", ds, "--results", r, "--scan-type", "grad-sdf", "--data-type", "synth",
               "--voxel-size", "0.02", "--trunc", trunc, "--width", str(W), "--height", str(H), "--hash-capacity", "18", "--sync"]
        out = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert ("Save gradient statistics to disk" in out.stdout) == bool(extra)
        res[tag] = (r, out)
    plain, flag, wide = (sorted(os.listdir(res[t][0])) for t in ("plain", "flag", "wide"))
    assert flag == sorted(plain + ["gradient_sdf_gradient_stats.txt"]) and "gradient_sdf_mesh_final.ply" in plain
    for f in plain:
        assert open(res["plain"][0] + f, "rb").read() == open(res["flag"][0] + f, "rb").read(), f
    assert wide == plain and "does not fit the library's limit of 256 thresholds" in res["wide"][1].stderr      # 0.26 m: 260 thresholds
    table, names = _parse_table(res["flag"][0] + "gradient_sdf_gradient_stats.txt")
    vs = f32(0.02)
    g = pkg.GradSdf(vs, f32(5) * vs, W, H, seq.K, capacity_log2=18)
    poses = np.loadtxt(ds + "pose.txt")
    for i in range(n):
        d = seq.depth_u16(i).astype(np.float32) * np.float32(0.001)
        R = O.quat_to_R(O.R_to_quat(O.quat_to_R(poses[i, 4:8].astype(np.float32))))
        g.update(d, R, poses[i, 1:4].astype(np.float32))
    thr = G.ladder(f32(5) * vs)
    st = g.gradient_stats(np.loadtxt(sfile).astype(f32), thr)
    g.close()
    print("Scan3D: medians at d = 0.1:", table[:, -1, 3].round(2))
    assert names == list(G.ESTIMATORS) and table.shape == (4, 100, 6) and np.array_equal(table[:, :, 0].astype(f32), np.tile(thr, (4, 1)))
    assert np.array_equal(table[:, :, 1:], st, equal_nan=True) and st[0, -1, 0] > 3000
