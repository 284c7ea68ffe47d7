"""The plain-SDF baseline on the GPU (MapPixelSdf: gsdf_set_map_type(GSDF_MAP_BASE), --scan-type base-sdf): shared fusion,
the trilinear query bit for bit against the numpy restatement (tests/base_sdf_ref.py), the tracker pass by pass, the frame
loop entries, the contract of the map type, and Scan3D end to end."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import base_sdf_ref as B  # noqa: E402
from conftest import pose7_from  # noqa: E402
from lockstep import TOL  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32


def _quat_to_R_f32(q):
    """Eigen's toRotationMatrix in float32 as the library's gsdf_quat_to_R (csrc/gsdf_math.h)"""
    x, y, z, w = (f32(v) for v in q)
    tx, ty, tz = f32(2) * x, f32(2) * y, f32(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[f32(1) - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, f32(1) - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, f32(1) - (txx + tyy)]], f32)


def _tum640():
    g = np.load(os.path.join(ROOT, "tests", "golden", "tum_640x480.npz"))
    depth = g["depth_u16"].astype(f32) * g["unit"]
    return g, depth


def _pair(pkg, vs, T, W, H, K, cap=20):
    gg = pkg.GradSdf(vs, T, W, H, K, capacity_log2=cap)
    gb = pkg.GradSdf(vs, T, W, H, K, capacity_log2=cap, map_type=pkg.MAP_BASE)
    assert gg.map_type == pkg.MAP_GRAD and gb.map_type == pkg.MAP_BASE
    return gg, gb


def _same_map(a, b):
    ka, pa = a.export(sorted=True)
    kb, pb = b.export(sorted=True)
    assert np.array_equal(ka, kb)
    assert np.array_equal(pa[:, 0], pb[:, 0]) and np.array_equal(pa[:, 4], pb[:, 4])
    return ka, pa


# ---- 1. fusion is shared --------------------------------------------------------------------------------------------------
def test_fusion_is_shared_tum640(pkg):
    g, depth = _tum640()
    W, H = int(g["W"]), int(g["H"])
    gg, gb = _pair(pkg, g["voxel_size"], g["trunc_dist"], W, H, g["K"], cap=21)
    for i in range(depth.shape[0]):
        for m in (gg, gb):
            m.update(depth[i], g["R"][i], g["t"][i])
    k, _ = _same_map(gg, gb)
    assert len(k) > 10000
    gg.close(); gb.close()


def test_fusion_is_shared_synth32(pkg):
    W, H = 320, 240
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=32, seed=2, step_deg=1.0)
    vs = f32(0.02)
    gg, gb = _pair(pkg, vs, f32(5) * vs, W, H, seq.K)
    for i in range(32):
        d, R, t = seq.frame(i)
        gg.update(d, R, t)
        gb.update(d, R, t)
    _same_map(gg, gb)
    gg.close(); gb.close()


# ---- 2. query is bit-exact --------------------------------------------------------------------------------------------------
def test_query_bit_exact_against_restatement(pkg):
    g, depth = _tum640()
    W, H = int(g["W"]), int(g["H"])
    vs, T = g["voxel_size"], g["trunc_dist"]
    gb = pkg.GradSdf(vs, T, W, H, g["K"], capacity_log2=21, map_type=pkg.MAP_BASE)
    gb.update(depth[0], g["R"][0], g["t"][0])
    keys, pay = gb.export(sorted=True)
    m = B.BaseMap.from_export(keys, pay, vs, T)
    rng = np.random.default_rng(7)
    c = keys.astype(f32) * vs
    sel = rng.integers(0, len(keys), 600_000)
    band = (c[sel] + rng.uniform(-1.5, 1.5, (len(sel), 3)).astype(f32) * vs).astype(f32)   # around voxels: 0..8 corners present
    # cubes straddling 2 / 4 / 8 blocks: floor index 3 mod 4 on 1..3 axes
    kk = keys[rng.integers(0, len(keys), 200_000)].copy()
    for a in range(3):
        kk[rng.random(len(kk)) < 0.5, a] |= 3
    strad = ((kk.astype(f32) + rng.uniform(0, 1, (len(kk), 3)).astype(f32)) * vs).astype(f32)
    lo, hi = c.min(0) - 4 * vs, c.max(0) + 4 * vs
    box = rng.uniform(lo, hi, (200_000, 3)).astype(f32)                                      # mostly empty space
    exact = (keys[:1000].astype(f32) * vs).astype(f32)                                       # voxel centres
    pts = np.concatenate([band, strad, box, exact, -box[:1000]]).astype(f32)
    d, gr, w = gb.query(pts)
    wr, dr, grr = m.sample(pts)
    assert np.array_equal(w.view(np.uint32), wr.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), dr.view(np.uint32))
    assert np.array_equal(gr.view(np.uint32), grr.view(np.uint32))
    # every case occurs: all 8 corners, some, none
    assert (w > 0).sum() > 10000 and ((w == 0) & (d == 0)).sum() > 1000 and (d == -T).sum() > 1000
    gb.close()


# ---- 3. tracker parity, pass by pass ----------------------------------------------------------------------------------------
def _passwise(pkg, O, gb, m, depth, K, start, conv=1e-3, damping=1.0, sampling=None):
    """each pass k: same hit count (exact on the first pass, which starts from the identical pose), pose within TOL; the same
    decision and pass count at the end"""
    c_r, pose_r, used, trace = B.optimize_sampled(O, m, depth, K, start, conv=conv, damping=damping, sampling=sampling or 1)
    prev_hits = 0
    for k in range(1, used + 1):
        n0 = gb.stats()["n_hit"]
        ck, pk, passes = gb.track(depth, start, iters=k, conv=conv, damping=damping, sampling=sampling)
        hits = gb.stats()["n_hit"] - n0
        c_k, pose_k, used_k, tr_k = B.optimize_sampled(O, m, depth, K, start, iters=k, conv=conv, damping=damping,
                                                      sampling=sampling or 1)
        assert passes == used_k and ck == c_k, (k, passes, used_k, ck, c_k)
        h_pass = hits - prev_hits
        if k == 1:
            assert h_pass == int(tr_k[0, 28]), (h_pass, tr_k[0, 28])
        else:                                   # later passes start from poses that differ in the last bits
            assert abs(h_pass - int(tr_k[k - 1, 28])) <= max(2, 1e-4 * tr_k[k - 1, 28]), (k, h_pass, tr_k[k - 1, 28])
        prev_hits = hits
        assert np.abs(pk[:3] - pose_k[:3]).max() < TOL and np.abs(np.abs(pk[3:]) - np.abs(pose_k[3:])).max() < TOL, (k, pk, pose_k)
    cg, pg, passes = gb.track(depth, start, conv=conv, damping=damping, sampling=sampling)
    assert cg == c_r and passes == used, (cg, c_r, passes, used, trace[:, 35])
    return used


def _tracked_setup(pkg, O, W, H, kind="tum", n=3, seed=0):
    seq = pkg.synth.Sequence(kind, W, H, n_frames=n, seed=seed)
    vs = f32(0.02)
    T = f32(5) * vs
    gb = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=21, map_type=pkg.MAP_BASE)
    d0, R0, t0 = seq.frame(0)
    gb.update(d0, R0, t0)
    keys, pay = gb.export(sorted=True)
    m = B.BaseMap.from_export(keys, pay, vs, T)
    d1, R1, t1 = seq.frame(1)
    start = pose7_from(O, R0, t0)
    return seq, gb, m, d1, start


@pytest.mark.parametrize("conv,damping", [(1e-3, 1.0), (1e-3, 0.5), (1e-2, 1.0), (1e-4, 1.0)])
def test_tracker_parity_passwise(pkg, O, conv, damping):
    seq, gb, m, d1, start = _tracked_setup(pkg, O, 640, 480)
    used = _passwise(pkg, O, gb, m, d1, seq.K, start, conv=conv, damping=damping)
    print("MEASURED base tracker conv %g damping %g: %d passes" % (conv, damping, used))
    gb.close()


@pytest.mark.parametrize("sampling", [2, 3, 5])
def test_tracker_sampled_parity_passwise(pkg, O, sampling):
    seq, gb, m, d1, start = _tracked_setup(pkg, O, 640, 480)
    _passwise(pkg, O, gb, m, d1, seq.K, start, sampling=sampling)
    gb.close()


def test_tracker_parity_c3_geometry(pkg, O):
    seq, gb, m, d1, start = _tracked_setup(pkg, O, 1280, 960)
    _passwise(pkg, O, gb, m, d1, seq.K, start)
    gb.close()


# ---- 4. frame loop ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["track_and_fuse_dev", "track_and_fuse_ahead_dev"])
def test_frame_loop_equals_track_then_update(pkg, O, entry):
    W, H, n = 320, 240, 33
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0)
    vs = f32(0.02)
    T = f32(5) * vs
    fr = [seq.frame(i) for i in range(n)]
    res = []
    for one_call in (True, False):
        g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=21, map_type=pkg.MAP_BASE)
        g.update(*fr[0])
        pose = pose7_from(O, fr[0][1], fr[0][2])
        g.set_pose(pose)
        poses = []
        if one_call:
            dev = [g.upload(f[0]) for f in fr]
            for i in range(1, n):
                if entry == "track_and_fuse_dev":
                    g.track_and_fuse_dev(dev[i])
                else:
                    g.track_and_fuse_ahead_dev(dev[i], dev[i + 1] if i + 1 < n else None)
            g.sync()
            log = g.frame_log()
            assert log.shape[0] == n - 1
            poses = [(int(r[7]), int(r[8]), r[:7].copy()) for r in log]
        else:
            for i in range(1, n):
                conv, pose, passes = g.track(fr[i][0], pose)
                poses.append((int(conv), int(passes), pose.copy()))
                if conv:
                    g.update(fr[i][0], _quat_to_R_f32(pose[3:]), pose[:3])
        k, p = g.export(sorted=True)
        res.append((poses, k, p))
        g.close()
    (p1, k1, v1), (p2, k2, v2) = res
    assert [a[:2] for a in p1] == [b[:2] for b in p2]
    for a, b in zip(p1, p2):
        assert np.array_equal(a[2], b[2])
    assert np.array_equal(k1, k2) and np.array_equal(v1, v2)


# ---- 5. contract ------------------------------------------------------------------------------------------------------------
def test_map_type_contract(pkg):
    W, H = 160, 120
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=1, seed=1)
    vs = f32(0.02)
    gb = pkg.GradSdf(vs, f32(5) * vs, W, H, seq.K, capacity_log2=18, map_type=pkg.MAP_BASE)
    gg = pkg.GradSdf(vs, f32(5) * vs, W, H, seq.K, capacity_log2=18)
    with pytest.raises(pkg.GsdfError) as e:
        gb.set_map_type(7)
    assert e.value.code == pkg.binding.ERR_INVALID
    gb.update(*seq.frame(0))
    gg.update(*seq.frame(0))
    with pytest.raises(pkg.GsdfError) as e:
        gb.set_map_type(pkg.MAP_GRAD)                  # map not empty
    assert e.value.code == pkg.binding.ERR_INVALID and gb.map_type == pkg.MAP_BASE
    gb.set_map_type(pkg.MAP_BASE)                      # (no change: allowed)
    with pytest.raises(pkg.GsdfError) as e:
        gg.merge_from(gb)                              # cross-type merge
    assert e.value.code == pkg.binding.ERR_INVALID
    imgs = np.zeros((1, H, W, 3), f32)
    poses = np.eye(4, dtype=f32).reshape(1, 16)
    with pytest.raises(pkg.GsdfError) as e:
        gb.ba_setup(imgs, poses, np.zeros(1, np.int32))
    assert e.value.code == pkg.binding.ERR_INVALID and "Gradient-SDF" in str(e.value)
    gb.reset()
    assert gb.map_type == pkg.MAP_BASE and gb.count() == 0
    gb.set_map_type(pkg.MAP_GRAD)                      # empty again: allowed
    assert gb.map_type == pkg.MAP_GRAD
    gb.close(); gg.close()


# ---- 6. Scan3D end to end ---------------------------------------------------------------------------------------------------
def test_scan3d_base_sdf_end_to_end(pkg, tmp_path):
    W, H, n = 320, 240, 8
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=0, step_deg=0.5)
    ds = pkg.synth.write_dataset(seq, str(tmp_path / "ds"), layout="synth", with_poses=False)
    res = {}
    for flavour in ("pipe", "sync"):
        r = str(tmp_path / ("out_" + flavour)) + "/"
        os.makedirs(r)
        cmd = [os.path.join(HOST, "Scan3D"), "--input", ds, "--results", r, "--scan-type", "base-sdf", "--data-type", "synth",
               "--voxel-size", "0.02", "--trunc", "5", "--width", str(W), "--height", str(H), "--hash-capacity", "20",
               "--save-sdf"] + (["--sync"] if flavour == "sync" else [])
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert os.path.exists(r + "gradient_sdf_sdf_d.txt") and os.path.exists(r + "gradient_sdf_sdf_weight.txt")
        assert not glob.glob(r + "*_sdf_n*")
        assert os.path.getsize(r + "gradient_sdf_mesh_final.ply") > 1000
        res[flavour] = r
    # the device-resident loop against the facade's blocking RigidPointOptimizer / MapPixelSdf calls
    pa, pb = np.loadtxt(res["pipe"] + "_poses.txt"), np.loadtxt(res["sync"] + "_poses.txt")
    assert pa.shape == pb.shape == (n, 8)
    assert np.abs(pa - pb).max() < 1e-5
    # ... and against the Python binding driving the same loop
    vs = f32(0.02)
    g = pkg.GradSdf(vs, f32(5) * vs, W, H, seq.K, capacity_log2=20, map_type=pkg.MAP_BASE)
    d0 = seq.depth_u16(0).astype(f32) * f32(0.001) if hasattr(seq, "depth_u16") else seq.frame(0)[0]
    g.update(d0, np.eye(3, dtype=f32), np.zeros(3, f32))
    pose = np.array([0, 0, 0, 0, 0, 0, 1], f32)
    for i in range(1, n):
        d = seq.depth_u16(i).astype(f32) * f32(0.001)
        conv, pose, _ = g.track(d, pose)
        if conv:
            g.update(d, _quat_to_R_f32(pose[3:]), pose[:3])
        assert np.abs(pa[i, 1:4] - pose[:3]).max() < 1e-4, (i, pa[i], pose)
    da = np.loadtxt(res["pipe"] + "gradient_sdf_sdf_d.txt")
    assert da.shape[0] == g.count()
    g.close()
