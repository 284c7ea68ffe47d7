"""The indexed iso-surface mesh on the GPU (gsdf_extract_mesh_indexed, GradSdf.extract_mesh_indexed, the host facade and
Scan3D --mesh-indexed) against the numpy restatement (tests/indexed_mesh_ref.py) fed with the context's own export: faces and
vertex positions bit for bit, normals within 1e-4 (the project's bar for gradients); V[F] against the soup of gsdf_extract_mesh
within the cost of welding measured on the CPU (indexed_mesh_ref.WELD_MEASURED); the call's protocol; an analytic closed sphere; the binary PLY.

Bit equality of positions is what the soup meets for the same interpolate under -ffp-contract=off; the normal passes through
float32 square roots and divisions on both sides and is held to the gradient bar instead."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indexed_mesh_ref as IM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32
pytestmark = pytest.mark.gpu


def _fixture_map(pkg, name, frames, cap, map_type=None):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    depth = z["depth_u16"].astype(np.float32) * np.float32(z["unit"])
    g = pkg.GradSdf(z["voxel_size"], z["trunc_dist"], int(z["W"]), int(z["H"]), z["K"], capacity_log2=cap, map_type=map_type)
    for i in range(frames):
        g.update(depth[i], z["R"][i], z["t"][i])
    return g, f32(z["voxel_size"])


def _first_triangles():
    tt = IM.TRI.copy()
    tt[:, 3:] = -1                                                             # a caller's table: the first triangle of every case
    return tt


def _check(g, vs, iso=0.0, tri_table=None, min_faces=1):
    """every property of one extraction; returns (V, N, F, restatement)"""
    keys, pay = g.export(sorted=True)
    ref = IM.compute(keys, pay, vs, iso=iso, tri_table=tri_table)
    V, N, F = g.extract_mesh_indexed(tri_table=tri_table, iso=iso)
    soup = g.extract_mesh(tri_table=tri_table, iso=iso)
    cost = IM.weld_cost(V, F, soup, vs)
    dn = float(np.abs(N.astype(np.float64) - ref["N"].astype(np.float64)).max()) if len(N) == len(ref["N"]) and len(N) else 0.0
    print("voxels %d faces %d (restatement %d) vertices %d (%d), %.3f vertices per face, weld cost %.3f spacings, normals |d|max %.2e"
          % (len(keys), len(F), len(ref["F"]), len(V), len(ref["V"]), len(V) / max(len(F), 1), cost, dn))
    assert V.dtype == np.float32 and N.dtype == np.float32 and F.dtype == np.int32
    assert len(F) >= min_faces
    assert F.shape == ref["F"].shape and np.array_equal(F, ref["F"])
    assert V.shape == ref["V"].shape and np.array_equal(V.view(np.uint32), ref["V"].view(np.uint32))
    assert N.shape == ref["N"].shape and dn <= 1e-4
    # the soup: same faces in the same order; the weld moves a corner by a rounding of the other walk's interpolation at most
    assert soup.shape == ref["soup"].shape == (len(F), 3, 3) and np.array_equal(soup.view(np.uint32), ref["soup"].view(np.uint32))
    assert IM.no_guarded_edges(pay, iso) and cost <= IM.WELD_MEASURED
    assert F.min() == 0 and F.max() == len(V) - 1 and len(np.unique(F)) == len(V)          # every id in [0, nV) is used
    assert (F[:, 0] != F[:, 1]).all() and (F[:, 0] != F[:, 2]).all() and (F[:, 1] != F[:, 2]).all()
    nn = np.linalg.norm(N.astype(np.float64), axis=1)
    assert ((np.abs(nn - 1) < 1e-5) | (nn == 0)).all()
    return V, N, F, ref


@pytest.fixture(scope="module")
def tum(pkg):
    g, vs = _fixture_map(pkg, "tum_128x96", 3, 16)
    yield g, vs
    g.close()


def test_gpu_indexed_mesh_spheres_two_frames(pkg):
    g, vs = _fixture_map(pkg, "spheres_64x48", 2, 14)
    _check(g, vs)
    g.close()


def test_gpu_indexed_mesh_tum_three_frames(tum):
    g, vs = tum
    V, N, F, ref = _check(g, vs, min_faces=3000)
    assert (np.linalg.norm(N, axis=1) > 0).mean() > 0.99


def test_gpu_indexed_mesh_base_sdf_context(pkg):
    g, vs = _fixture_map(pkg, "spheres_160x120", 2, 16, map_type=pkg.MAP_BASE)
    assert g.map_type == pkg.MAP_BASE
    V, N, F, ref = _check(g, vs, min_faces=1000)
    assert (np.linalg.norm(N, axis=1) > 0).any()                               # a base context stores the gradient sums too
    g.close()


def test_gpu_indexed_mesh_iso_quarter_voxel(tum):
    g, vs = tum
    V, N, F, ref = _check(g, vs, iso=float(f32(0.25) * vs), min_faces=3000)
    V0 = g.extract_mesh_indexed()[0]
    assert V.shape != V0.shape or not np.array_equal(V, V0)


def test_gpu_indexed_mesh_callers_table(tum):
    g, vs = tum
    V, N, F, ref = _check(g, vs, tri_table=_first_triangles(), min_faces=1000)
    assert len(F) < len(g.extract_mesh())


def test_gpu_indexed_mesh_analytic_sphere_is_closed(pkg):
    """the sphere of tests/test_indexed_mesh.py loaded through merge_raw: keys on both sides of 0 on every axis and in dozens of
    4 x 4 x 4 blocks -- a weld that went wrong across a block boundary or a negative coordinate leaves an open edge"""
    vs, radius, centre = f32(0.02), 6.3, (0.37, -0.21, 0.13)
    keys, pay = IM.sphere_map(radius, centre, vs, band=3.0)
    g = pkg.GradSdf(vs, f32(5) * vs, 64, 48, pkg.synth.intrinsics(64, 48), capacity_log2=15)
    raw = pay.copy()                                                           # raw sums s = w d, w g, w with w = 1
    g.merge_raw(keys, raw)
    V, N, F, ref = _check(g, vs, min_faces=1000)
    assert ref["table_triangles"] == len(F)                                    # no degenerate triangle dropped: closedness is fair
    nv, ne, nf, bad = IM.manifold_counts(F)
    print("sphere: vertices %d edges %d faces %d, edges not in two faces %d" % (nv, ne, nf, bad))
    assert bad == 0 and nv == len(V) and nv - ne + nf == 2
    c = np.asarray(centre, np.float64) * float(vs)
    rho = np.linalg.norm(V.astype(np.float64) - c, axis=1)
    assert np.abs(rho - radius * float(vs)).max() <= 0.05 * float(vs)
    assert np.abs(N.astype(np.float64) + (V.astype(np.float64) - c) / rho[:, None]).max() < 0.02
    g.close()


def test_gpu_indexed_mesh_zero_and_nan_gradients(pkg):
    """the (0, 0, 0) normal on the device: a map without gradients, and one where the blend of a vertex meets a NaN gradient"""
    vs = f32(0.02)
    xs, ys, zs = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    keys = (np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1) + np.array([-1, 3, 7])).astype(np.int32)     # across a block boundary in x
    raw = np.zeros((8, 5), np.float32)
    raw[:, 0] = (keys[:, 2] - 7 - 0.4).astype(np.float32) * vs                 # w = 1: the raw sums are the values
    raw[:, 4] = 1
    K = pkg.synth.intrinsics(64, 48)
    g = pkg.GradSdf(vs, f32(5) * vs, 64, 48, K, capacity_log2=14)
    g.merge_raw(keys, raw)
    V, N, F, ref = _check(g, vs, min_faces=2)
    assert len(F) == 2 and len(V) == 4 and np.all(N == 0)
    g.close()
    raw[:, 3] = 1
    raw[keys[:, 0] == -1, 1] = np.nan
    g = pkg.GradSdf(vs, f32(5) * vs, 64, 48, K, capacity_log2=14)
    g.merge_raw(keys, raw)
    V, N, F, ref = _check(g, vs, min_faces=2)
    lone = np.isclose(V[:, 0], -1 * float(vs))
    assert lone.sum() == 2 and np.all(N[lone] == 0) and np.allclose(N[~lone], [0, 0, -1])
    g.close()


def _raw_call(g, V, N, F, max_v, max_f, iso=0.0):
    nv, nf = C.c_int64(-1), C.c_int64(-1)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))           # noqa: E731
    ip = None if F is None else F.ctypes.data_as(C.POINTER(C.c_int32))
    rc = g.L.gsdf_extract_mesh_indexed(g.h, C.c_float(iso), None, fp(V), fp(N), ip, max_v, max_f, C.byref(nv), C.byref(nf))
    return rc, nv.value, nf.value


def test_gpu_indexed_mesh_protocol(pkg, tum):
    g, vs = tum
    INVALID = pkg.binding.ERR_INVALID
    soup_before = g.extract_mesh()
    V0, N0, F0 = g.extract_mesh_indexed()
    rc, nv, nf = _raw_call(g, None, None, None, 0, 0)                          # the sizing call reports the counts
    assert (rc, nv, nf) == (0, len(V0), len(F0))
    for dv, df in ((1, 0), (0, 1)):                                            # one too small in vertices / in faces: both untouched
        V = np.full((nv, 3), 7.5, np.float32)
        N = np.full((nv, 3), 7.5, np.float32)
        F = np.full((nf, 3), -7, np.int32)
        rc, rv, rf = _raw_call(g, V, N, F, nv - dv, nf - df)
        assert rc == INVALID and (rv, rf) == (nv, nf) and "too small" in g.L.gsdf_last_error().decode()
        assert (V == 7.5).all() and (N == 7.5).all() and (F == -7).all()
    V = np.empty((nv, 3), np.float32)
    F = np.empty((nf, 3), np.int32)
    assert _raw_call(g, V, None, F, nv, nf) == (0, nv, nf)                     # normals_out = NULL
    assert V.tobytes() == V0.tobytes() and F.tobytes() == F0.tobytes()
    assert _raw_call(g, None, None, F, 0, nf)[0] == INVALID                    # room for faces only is not a sizing call
    nvp = C.c_int64(0)
    assert g.L.gsdf_extract_mesh_indexed(g.h, C.c_float(0), None, None, None, None, 0, 0, C.byref(nvp), None) == INVALID
    assert g.L.gsdf_extract_mesh_indexed(g.h, C.c_float(0), None, None, None, F.ctypes.data_as(C.POINTER(C.c_int32)), nv, nf,
                                         C.byref(nvp), C.byref(nvp)) == INVALID                      # max_vertices > 0 without a buffer
    # a second call, and the map moved into a larger table: the same bytes
    again = g.extract_mesh_indexed()
    cap = g.capacity_log2()
    g.grow(cap + 1)
    assert g.capacity_log2() == cap + 1
    grown = g.extract_mesh_indexed()
    for a, b, c in zip((V0, N0, F0), again, grown):
        assert a.shape == b.shape == c.shape and a.tobytes() == b.tobytes() == c.tobytes()
    assert g.extract_mesh().tobytes() == soup_before.tobytes()                 # gsdf_extract_mesh before and after
    # an empty map
    e = pkg.GradSdf(vs, f32(5) * vs, 64, 48, pkg.synth.intrinsics(64, 48), capacity_log2=14)
    assert _raw_call(e, None, None, None, 0, 0) == (0, 0, 0)
    Ve, Ne, Fe = e.extract_mesh_indexed()
    assert Ve.shape == (0, 3) and Ne.shape == (0, 3) and Fe.shape == (0, 3)
    V = np.full((4, 3), 7.5, np.float32)
    F = np.full((4, 3), -7, np.int32)
    assert _raw_call(e, V, V.copy(), F, 4, 4) == (0, 0, 0) and (V == 7.5).all() and (F == -7).all()
    e.close()


def _dataset(pkg, tmp_path, W=160, H=120, n=3):
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=4, step_deg=2.0)
    return seq, pkg.synth.write_dataset(seq, str(tmp_path / "ds"), layout="synth")


def test_scan3d_mesh_indexed_flag(pkg, O, tmp_path):
    """Scan3D --mesh-indexed on the synthetic directory of tests/test_host.py: one more file, the others byte for byte as without
    the flag; the binary PLY equals extract_mesh_indexed of a context fused from the same files' content the CLI's way (pose file
    -> quaternion -> R -> SE3 -> R, the path of test_host.py::test_scan3d_gt_pose_fusion_matches_oracle)."""
    W, H, n = 160, 120, 3
    seq, ds = _dataset(pkg, tmp_path, W, H, n)
    res = {}
    for flag in (False, True):
        r = str(tmp_path / ("out%d" % flag)) + "/"
        os.makedirs(r)
        cmd = [os.path.join(HOST, "Scan3D"), "--input", ds, "--results", r, "--scan-type", "grad-sdf", "--data-type", "synth",
               "--voxel-size", "0.02", "--trunc", "5", "--width", str(W), "--height", str(H), "--hash-capacity", "18", "--save-sdf", "--sync"]                # --sync: update() per frame, the entry g.update() below takes
        out = subprocess.run(cmd + (["--mesh-indexed"] if flag else []), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert ("Save indexed mesh to disk" in out.stdout) == flag
        res[flag] = r
    plain, with_flag = sorted(os.listdir(res[False])), sorted(os.listdir(res[True]))
    assert with_flag == sorted(plain + ["mesh_indexed.ply"]) and "gradient_sdf_mesh_final.ply" in plain
    for f in plain:
        assert open(res[False] + f, "rb").read() == open(res[True] + f, "rb").read(), f
    V, N, F, head = IM.parse_indexed_ply(res[True] + "mesh_indexed.ply")
    assert head[1] == "format binary_little_endian 1.0" and len(F) > 300
    vs = f32(0.02)
    g = pkg.GradSdf(vs, f32(5) * vs, W, H, seq.K, capacity_log2=18)
    poses = np.loadtxt(ds + "pose.txt")
    for i in range(n):
        d = seq.depth_u16(i).astype(np.float32) * np.float32(0.001)
        R = O.quat_to_R(O.R_to_quat(O.quat_to_R(poses[i, 4:8].astype(np.float32))))
        g.update(d, R, poses[i, 1:4].astype(np.float32))
    Vg, Ng, Fg = g.extract_mesh_indexed()
    g.close()
    print("Scan3D: vertices %d faces %d; python context %d / %d; ply %d bytes, ascii soup %d bytes"
          % (len(V), len(F), len(Vg), len(Fg), os.path.getsize(res[True] + "mesh_indexed.ply"),
             os.path.getsize(res[True] + "gradient_sdf_mesh_final.ply")))
    assert F.shape == Fg.shape and np.array_equal(F, Fg)
    assert np.array_equal(V.view(np.uint32), Vg.view(np.uint32)) and np.array_equal(N.view(np.uint32), Ng.view(np.uint32))


@pytest.mark.parametrize("kind", ["grad", "base"])
def test_indexed_mesh_selftest_binary(pkg, tmp_path, kind):
    """host/indexed_mesh_selftest: MapGradPixelSdf / MapPixelSdf::extract_mesh_indexed through the C++ facade; its PLY and its
    C-ABI arrays against the restatement of the map it dumps"""
    W, H, n, vs = 160, 120, 3, f32(0.02)
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=4, step_deg=2.0)
    d = tmp_path
    np.asarray(seq.K, np.float32).reshape(9).tofile(d / "K.bin")
    np.stack([seq.frame(i)[0] for i in range(n)]).astype(np.float32).tofile(d / "depth.bin")
    np.stack([pkg.synth.pose16(*seq.pose(i)) for i in range(n)]).astype(np.float32).tofile(d / "poses.bin")
    out = subprocess.run([os.path.join(HOST, "indexed_mesh_selftest"), str(d), str(W), str(H), str(n), repr(float(vs)), "5"]
                         + (["base"] if kind == "base" else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "indexed_mesh_selftest: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    keys = np.fromfile(d / "map_keys.bin", np.int32).reshape(-1, 3)
    pay = np.fromfile(d / "map_payload.bin", np.float32).reshape(-1, 5)
    ref = IM.compute(keys, pay, vs)
    V, N, F, head = IM.parse_indexed_ply(str(d / "mesh_indexed.ply"))
    assert len(F) > 300 and "vertices %d faces %d" % (len(V), len(F)) in out.stdout
    assert np.array_equal(F, ref["F"]) and np.array_equal(V.view(np.uint32), ref["V"].view(np.uint32))
    assert np.abs(N - ref["N"]).max() <= 1e-4
    assert np.fromfile(d / "mesh_v.bin", np.float32).tobytes() == V.tobytes()
    assert np.fromfile(d / "mesh_n.bin", np.float32).tobytes() == N.tobytes()
    assert np.fromfile(d / "mesh_f.bin", np.int32).tobytes() == F.tobytes()
