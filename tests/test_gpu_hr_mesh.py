"""The coloured sub-voxel mesh on the GPU (gsdf_color_mesh, GradSdf.color_mesh, host/HrLayeredMarchingCubes.h) against the numpy
restatement of HrLayeredMarchingCubes::computeIsoSurface (tests/hr_mesh_ref.py) fed with the exported snapshot: triangle count
and order, vertex floats bit for bit, colour bytes equal; tiny maps for the boundary rules; the call's contract; the facade's PLY.

Bit equality is what the plain mesh meets for the same interpolate under -ffp-contract=off, and both sides start from the same
exported floats: every operation of the restatement is a correctly rounded float32 / float64 one, as on the device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hr_mesh_ref as HR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32
pytestmark = pytest.mark.gpu
W, H, VS, TRUNC = 160, 120, f32(0.02), 5


def _scene(pkg, n_frames=6, n_kf=6, cap=20, ba_it=2):
    """the recipe of tests/test_gpu_color_upsampler.py::_scene: fuse with vis_ on at the true poses, PhotoBA from perturbed key
    poses (main_photo_ba.cpp:237-306)"""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n_frames, seed=0, noise=False)
    T = f32(TRUNC) * VS
    frames = [seq.frame(i) for i in range(n_frames)]
    kf = np.linspace(0, n_frames - 1, n_kf).astype(np.int32)
    imgs = np.stack([pkg.synth.render_color_bgr(seq, int(i)) for i in kf]).astype(np.float32)
    P = np.stack([pkg.synth.pose16(*seq.pose(int(i))) for i in kf]).astype(np.float32)
    Pp = P.copy()
    rng = np.random.default_rng(0)
    Pp[1:, :3, 3] += (0.004 * rng.standard_normal((len(kf) - 1, 3))).astype(np.float32)
    g = pkg.GradSdf(VS, T, W, H, seq.K, capacity_log2=cap)
    g.enable_vis(max(64, n_frames))
    for f in frames:
        g.update(*f)
    g.ba_setup(imgs, Pp, kf)
    if ba_it:
        g.ba_optimize(ba_it)
    return seq, g, imgs, Pp, kf


@pytest.fixture(scope="module")
def scene(pkg):
    """the small scene with its snapshot, and the restatement of the snapshot at iso 0 (computed once, read only)"""
    seq, g, imgs, Pp, kf = _scene(pkg)
    g.color_compute(len(kf), imgs, Pp, kf)
    keys, rows = g.color_export()
    ref = HR.compute(keys, rows, VS)
    yield g, keys, rows, ref
    g.close()


def _same_mesh(got, ref):
    (t, c), (rt, rc) = got, ref
    assert t.shape == rt.shape and c.shape == rc.shape, (t.shape, rt.shape)
    assert t.dtype == np.float32 and c.dtype == np.uint8
    assert np.array_equal(t.view(np.uint32), rt.view(np.uint32))
    assert np.array_equal(c, rc)


def test_gpu_hr_mesh_parity_small_scene(scene):
    g, keys, rows, ref = scene
    got = g.color_mesh()
    print("triangles", len(got[0]), "restatement", len(ref[0]), "hr voxels", len(keys))
    _same_mesh(got, ref)
    assert len(got[0]) > 1000
    nan_voxels = np.isnan(rows[:, 13:37]).any()
    assert nan_voxels and (got[1] != 0).any() and (got[1].reshape(-1, 3) == 0).all(1).any()      # both kinds of colour occur


def _tiny(pkg, keys, dist, grad=(0, 0, 1), weight=4.0):
    """a map made through merge_raw (raw sums w d, w g, w), no vis_ bit set, and its snapshot"""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=1, seed=0, noise=False)
    g = pkg.GradSdf(VS, f32(TRUNC) * VS, W, H, seq.K, capacity_log2=16)      # the constructor runs gsdf_normals_init
    g.enable_vis(64)
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    pay = np.zeros((len(keys), 5), np.float32)
    pay[:, 0] = f32(weight) * np.asarray(dist, np.float32)
    pay[:, 1:4] = f32(weight) * np.asarray(grad, np.float32)
    pay[:, 4] = weight
    g.merge_raw(keys, pay)
    P = np.eye(4, dtype=np.float32).reshape(1, 16)
    nv = g.color_compute(1, np.zeros((1, H, W, 3), np.float32), P, np.zeros(1, np.int32))
    assert nv == len(keys)
    return g


def _block(lo, shape, drop=()):
    xs, ys, zs = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    rel = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1)
    rel = np.array([r for r in rel if tuple(r) not in set(map(tuple, drop))])
    return rel, rel + np.asarray(lo)


def _plane_z(rel):
    return (rel[:, 2] - 1.15).astype(np.float32) * VS                         # cuts the middle coarse layer


TINY = {
    "single voxel": lambda: (np.array([[3, 4, 5]]), [0.0], (0, 0, 1), 0),
    "3x3x3 plane block": lambda: (_block((0, 0, 0), (3, 3, 3))[1], _plane_z(_block((0, 0, 0), (3, 3, 3))[0]), (0, 0, 1), 32),
    "3x3x3 with one voxel missing": lambda: (_block((0, 0, 0), (3, 3, 3), [(1, 1, 1)])[1],
                                              _plane_z(_block((0, 0, 0), (3, 3, 3), [(1, 1, 1)])[0]), (0, 0, 1), 14),
    # 7 x 5 x 4 = 140 voxels: four full workgroups of 32 voxels and a partial one; a slanted plane (distances halved to stay
    # inside the snapshot's gate of sqrt(3) voxels)
    "140 voxels, slanted": lambda: (_block((2, 1, 7), (7, 5, 4))[1],
                                     ((_block((2, 1, 7), (7, 5, 4))[0] @ np.array([0.3, 0.2, 0.9])) - 2.6).astype(np.float32) * f32(0.5) * VS,
                                     (0.3, 0.2, 0.9), None),
    "negative keys": lambda: (_block((-5, -9, -3), (4, 3, 3))[1],
                              ((_block((-5, -9, -3), (4, 3, 3))[0] @ np.array([0.5, -0.4, 0.7])) - 0.6).astype(np.float32) * f32(0.5) * VS,
                              (0.5, -0.4, 0.7), None),
}


@pytest.mark.parametrize("name", list(TINY))
def test_gpu_hr_mesh_tiny_maps(pkg, name):
    keys, dist, grad, n_expected = TINY[name]()
    g = _tiny(pkg, keys, dist, grad)
    k, r = g.color_export()
    assert len(k) == len(keys) and (name != "140 voxels, slanted" or len(k) % 32)
    assert np.isnan(r[:, 13:37]).all()                                        # no vis_ bit: every colour NaN, every byte 0
    ref = HR.compute(k, r, VS)
    got = g.color_mesh()
    print(name, "triangles", len(got[0]), "restatement", len(ref[0]))
    _same_mesh(got, ref)
    assert np.all(got[1] == 0)
    if n_expected is not None:
        assert len(got[0]) == n_expected
    else:
        assert len(got[0]) > 0
    g.close()


def test_gpu_hr_mesh_box_too_large_for_the_sweep_key(pkg):
    """two voxels more than 2^19 apart: 2 extent fine cells do not fit 20 bits -- an error, not a wrapped key"""
    g = _tiny(pkg, [[0, 0, 0], [600000, 0, 0]], [0.0, 0.0])
    with pytest.raises(pkg.binding.GsdfError) as e:
        g.color_mesh()
    assert e.value.code == pkg.binding.ERR_INVALID and "2^19" in str(e.value)
    g.close()


def test_gpu_hr_mesh_contract(pkg, scene):
    g, keys, rows, ref = scene
    L, INVALID = g.L, pkg.binding.ERR_INVALID
    u8p = C.POINTER(C.c_uint8)
    fresh = pkg.GradSdf(VS, f32(TRUNC) * VS, W, H, np.array([[100, 0, 80], [0, 100, 60], [0, 0, 1]], np.float32), capacity_log2=16)
    with pytest.raises(pkg.binding.GsdfError) as e:                           # before any color_compute
        fresh.color_mesh()
    assert e.value.code == INVALID
    fresh.close()
    n = C.c_int64(0)
    assert L.gsdf_color_mesh(g.h, C.c_float(0), None, None, 0, C.byref(n)) == 0      # the sizing call ...
    need = n.value
    assert need == len(ref[0])
    tris = np.empty((need, 3, 3), np.float32)
    rgb = np.empty((need, 3, 3), np.uint8)
    got = C.c_int64(0)
    assert L.gsdf_color_mesh(g.h, C.c_float(0), pkg.binding._fp(tris), rgb.ctypes.data_as(u8p), need, C.byref(got)) == 0
    assert got.value == need                                                  # ... and the exact-size call agree
    _same_mesh((tris, rgb), ref)
    short = np.empty((need - 1, 3, 3), np.float32)
    got = C.c_int64(0)
    assert L.gsdf_color_mesh(g.h, C.c_float(0), pkg.binding._fp(short), None, need - 1, C.byref(got)) == INVALID
    assert got.value == need                                                  # one triangle short: the need is reported
    only = np.empty((need, 3, 3), np.float32)
    assert L.gsdf_color_mesh(g.h, C.c_float(0), pkg.binding._fp(only), None, need, C.byref(got)) == 0      # colors_out = NULL
    assert np.array_equal(only.view(np.uint32), ref[0].view(np.uint32))
    iso = g.color_mesh(iso=0.003)
    _same_mesh(iso, HR.compute(keys, rows, VS, iso=0.003))
    assert len(iso[0]) != need or not np.array_equal(iso[0], ref[0])


def test_gpu_hr_mesh_leaves_table_snapshot_and_cloud(scene):
    g, keys, rows, ref = scene
    before = (g.export(sorted=True), g.color_export(), g.color_cloud())
    g.color_mesh()
    g.color_mesh(iso=0.003)
    after = (g.export(sorted=True), g.color_export(), g.color_cloud())
    for a, b in zip(before, after):
        for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
            assert x.shape == y.shape and x.tobytes() == y.tobytes()


def test_gpu_hr_mesh_follows_the_next_compute(pkg):
    seq, g, imgs, Pp, kf = _scene(pkg, ba_it=0)
    g.color_compute(len(kf), imgs, Pp, kf)
    first = g.color_mesh()
    g.update(*seq.frame(3))                                                   # more fusion: the snapshot, and so the mesh, stay
    _same_mesh(g.color_mesh(), first)
    g.color_compute(len(kf), imgs, Pp, kf)
    second = g.color_mesh()
    _same_mesh(second, HR.compute(*g.color_export(), VS))
    assert second[0].shape != first[0].shape or not np.array_equal(second[0], first[0])
    g.close()


def test_gpu_hr_mesh_facade_ply_matches_restatement(pkg, tmp_path):
    """host/color_mesh_selftest: MapGradPixelSdf::update, ColorUpsampler, extractMesh through HrLayeredMarchingCubes -- its PLY
    text against one written from the restatement of the snapshot it dumps"""
    n = 4
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0, noise=False)
    d = tmp_path
    np.asarray(seq.K, np.float32).reshape(9).tofile(d / "K.bin")
    np.stack([seq.frame(i)[0] for i in range(n)]).astype(np.float32).tofile(d / "depth.bin")
    np.stack([pkg.synth.render_color_bgr(seq, i) for i in range(n)]).astype(np.float32).tofile(d / "images.bin")
    np.stack([pkg.synth.pose16(*seq.pose(i)) for i in range(n)]).astype(np.float32).tofile(d / "poses.bin")
    out = subprocess.run([os.path.join(HOST, "color_mesh_selftest"), str(d), str(W), str(H), str(n), repr(float(VS)), str(TRUNC)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "color_mesh_selftest: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Mesh %s.ply successfully saved." % (d / "mesh") in out.stdout
    keys = np.fromfile(d / "snap_keys.bin", np.int32).reshape(-1, 3)
    rows = np.fromfile(d / "snap_rows.bin", np.float32).reshape(-1, 37)
    tris, rgb = HR.compute(keys, rows, VS)
    assert len(tris) > 1000
    assert (d / "mesh.ply").read_text() == HR.ply_text(tris, rgb)
