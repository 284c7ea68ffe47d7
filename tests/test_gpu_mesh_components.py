"""Connected components of the indexed mesh and the filtered mesh on the GPU (gsdf_mesh_components,
gsdf_extract_mesh_indexed_filtered, GradSdf.mesh_components / extract_mesh_indexed_filtered, the host facade and
Scan3D --mesh-min-faces) against the numpy restatement (tests/mesh_components_ref.py) fed with the context's own
extract_mesh_indexed(): ids, labels, counts and the filtered V / N / F bit for bit, the boxes by value (both are minima and maxima
of the same floats; only the sign of a zero is free)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indexed_mesh_ref as IM  # noqa: E402
import mesh_components_ref as MC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32
pytestmark = pytest.mark.gpu
MIN_FACES = (1, 2, 10, 100, 10**9, MC.KEEP_LARGEST)


def _fixture_map(pkg, name, frames, cap, map_type=None):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    depth = z["depth_u16"].astype(np.float32) * np.float32(z["unit"])
    g = pkg.GradSdf(z["voxel_size"], z["trunc_dist"], int(z["W"]), int(z["H"]), z["K"], capacity_log2=cap, map_type=map_type)
    for i in range(frames):
        g.update(depth[i], z["R"][i], z["t"][i])
    return g, f32(z["voxel_size"])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check(g, iso=0.0, tri_table=None, min_faces=MIN_FACES, label=""):
    """every property of one map at one iso value; returns the restatement's component dict"""
    V, N, F = g.extract_mesh_indexed(tri_table=tri_table, iso=iso)
    ref = MC.compute(V, F)
    vc, fc, counts, bbox = g.mesh_components(iso=iso, tri_table=tri_table)
    order = np.argsort(-ref["counts"][:, 0], kind="stable")
    print("%s iso %.4g: faces %d vertices %d components %d (device %d), face counts %s"
          % (label, iso, len(F), len(V), ref["C"], len(counts), " / ".join(str(int(ref["counts"][i, 0])) for i in order[:12])))
    assert _same(vc, ref["vertex_comp"]) and _same(fc, ref["face_comp"]) and _same(counts, ref["counts"])
    assert bbox.dtype == np.float32 and bbox.shape == ref["bbox"].shape and np.array_equal(bbox, ref["bbox"])
    for m in min_faces:
        Vr, Nr, Fr, Cr, kr = MC.filter_mesh(V, N, F, m, ref)
        Vg, Ng, Fg, Cg, kg = g.extract_mesh_indexed_filtered(m, iso=iso, tri_table=tri_table)
        print("  min_faces %d: kept %d of %d components, faces %d of %d, vertices %d of %d" % (m, kg, Cg, len(Fg), len(F), len(Vg), len(V)))
        assert (Cg, kg) == (Cr, kr), m
        assert _same(Vg, Vr) and _same(Ng, Nr) and _same(Fg, Fr), m
    return ref


@pytest.fixture(scope="module")
def tum(pkg):
    g, vs = _fixture_map(pkg, "tum_128x96", 3, 16)
    yield g, vs
    g.close()


@pytest.fixture(scope="module")
def spheres(pkg):
    g, vs = _fixture_map(pkg, "spheres_160x120", 2, 16)
    yield g, vs
    g.close()


def _has_work(ref):
    assert ref["C"] > 3 and (ref["counts"][:, 0] < 10).any()                   # the filter has something to remove


def test_gpu_mesh_components_spheres(spheres):
    g, vs = spheres
    _has_work(_check(g, label="spheres_160x120"))
    _has_work(_check(g, iso=float(f32(0.25) * vs), label="spheres_160x120"))


def test_gpu_mesh_components_tum(tum):
    g, vs = tum
    _has_work(_check(g, label="tum_128x96"))
    _has_work(_check(g, iso=float(f32(0.25) * vs), label="tum_128x96"))


def test_gpu_mesh_components_callers_table(tum):
    g, vs = tum
    tt = IM.TRI.copy()
    tt[:, 3:] = -1                                                             # a caller's table: the first triangle of every case
    ref = _check(g, tri_table=tt, label="tum_128x96, first triangles")
    assert ref["C"] > 3


def test_gpu_mesh_components_base_sdf_context(pkg):
    g, vs = _fixture_map(pkg, "spheres_160x120", 2, 16, map_type=pkg.MAP_BASE)
    assert g.map_type == pkg.MAP_BASE
    _has_work(_check(g, label="spheres_160x120 base"))
    g.close()


def _load(pkg, pieces, cap=18, vs=f32(0.02)):
    g = pkg.GradSdf(vs, f32(5) * vs, 64, 48, pkg.synth.intrinsics(64, 48), capacity_log2=cap)
    for keys, pay in pieces:
        g.merge_raw(keys, pay.copy())                                          # raw sums s = w d, w g, w with w = 1
    return g


def test_gpu_long_strip_is_one_component(pkg):
    """about 8 k voxels in hundreds of blocks, negative and positive keys, a graph whose diameter is the strip's length: a label
    spread limited in its rounds leaves it in pieces.  The union is one lock-free pass, so there are no rounds to count: 1."""
    L = 1000
    g = _load(pkg, [MC.strip_map(L)])
    ref = _check(g, min_faces=(1, 4 * L, 4 * L + 1, MC.KEEP_LARGEST), label="strip")
    vc, fc, counts, bbox = g.mesh_components()
    print("strip: faces %d vertices %d components %d, union passes 1" % (counts[0, 0], counts[0, 1], len(counts)))
    assert ref["C"] == 1 and counts.tolist() == [list(MC.strip_counts(L))] and not vc.any() and not fc.any()
    assert bbox[0, 0] == f32(-L) * f32(0.02) and bbox[0, 3] == f32(L) * f32(0.02) and bbox[0, 2] == bbox[0, 5]
    g.close()


def test_gpu_two_equal_strips_and_a_small_piece(pkg):
    L = 1000
    g = _load(pkg, [MC.strip_map(L), MC.strip_map(L, y0=4), MC.strip_map(0, y0=8, cubes=3)])
    big, small = MC.strip_counts(L), MC.strip_counts(cubes=3)
    ref = _check(g, min_faces=(1, small[0], small[0] + 1, big[0], big[0] + 1, MC.KEEP_LARGEST), label="strips")
    V, N, F = g.extract_mesh_indexed()
    vc, fc, counts, bbox = g.mesh_components()
    assert counts.tolist() == [list(big), list(big), list(small)]
    Vk, Nk, Fk, nc, kept = g.extract_mesh_indexed_filtered(pkg.MESH_KEEP_LARGEST)
    assert (nc, kept) == (3, 1) and vc[0] == 0 and _same(Vk, V[vc == 0]) and len(Fk) == big[0]         # the one that holds vertex 0
    Vk, Nk, Fk, nc, kept = g.extract_mesh_indexed_filtered(small[0] + 1)                               # between the two counts
    assert (nc, kept) == (3, 2) and _same(Vk, V[vc < 2]) and len(Fk) == 2 * big[0]
    g.close()


def test_gpu_analytic_sphere_is_one_component(pkg):
    vs, radius, centre = f32(0.02), 6.3, (0.37, -0.21, 0.13)
    keys, pay = IM.sphere_map(radius, centre, vs, band=3.0)
    g = _load(pkg, [(keys, pay)], cap=15, vs=vs)
    V, N, F = g.extract_mesh_indexed()
    ref = _check(g, min_faces=(1, 2, len(F) // 2, len(F), MC.KEEP_LARGEST), label="sphere")
    assert ref["C"] == 1 and len(F) > 1000
    for m in (1, len(F) // 2, len(F)):
        Vk, Nk, Fk, nc, kept = g.extract_mesh_indexed_filtered(m)
        assert (nc, kept) == (1, 1) and _same(Vk, V) and _same(Nk, N) and _same(Fk, F)
    assert g.extract_mesh_indexed_filtered(len(F) + 1)[2].shape == (0, 3)
    g.close()


def _i32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _raw_components(g, vc, fc, counts, bbox, max_v, max_f, max_c):
    nv, nf, nc = C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    rc = g.L.gsdf_mesh_components(g.h, C.c_float(0), None, _i32(vc), _i32(fc), max_v, max_f, _i32(counts), _fp(bbox), max_c,
                                  C.byref(nv), C.byref(nf), C.byref(nc))
    return rc, nv.value, nf.value, nc.value


def _raw_filtered(g, m, V, N, F, max_v, max_f):
    n = [C.c_int64(-1) for _ in range(4)]
    rc = g.L.gsdf_extract_mesh_indexed_filtered(g.h, C.c_float(0), None, m, _fp(V), _fp(N), _i32(F), max_v, max_f, *[C.byref(x) for x in n])
    return (rc,) + tuple(x.value for x in n)


def test_gpu_mesh_components_protocol(pkg, tum):
    g, vs = tum
    INVALID = pkg.binding.ERR_INVALID
    soup_before = g.extract_mesh()
    V0, N0, F0 = g.extract_mesh_indexed()
    vc0, fc0, counts0, bbox0 = g.mesh_components()
    nv, nf, nc = len(V0), len(F0), len(counts0)
    assert _raw_components(g, None, None, None, None, 0, 0, 0) == (0, nv, nf, nc)                       # the sizing call
    sent = lambda: (np.full(nv, -7, np.int32), np.full(nf, -7, np.int32), np.full((nc, 2), -7, np.int32),        # noqa: E731
                    np.full((nc, 6), 7.5, np.float32))
    for dv, df, dc in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):                       # each maximum one too small: nothing is written
        vc, fc, counts, bbox = sent()
        assert _raw_components(g, vc, fc, counts, bbox, nv - dv, nf - df, nc - dc) == (INVALID, nv, nf, nc)
        assert "too small" in g.L.gsdf_last_error().decode()
        assert (vc == -7).all() and (fc == -7).all() and (counts == -7).all() and (bbox == 7.5).all()
    # NULL combinations: a maximum counts only where its array is given
    vc, fc, counts, bbox = sent()
    assert _raw_components(g, vc, None, None, None, nv, 0, 0) == (0, nv, nf, nc) and _same(vc, vc0)
    assert _raw_components(g, None, fc, None, None, 0, nf, 0) == (0, nv, nf, nc) and _same(fc, fc0)
    assert _raw_components(g, None, None, counts, None, 0, 0, nc) == (0, nv, nf, nc) and _same(counts, counts0)
    assert _raw_components(g, None, None, None, bbox, 0, 0, nc) == (0, nv, nf, nc) and _same(bbox, bbox0)
    assert _raw_components(g, None, None, None, None, nv, nf, nc) == (0, nv, nf, nc)
    assert _raw_components(g, vc, None, None, bbox, nv, 0, 0)[0] == INVALID                            # bbox given, no room for it
    one = C.c_int64(0)
    assert g.L.gsdf_mesh_components(g.h, C.c_float(0), None, None, None, 0, 0, None, None, 0, C.byref(one), C.byref(one), None) == INVALID
    # the filtered mesh: its sizing call reports the filtered counts
    Vr, Nr, Fr, Cr, kr = MC.filter_mesh(V0, N0, F0, 10)
    kv, kf = len(Vr), len(Fr)
    assert 0 < kf < nf
    assert _raw_filtered(g, 10, None, None, None, 0, 0) == (0, kv, kf, Cr, kr)
    for dv, df in ((1, 0), (0, 1)):
        V, N, F = np.full((kv, 3), 7.5, np.float32), np.full((kv, 3), 7.5, np.float32), np.full((kf, 3), -7, np.int32)
        assert _raw_filtered(g, 10, V, N, F, kv - dv, kf - df) == (INVALID, kv, kf, Cr, kr)
        assert "too small" in g.L.gsdf_last_error().decode()
        assert (V == 7.5).all() and (N == 7.5).all() and (F == -7).all()
    V, F = np.empty((kv, 3), np.float32), np.empty((kf, 3), np.int32)
    assert _raw_filtered(g, 10, V, None, F, kv, kf) == (0, kv, kf, Cr, kr) and _same(V, Vr) and _same(F, Fr)     # normals_out = NULL
    assert _raw_filtered(g, 10, None, None, F, kv, kf)[0] == INVALID                                    # max_vertices > 0 without a buffer
    for bad in (0, -2):
        assert _raw_filtered(g, bad, None, None, None, 0, 0)[0] == INVALID
        with pytest.raises(pkg.GsdfError):
            g.extract_mesh_indexed_filtered(bad)
    assert _raw_filtered(g, 10**9, V, None, F, kv, kf) == (0, 0, 0, Cr, 0)                              # above every component: 0 / 0, OK
    # a second call, and the map moved into a larger table: the same bytes
    first = g.mesh_components() + g.extract_mesh_indexed_filtered(10)[:3] + g.extract_mesh_indexed_filtered(pkg.MESH_KEEP_LARGEST)[:3]
    cap = g.capacity_log2()
    g.grow(cap + 1)
    assert g.capacity_log2() == cap + 1
    grown = g.mesh_components() + g.extract_mesh_indexed_filtered(10)[:3] + g.extract_mesh_indexed_filtered(pkg.MESH_KEEP_LARGEST)[:3]
    for a, b, c in zip((vc0, fc0, counts0, bbox0, Vr, Nr, Fr), first, grown):
        assert _same(a, b) and _same(a, c)
    for a, b in zip(first[7:], grown[7:]):
        assert _same(a, b)
    assert _same(g.extract_mesh(), soup_before)                                # the older entries before and after
    for a, b in zip((V0, N0, F0), g.extract_mesh_indexed()):
        assert _same(a, b)
    # an empty map
    e = pkg.GradSdf(vs, f32(5) * vs, 64, 48, pkg.synth.intrinsics(64, 48), capacity_log2=14)
    assert _raw_components(e, None, None, None, None, 0, 0, 0) == (0, 0, 0, 0)
    vc, fc, counts, bbox = sent()
    assert _raw_components(e, vc, fc, counts, bbox, nv, nf, nc) == (0, 0, 0, 0) and (vc == -7).all() and (bbox == 7.5).all()
    assert _raw_filtered(e, 1, None, None, None, 0, 0) == (0, 0, 0, 0, 0)
    assert [a.shape for a in e.mesh_components()] == [(0,), (0,), (0, 2), (0, 6)]
    Ve, Ne, Fe, ce, ke = e.extract_mesh_indexed_filtered(pkg.MESH_KEEP_LARGEST)
    assert Ve.shape == (0, 3) and Ne.shape == (0, 3) and Fe.shape == (0, 3) and (ce, ke) == (0, 0)
    e.close()


def test_scan3d_mesh_min_faces_flag(pkg, O, tmp_path):
    """Scan3D --mesh-min-faces on the synthetic directory of tests/test_gpu_indexed_mesh.py: one more file, the others byte for
    byte as without the flag; the PLY equals the filtered arrays of a context fused from the same files the CLI's way"""
    W, H, n = 160, 120, 3
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=4, step_deg=2.0)
    ds = pkg.synth.write_dataset(seq, str(tmp_path / "ds"), layout="synth")
    vs = f32(0.02)
    g = pkg.GradSdf(vs, f32(5) * vs, W, H, seq.K, capacity_log2=18)
    poses = np.loadtxt(ds + "pose.txt")
    for i in range(n):
        d = seq.depth_u16(i).astype(np.float32) * np.float32(0.001)
        R = O.quat_to_R(O.R_to_quat(O.quat_to_R(poses[i, 4:8].astype(np.float32))))
        g.update(d, R, poses[i, 1:4].astype(np.float32))
    nf_all = len(g.extract_mesh_indexed()[2])
    res = {}
    for flag in (None, "10", "largest"):
        r = str(tmp_path / ("out_%s" % flag)) + "/"
        os.makedirs(r)
        cmd = [os.path.join(HOST, "Scan3D"), "--input", ds, "--results", r, "--scan-type", "grad-sdf", "--data-type", "synth",
               "--voxel-size", "0.02", "--trunc", "5", "--width", str(W), "--height", str(H), "--hash-capacity", "18", "--save-sdf", "--sync"]
        out = subprocess.run(cmd + (["--mesh-min-faces", flag] if flag else []), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = re.findall(r"^Mesh components: (\d+), kept (\d+), faces (\d+) of (\d+)$", out.stdout, re.M)
        assert len(lines) == (1 if flag else 0)
        res[flag] = (r, [int(v) for v in lines[0]] if flag else None)
    plain = sorted(os.listdir(res[None][0]))
    assert "mesh_indexed.ply" not in plain and "gradient_sdf_mesh_final.ply" in plain
    for flag in ("10", "largest"):
        r, line = res[flag]
        assert sorted(os.listdir(r)) == sorted(plain + ["mesh_indexed_clean.ply"])
        for f in plain:
            assert open(res[None][0] + f, "rb").read() == open(r + f, "rb").read(), f
        V, N, F, head = IM.parse_indexed_ply(r + "mesh_indexed_clean.ply")
        Vg, Ng, Fg, nc, kept = g.extract_mesh_indexed_filtered(pkg.MESH_KEEP_LARGEST if flag == "largest" else int(flag))
        print("Scan3D --mesh-min-faces %s: components %d kept %d, faces %d of %d" % (flag, nc, kept, len(Fg), nf_all))
        assert line == [nc, kept, len(Fg), nf_all] and len(F) > 300
        assert _same(F, Fg) and _same(V, Vg) and _same(N, Ng)
    g.close()
    bad = subprocess.run([os.path.join(HOST, "Scan3D"), "--input", ds, "--mesh-min-faces", "0"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--mesh-min-faces" in bad.stderr


@pytest.mark.parametrize("kind", ["grad", "base"])
def test_mesh_components_selftest_binary(pkg, tmp_path, kind):
    """host/mesh_components_selftest: MapGradPixelSdf / MapPixelSdf::mesh_components and ::extract_mesh_indexed(filename, min_faces)
    through the C++ facade; its dumps and its PLY against the restatement of the map it dumps"""
    W, H, n, vs = 160, 120, 3, f32(0.02)
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=4, step_deg=2.0)
    d = tmp_path
    np.asarray(seq.K, np.float32).reshape(9).tofile(d / "K.bin")
    np.stack([seq.frame(i)[0] for i in range(n)]).astype(np.float32).tofile(d / "depth.bin")
    np.stack([pkg.synth.pose16(*seq.pose(i)) for i in range(n)]).astype(np.float32).tofile(d / "poses.bin")
    m = "largest" if kind == "base" else "10"
    out = subprocess.run([os.path.join(HOST, "mesh_components_selftest"), str(d), str(W), str(H), str(n), repr(float(vs)), "5", m]
                         + (["base"] if kind == "base" else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mesh_components_selftest: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    keys = np.fromfile(d / "map_keys.bin", np.int32).reshape(-1, 3)
    pay = np.fromfile(d / "map_payload.bin", np.float32).reshape(-1, 5)
    mesh = IM.compute(keys, pay, vs)
    ref = MC.compute(mesh["V"], mesh["F"])
    assert np.fromfile(d / "comp_v.bin", np.int32).tobytes() == ref["vertex_comp"].tobytes()
    assert np.fromfile(d / "comp_f.bin", np.int32).tobytes() == ref["face_comp"].tobytes()
    assert np.fromfile(d / "comp_counts.bin", np.int32).tobytes() == ref["counts"].tobytes()
    assert np.array_equal(np.fromfile(d / "comp_bbox.bin", np.float32).reshape(-1, 6), ref["bbox"])
    Vr, Nr, Fr, Cr, kr = MC.filter_mesh(mesh["V"], mesh["N"], mesh["F"], MC.KEEP_LARGEST if m == "largest" else int(m), ref)
    V, N, F, head = IM.parse_indexed_ply(str(d / "mesh_indexed_clean.ply"))
    assert "Mesh components: %d, kept %d, faces %d of %d" % (Cr, kr, len(Fr), len(mesh["F"])) in out.stdout
    assert len(F) > 300 and _same(F, Fr) and _same(V, Vr) and np.abs(N - Nr).max() <= 1e-4
    table = np.loadtxt(d / "components.txt", ndmin=2)
    assert np.array_equal(table[:, :3].astype(np.int64), np.column_stack([np.arange(Cr), ref["counts"]]))
    assert np.array_equal(table[:, 3:].astype(np.float32), ref["bbox"])
