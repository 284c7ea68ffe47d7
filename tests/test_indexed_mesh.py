"""The indexed iso-surface mesh (gsdf_extract_mesh_indexed) without a GPU: the C-ABI exports the entry; the numpy restatement
(tests/indexed_mesh_ref.py) gives the oracle's triangle soup, a weld whose cost in float spacings is measured and printed, and a
closed 2-manifold on an analytic sphere; the binary PLY writer round-trips."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indexed_mesh_ref as IM  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32
weld_cost, no_guarded_edges = IM.weld_cost, IM.no_guarded_edges


def _oracle_map(O, name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    depth = z["depth_u16"].astype(np.float32) * np.float32(z["unit"])
    o = O.Oracle(z["voxel_size"], z["trunc_dist"], int(z["W"]), int(z["H"]), z["K"])
    for i in range(depth.shape[0] - 1):                                        # the fixture's map: all frames but the last
        o.update(depth[i], z["R"][i], z["t"][i])
    return o, f32(z["voxel_size"])


@pytest.fixture(scope="module", params=["spheres_64x48", "spheres_160x120", "tum_128x96"])
def oracle_case(O, request):
    o, vs = _oracle_map(O, request.param)
    keys, pay = o.export()
    return request.param, vs, pay, o.extract_mesh(), IM.compute(keys, pay, vs)


def test_abi_exports_the_indexed_mesh_entry(pkg):
    so = os.path.join(ROOT, "gradient-sdf_amd", "csrc", "libgsdf.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    assert re.search(r"\bT gsdf_extract_mesh_indexed\b", out)
    assert re.search(r"\bint gsdf_extract_mesh_indexed\(gsdf_ctx\* c, float iso, const int8_t tri_table\[256 \* 16\],", hdr)
    assert "gsdf_extract_mesh_indexed" in pkg.binding.ABI_SYMBOLS
    assert callable(pkg.GradSdf.extract_mesh_indexed)


def test_restatement_soup_equals_the_oracle(oracle_case):
    name, vs, pay, soup, r = oracle_case
    print(name, "triangles", len(soup), "restatement", len(r["soup"]))
    assert r["soup"].shape == soup.shape and len(soup) > 0
    assert np.array_equal(r["soup"].view(np.uint32), soup.view(np.uint32))


def test_weld_cost_in_float_spacings(oracle_case):
    name, vs, pay, soup, r = oracle_case
    V, N, F = r["V"], r["N"], r["F"]
    cost = weld_cost(V, F, soup, vs)
    moved = int((V[F] != soup).any(axis=2).sum())
    print("%s: faces %d vertices %d (%.3f per face), corners moved by the weld %d of %d, largest move %.3f float spacings"
          % (name, len(F), len(V), len(V) / len(F), moved, F.size, cost))
    assert no_guarded_edges(pay)                                               # the figure is a measurement: printed, not bounded here
    assert F.shape == (len(soup), 3) and F.min() == 0 and len(np.unique(F)) == len(V) == F.max() + 1
    assert (F[:, 0] != F[:, 1]).all() and (F[:, 0] != F[:, 2]).all() and (F[:, 1] != F[:, 2]).all()
    nn = np.linalg.norm(N.astype(np.float64), axis=1)
    assert ((np.abs(nn - 1) < 1e-6) | (nn == 0)).all()
    # ids are the ranks of the edge keys, the position is the first corner's
    ek = r["edge_keys"].reshape(-1)
    order = np.argsort(ek, kind="stable")
    first = order[np.concatenate([[True], ek[order][1:] != ek[order][:-1]])]
    assert np.array_equal(F.reshape(-1)[first], np.arange(len(V))) and np.array_equal(V, soup.reshape(-1, 3)[first])


def test_analytic_sphere_is_a_closed_two_manifold():
    vs, radius, centre = f32(0.02), 6.3, (0.37, -0.21, 0.13)
    keys, pay = IM.sphere_map(radius, centre, vs, band=3.0)
    assert keys.min() < -4 and keys.max() > 4                                  # negative and positive, several 4 x 4 x 4 blocks
    assert len(np.unique(keys >> 2, axis=0)) > 20
    r = IM.compute(keys, pay, vs)
    V, N, F = r["V"], r["N"], r["F"]
    # closedness is a fair demand only if the soup dropped no degenerate triangle
    assert r["table_triangles"] == len(F), "a degenerate triangle was dropped: move the centre"
    nv, ne, nf, bad = IM.manifold_counts(F)
    print("sphere: vertices %d edges %d faces %d, edges not in two faces %d" % (nv, ne, nf, bad))
    assert bad == 0 and nv == len(V) and nv - ne + nf == 2
    c = np.asarray(centre, np.float64) * float(vs)
    rho = np.linalg.norm(V.astype(np.float64) - c, axis=1)
    err = np.abs(rho - radius * float(vs)).max() / float(vs)
    print("sphere: largest | |v - c| - r | = %.4f vs" % err)
    assert err <= 0.05                                                         # linear interpolation of an exact distance: vs^2 / 8 r = 0.02 vs
    # the stored gradient is radial: so is the blend of two of them, to the angle between neighbouring voxels' directions
    radial = (V.astype(np.float64) - c) / rho[:, None]
    assert np.abs(N.astype(np.float64) + radial).max() < 0.02
    assert no_guarded_edges(pay)


def test_weld_joins_opposite_walks_of_one_edge():
    """two cubes side by side in x share the y edge at their common face: the left cube walks it as its edge 0 (-y), the right one
    as its edge 2 (+y).  The two corners must become one vertex although their position bits may differ."""
    xs, ys, zs = np.meshgrid(np.arange(3), np.arange(2), np.arange(2), indexing="ij")
    keys = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1) + np.array([-1, 5, 2])
    pay = np.zeros((len(keys), 5), f32)
    pay[:, 0] = ((keys[:, 1] - 5) - 0.3371).astype(f32) * f32(0.02)            # the plane y = 5.3371 voxels
    pay[:, 2] = 1
    pay[:, 4] = 2
    r = IM.compute(keys, pay, 0.02)
    assert len(r["F"]) == 4 and len(r["V"]) == 6                               # two quads sharing an edge: 8 - 2 vertices
    assert np.allclose(r["N"], [0, -1, 0])                                     # normal = -g^
    axis = r["edge_keys"] & 3
    assert (axis == 1).all()
    nv, ne, nf, bad = IM.manifold_counts(r["F"])
    assert (nv, ne, nf) == (6, 9, 4)


def test_zero_and_nan_gradients_give_a_zero_normal():
    xs, ys, zs = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    keys = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1)
    pay = np.zeros((8, 5), f32)
    pay[:, 0] = (keys[:, 2] - 0.4).astype(f32) * f32(0.02)
    pay[:, 4] = 1
    r = IM.compute(keys, pay, 0.02)
    assert len(r["F"]) == 2 and len(r["V"]) == 4 and np.all(r["N"] == 0)       # no gradient at all
    pay[:, 3] = 1
    pay[keys[:, 0] == 0, 1] = np.nan
    r = IM.compute(keys, pay, 0.02)
    lone = np.isclose(r["V"][:, 0], 0.0)
    assert lone.sum() == 2 and np.all(r["N"][lone] == 0) and np.allclose(r["N"][~lone], [0, 0, -1])


def test_iso_value_and_caller_table():
    keys, pay = IM.sphere_map(4.2, (0.1, 0.2, -0.3), 0.02, band=2.5)
    a, b = IM.compute(keys, pay, 0.02), IM.compute(keys, pay, 0.02, iso=0.005)
    rho = lambda r: np.linalg.norm(r["V"].astype(np.float64) - np.array([0.1, 0.2, -0.3]) * 0.02, axis=1).mean()   # noqa: E731
    assert abs((rho(b) - rho(a)) - 0.005) < 2e-4
    tt = IM.TRI.copy()
    tt[:, 3:] = -1                                                             # a caller's table: the first triangle of every case
    c = IM.compute(keys, pay, 0.02, tri_table=tt)
    assert 0 < len(c["F"]) < len(a["F"]) and len(np.unique(c["F"])) == len(c["V"])


def test_binary_ply_round_trip(tmp_path):
    """host/indexed_mesh_selftest --ply-only: MarchingCubes::saveIndexedPly without a device"""
    ply = tmp_path / "tet.ply"
    out = subprocess.run([os.path.join(HOST, "indexed_mesh_selftest"), "--ply-only", str(ply)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "indexed_mesh_selftest: OK" in out.stdout, out.stdout + out.stderr
    assert sorted(os.listdir(tmp_path)) == ["tet.ply"]                         # the refused inputs left no file
    V, N, F, head = IM.parse_indexed_ply(str(ply))
    assert head == ["ply", "format binary_little_endian 1.0", "element vertex 4", "property float x", "property float y",
                    "property float z", "property float nx", "property float ny", "property float nz", "element face 4",
                    "property list uchar int vertex_indices", "end_header"]
    assert np.array_equal(V, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], f32))
    assert np.array_equal(N[:3], np.array([[-.5, -.5, -.5], [1, 0, 0], [0, 1, 0]], f32)) and np.signbit(N[3, 2])
    assert np.array_equal(F, np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.int32))
    assert IM.manifold_counts(F) == (4, 6, 4, 0)
