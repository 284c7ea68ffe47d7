"""The coloured sub-voxel mesh (gsdf_color_mesh, host/HrLayeredMarchingCubes.h) without a GPU: the C-ABI exports the entry, the
C++ facade header compiles, and the numpy restatement of HrLayeredMarchingCubes::computeIsoSurface (tests/hr_mesh_ref.py) gives
the known answers of the sweep bounds, zeroWeights, voxelToWorld, setVoxel's bytes and getColor on hand-made snapshots."""
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hr_mesh_ref as HR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32
VS = f32(0.02)


def block(lo=(0, 0, 0), n=3, axis=2, cut=2.3, colour=(0.5, 0.5, 0.5), weight=10.0, drop=()):
    """a snapshot (keys, rows) of an n x n x n coarse block with minimum `lo`, cut by the plane through fine coordinate `cut`
    of `axis`: d[i] is the signed distance of the fine cell in the reference's mesh coordinates (voxelToWorld: fine cell i sits
    at (min + i / 2) vs).  colour: one (r, g, b) for all cells, or a function of the fine coordinate along `axis`."""
    g = np.arange(n)
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    rel = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)                    # (z, y, x) order
    rel = np.array([r for r in rel if tuple(r) not in set(map(tuple, drop))])
    keys = (rel + np.asarray(lo)).astype(np.int32)
    rows = np.zeros((len(keys), 37), np.float32)
    rows[:, 1] = weight
    rows[:, 2 + axis] = 1
    for i in range(8):
        fine = 2 * rel[:, axis] + ((i >> axis) & 1)
        rows[:, 5 + i] = ((fine - cut) * 0.5 * float(VS)).astype(np.float32)
        for ch in range(3):
            rows[:, 13 + 8 * ch + i] = [colour(int(f))[ch] for f in fine] if callable(colour) else colour[ch]
    rows[:, 0] = rows[:, 5:13].mean(1)
    return keys, rows


def anchors(tris, lo):
    """fine anchor (x, y, z) of the cube a triangle of a flat sheet came from: the floor of its least coordinates"""
    fine = (tris.astype(np.float64) / float(VS) - np.asarray(lo)) * 2
    return np.floor(fine.min(1) + 1e-4).astype(int)


def test_abi_exports_the_mesh_entry(pkg):
    so = os.path.join(ROOT, "gradient-sdf_amd", "csrc", "libgsdf.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    assert re.search(r"\bT gsdf_color_mesh\b", out)
    assert re.search(r"\bint gsdf_color_mesh\(gsdf_ctx\* c, float iso, float\* triangles_out", hdr)
    assert "gsdf_color_mesh" in pkg.binding.ABI_SYMBOLS
    assert callable(pkg.GradSdf.color_mesh)


def test_hr_mesh_header_compiles(tmp_path):
    src = tmp_path / "hr.cpp"
    src.write_text('#include "HrLayeredMarchingCubes.h"\n'
                   'bool f(MapGradPixelSdf* m) { HrLayeredMarchingCubes a(0.02f), b(Vec3f(0.02f, 0.02f, 0.02f));\n'
                   '  return a.computeIsoSurface(m) && b.computeIsoSurface(m, 0.003f) && a.savePly("x.ply") && extractMesh(m, "x"); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", HOST, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_one_coarse_voxel_gives_no_triangles():
    keys, rows = block(n=1, cut=0.5)                                           # dim = 2: the sweep x < dim - 2 is empty
    tris, rgb = HR.compute(keys, rows, VS)
    assert tris.shape == (0, 3, 3) and rgb.shape == (0, 3, 3)
    assert HR.compute(keys[:0], rows[:0], VS)[0].shape == (0, 3, 3)


def test_plane_block_is_a_flat_sheet_that_stops_at_dim_minus_2():
    lo = (-4, 7, 50)
    keys, rows = block(lo=lo, cut=2.3)
    tris, rgb = HR.compute(keys, rows, VS)
    # dim = 6: anchors 0..3 per axis; the plane at fine z = 2.3 cuts the cubes anchored at z = 2: 4 x 4 of them, 2 triangles each
    # (all 5 x 5 cubes anchored at 0..4 have their 8 cells in the map: the sweep's bound drops the last row and column)
    assert len(tris) == 2 * 16
    a = anchors(tris, lo)
    assert np.array_equal(a[::2], a[1::2]) and np.all(a[:, 2] == 2)
    assert [tuple(v) for v in a[::2, :2]] == [(x, y) for y in range(4) for x in range(4)]     # y outer, x inner
    z0 = (lo[2] + 0.5 * 2.3) * float(VS)                                       # voxelToWorld: (min + i / 2) vs
    assert np.abs(tris[:, :, 2].astype(np.float64) - z0).max() < 1e-6
    xy = tris[:, :, :2].reshape(-1, 2).astype(np.float64)
    assert np.allclose(xy.min(0), [lo[0] * float(VS), lo[1] * float(VS)], atol=1e-6)          # sub-voxel 0 on the voxel centre
    assert np.allclose(xy.max(0), [(lo[0] + 2) * float(VS), (lo[1] + 2) * float(VS)], atol=1e-6)
    assert np.all(rgb == 127)                                                  # (uchar)(0.5f * 255) = 127 both ways


def test_removing_a_voxel_removes_the_cubes_that_touch_it():
    lo = (0, 0, 0)
    full = HR.compute(*block(lo=lo, cut=2.3), VS)[0]
    keys, rows = block(lo=lo, cut=2.3, drop=[(1, 1, 1)])
    tris = HR.compute(keys, rows, VS)[0]
    a = anchors(full, lo)
    # the voxel holds fine cells 2..3 per axis; a cube anchored at a spans a..a+1: it touches the voxel iff a in 1..3 on every axis
    touch = np.all((a >= 1) & (a <= 3), axis=1)
    assert touch.sum() == 2 * 9 and len(tris) == 2 * 7
    assert np.array_equal(tris, full[~touch])
    # a voxel of weight 0 is as good as missing (computeLutIndex :692-699)
    keys, rows = block(lo=lo, cut=2.3)
    rows[np.all(keys == (1, 1, 1), axis=1), 1] = 0
    assert np.array_equal(HR.compute(keys, rows, VS)[0], tris)


def test_constant_colour_comes_back_through_two_truncations():
    # (evaluated for all 256 bytes: in float the round trip b / 255.f * 255.f never falls below b, so the byte survives)
    cols = (0.2275, 0.6, 1.0)
    keys, rows = block(colour=cols)
    tris, rgb = HR.compute(keys, rows, VS)
    want = []
    for c in cols:
        b = np.uint8(f32(c) * f32(255))
        want.append(np.uint8(f32(b) / f32(255) * f32(255)))
    assert len(rgb) and np.all(rgb == np.array(want, np.uint8))
    assert want == [58, 153, 255]


# Edge 2 of a cube runs from cell (0,0,0) to cell (0,1,0) for getVertex (:451) and from (0,1,0) to (0,0,0) for getColor (:458).
# A plane across y with the cut at fine y = 2.3 has mu = 0.3 in getVertex's order and 0.7 in getColor's.  The byte pairs below were
# found by evaluating both orders for all 256 x 256 pairs at these two distances and keeping pairs whose results differ.
EDGE2_LOW, EDGE2_HIGH = (14, 28, 102), (4, 8, 32)


def _edge2_case():
    def colour(fine_y):
        src = EDGE2_LOW if fine_y <= 2 else EDGE2_HIGH
        return tuple((b + 0.5) / 255.0 for b in src)                           # (uchar)(c * 255) = b
    return block(axis=1, cut=2.3, colour=colour)


def _scalar_interp(t0, t1, c0, c1, iso=f32(0)):
    """interpolate :723-743 for one colour channel given as bytes, then getColor's * 255 and truncation"""
    c0, c1 = f32(c0) / f32(255), f32(c1) / f32(255)
    if abs(float(iso - t0)) < 1e-7:
        v = c0
    elif abs(float(iso - t1)) < 1e-7:
        v = c1
    elif abs(float(t0 - t1)) < 1e-7:
        v = c0
    else:
        mu = min(max(float(f32(iso - t0) / f32(t1 - t0)), 0.0), 1.0)
        v = f32(float(c0) + mu * float(f32(c1 - c0)))
    return int(f32(v * f32(255)))


def test_edge_2_colour_is_interpolated_in_the_order_of_the_getcolor_call():
    keys, rows = _edge2_case()
    tris, rgb = HR.compute(keys, rows, VS)
    t_lo, t_hi = f32((2 - 2.3) * 0.5 * float(VS)), f32((3 - 2.3) * 0.5 * float(VS))        # cells at fine y = 2 and 3
    as_called = [_scalar_interp(t_hi, t_lo, h, l) for l, h in zip(EDGE2_LOW, EDGE2_HIGH)]  # (x, y + 1, z) first
    as_vertex = [_scalar_interp(t_lo, t_hi, l, h) for l, h in zip(EDGE2_LOW, EDGE2_HIGH)]
    assert all(a != b for a, b in zip(as_called, as_vertex)), (as_called, as_vertex)
    # the first cube of the sweep is (0, 2, 0), corners with dy = 1 above the plane: index 1 + 8 + 16 + 128
    edges = HR.TRI[153][:6]
    assert 2 in edges
    first = rgb[:2].reshape(6, 3)
    assert np.all(anchors(tris[:2], (0, 0, 0)) == (0, 2, 0))
    assert list(first[list(edges).index(2)]) == as_called
    assert np.all(rgb.reshape(-1, 3) == np.array(as_called, np.uint8))         # every y edge's getColor call names y + 1 first


def test_nan_colour_gives_zero():
    keys, rows = block(colour=(np.nan, np.nan, np.nan))
    tris, rgb = HR.compute(keys, rows, VS)
    assert len(tris) == 32 and np.all(rgb == 0)
    assert np.array_equal(HR.to_byte(np.array([np.nan, 0.0, 254.99, 255.0], f32)), np.array([0, 0, 254, 255], np.uint8))


def test_iso_value_moves_the_sheet():
    keys, rows = block(cut=2.3)
    z = HR.compute(keys, rows, VS, iso=0.003)[0][:, :, 2].astype(np.float64)
    assert np.abs(z - (0.5 * 2.3 * float(VS) + 0.003)).max() < 1e-6


def test_ply_text_has_the_header_and_rows():
    keys, rows = block(colour=(0.2275, 0.6, 1.0))
    tris, rgb = HR.compute(keys, rows, VS)
    lines = HR.ply_text(tris[:2], rgb[:2]).splitlines()
    assert lines[:3] == ["ply", "format ascii 1.0", "element vertex 6"]
    assert lines[6:12] == ["property uchar red", "property uchar green", "property uchar blue", "element face 2",
                           "property list uchar int vertex_indices", "end_header"]
    p = tris[0, 0]
    assert lines[12] == "%g %g %g 58 153 255" % (float(p[0]), float(p[1]), float(p[2]))
    assert lines[18:] == ["3 0 1 2", "3 3 4 5"]
