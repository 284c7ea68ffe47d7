"""ColorUpsampler (ps_optimizer/ColorUpsampler.h/.cpp, gsdf_color_*) without a GPU: the C-ABI exports the colour entries, the C++
facade header compiles, and the numpy restatement (tests/color_upsampler_ref.py) gives the known answers of SdfVoxelHr,
computeColor, setAlbedo and extractCloud on small hand-made maps."""
import os
import re
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_upsampler_ref as CU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32

W, H = 64, 48
K = np.array([[100, 0, 32], [0, 100, 24], [0, 0, 1]], np.float32)
VS = f32(0.02)
PLANE_Z = f32(1.003)                       # between voxel centres: some sub-voxels lie within vs / 4 of it


def test_abi_exports_color_entries(pkg):
    so = os.path.join(ROOT, "gradient-sdf_amd", "csrc", "libgsdf.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    for sym in ("gsdf_color_compute", "gsdf_color_export", "gsdf_color_cloud", "gsdf_color_counters"):
        assert re.search(r"\bT %s\b" % sym, out), sym
        assert re.search(r"\bint %s\(gsdf_ctx\* c," % sym, hdr), sym
        assert sym in pkg.binding.ABI_SYMBOLS
    for meth in ("color_compute", "color_export", "color_cloud"):
        assert callable(getattr(pkg.GradSdf, meth))


def test_color_upsampler_header_compiles(tmp_path):
    src = tmp_path / "cu.cpp"
    src.write_text('#include "ColorUpsampler.h"\n'
                   'size_t f(ColorUpsampler* u) { u->computeColor(); u->extractCloud("x"); return u->getFrameNumber() + u->getVoxelNumber(); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", HOST, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "extractMesh" not in open(os.path.join(HOST, "ColorUpsampler.h")).read().replace("extractMesh (HrLayered", "")


def _plane_map(scale=f32(7), weight=f32(10)):
    """voxels around the plane z = 1.003 m seen head-on by an identity camera: dist = z - 1.003, grad = scale * (0, 0, 1)"""
    xs, ys, zs = np.meshgrid(np.arange(-3, 4), np.arange(-3, 4), np.arange(47, 54), indexing="ij")
    keys = np.stack([xs.ravel(), ys.ravel(), zs.ravel()], 1).astype(np.int32)
    keys = keys[np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))]             # (z, y, x) order
    pay = np.zeros((len(keys), 5), np.float32)
    pay[:, 0] = VS * keys[:, 2].astype(np.float32) - PLANE_Z
    pay[:, 3] = scale
    pay[:, 4] = weight
    vis = np.full((len(keys), 2), 0xFFFFFFFF, np.uint32)
    return keys, pay, vis


def _const_images(*bgr):
    return np.stack([np.broadcast_to(np.array(c, np.float32), (H, W, 3)) for c in bgr]).copy()


def _poses(*ts):
    P = np.tile(np.eye(4, dtype=np.float32), (len(ts), 1, 1))
    for i, t in enumerate(ts):
        P[i, :3, 3] = t
    return P


def test_hr_distances_of_a_plane_are_the_analytic_ones():
    keys, pay, vis = _plane_map()
    sel = CU.select(keys, pay, VS)
    g, d = CU.hr_voxels(pay[sel], VS)
    centres = CU.subvoxel_centres(keys[sel], VS)
    assert np.array_equal(g, np.tile(np.array([0, 0, 1], np.float32), (len(sel), 1)))
    analytic = centres[:, :, 2].astype(np.float64) - float(PLANE_Z)                     # signed distance of each sub-voxel centre
    assert np.abs(d - analytic).max() < 1e-6
    assert np.all(np.abs(pay[sel, 0]) < CU.gate(VS)) and len(sel) < len(keys)


def test_constant_keyframes_give_their_colour():
    keys, pay, vis = _plane_map()
    bgr = (0.2, 0.5, 0.7)
    imgs = _const_images(bgr, bgr, bgr)
    sel, rows, counts = CU.compute(keys, pay, vis, imgs, _poses((0, 0, 0), (0.01, 0, 0), (0, -0.01, 0.02)), [0, 1, 2], K, VS)
    assert np.all(counts == 3)
    for ch, col in ((13, bgr[2]), (21, bgr[1]), (29, bgr[0])):
        c = rows[:, ch:ch + 8]
        assert np.all(np.abs(c - f32(col)) <= np.spacing(f32(col)))           # within 1 ulp


def test_one_subvoxel_outside_drops_the_keyframe_for_all_eight():
    keys, pay, vis = _plane_map()
    # the column x = -16 projects to m = fx x / z + cx = 0 at z = 1: its sub-voxels at x -+ vs/4 fall at m = -0.5 and +0.5
    edge = keys.copy()
    edge[:, 0] -= 16
    imgs = _const_images((0.1, 0.1, 0.1), (0.9, 0.9, 0.9))
    P = _poses((0, 0, 0), (-0.32, 0, 0))                                      # keyframe 1 looks at the column head-on
    sel, rows, counts = CU.compute(edge, pay, vis, imgs, P, [0, 1], K, VS)
    on_border = edge[sel, 0] == -16
    assert on_border.any() and np.all(counts[on_border] == 1)
    c = rows[on_border, 13:37]                                                # keyframe 0 counted for none of the 8
    assert np.all(np.abs(c - f32(0.9)) <= np.spacing(f32(0.9)))
    inside = edge[sel, 0] == -14
    assert np.all(counts[inside] == 2)


def test_unseen_voxel_is_nan_and_leaves_the_cloud():
    keys, pay, vis = _plane_map()
    vis[::2] = 0
    imgs = _const_images((0.3, 0.4, 0.5), (0.3, 0.4, 0.5))
    idx = [0, 1]
    sel, rows, counts = CU.compute(keys, pay, vis, imgs, _poses((0, 0, 0), (0.01, 0, 0)), idx, K, VS)
    unseen = (vis[sel, 0] == 0)
    assert unseen.any() and np.all(counts[unseen] == 0)
    assert np.all(np.isnan(rows[unseen, 13:37])) and not np.isnan(rows[~unseen, 13:37]).any()
    cl = CU.cloud(keys[sel], rows, vis[sel], idx, VS)
    seen_only = CU.cloud(keys[sel][~unseen], rows[~unseen], vis[sel][~unseen], idx, VS)
    assert len(cl) > 0 and np.array_equal(cl, seen_only)
    # every emitted point lies on the plane (dvec moves the sub-voxel centre onto it) with normal -z
    assert np.abs(cl[:, 2] - PLANE_Z).max() < 1e-6 and np.all(cl[:, 3:6] == np.array([0, 0, -1], np.float32))


def test_colours_above_one_clamp_to_one_and_below_zero_to_zero():
    keys, pay, vis = _plane_map()
    imgs = _const_images((1.5, -0.25, 0.5))
    sel, rows, counts = CU.compute(keys, pay, vis, imgs, _poses((0, 0, 0)), [0], K, VS)
    assert np.all(rows[:, 21:29] == f32(0)) and np.all(rows[:, 29:37] == f32(1))     # green -0.25, blue 1.5
    assert np.all(np.abs(rows[:, 13:21] - f32(0.5)) <= np.spacing(f32(0.5)))


def test_distance_exactly_at_the_gate_is_excluded():
    keys = np.array([[0, 0, 50], [1, 0, 50], [2, 0, 50]], np.int32)
    pay = np.zeros((3, 5), np.float32)
    pay[:, 3], pay[:, 4] = 1, 6
    gate = CU.gate(VS)
    pay[:, 0] = [gate, np.nextafter(gate, f32(0)), -gate]
    assert list(CU.select(keys, pay, VS)) == [1]
    pay[1, 4] = 0                                                             # a voxel that does not exist (w = 0)
    assert list(CU.select(keys, pay, VS)) == []


def test_cloud_weight_rule_and_ply_format():
    keys, pay, vis = _plane_map()
    pay[: len(pay) // 2, 4] = f32(4.99)                                       # weight < 5: no rows
    imgs = _const_images((0.25, 0.5, 1.0))
    sel, rows, _ = CU.compute(keys, pay, vis, imgs, _poses((0, 0, 0)), [0], K, VS)
    cl = CU.cloud(keys[sel], rows, vis[sel], [0], VS)
    heavy = CU.cloud(keys[sel][rows[:, 1] >= 5], rows[rows[:, 1] >= 5], vis[sel][rows[:, 1] >= 5], [0], VS)
    assert len(cl) > 0 and np.array_equal(cl, heavy)
    text = CU.ply_text(cl[:2])
    lines = text.splitlines()
    assert lines[:3] == ["ply", "format ascii 1.0", "element vertex 2"] and lines[12] == "end_header"
    assert lines[9:12] == ["property uchar red", "property uchar green", "property uchar blue"]
    assert lines[13].endswith(" 255 127 63")                                  # int(255.f * c): 255, 127.5 -> 127, 63.75 -> 63
