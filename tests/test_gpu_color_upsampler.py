"""ColorUpsampler on the GPU (gsdf_color_compute / _export / _cloud, host/ColorUpsampler.h) against the numpy restatement
(tests/color_upsampler_ref.py) on the exported table, vis_ vectors and keyframe images: parity bit for bit (NaN pattern
included), the pose / image / keyframe arguments, the snapshot semantics, the cloud and its PLY, and the error contract."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import color_upsampler_ref as CU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
f32 = np.float32
pytestmark = pytest.mark.gpu


def _scene(pkg, n_frames=6, n_kf=6, W=160, H=120, vs=0.02, trunc=5, cap=20, ba_it=2):
    """fuse with vis_ on at the true poses, PhotoBA from perturbed key poses (main_photo_ba.cpp:237-306)"""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n_frames, seed=0, noise=False)
    vs = f32(vs)
    T = f32(trunc) * vs
    frames = [seq.frame(i) for i in range(n_frames)]
    kf = np.linspace(0, n_frames - 1, n_kf).astype(np.int32)
    imgs = np.stack([pkg.synth.render_color_bgr(seq, int(i)) for i in kf]).astype(np.float32)
    P = np.stack([pkg.synth.pose16(*seq.pose(int(i))) for i in kf]).astype(np.float32)
    Pp = P.copy()
    rng = np.random.default_rng(0)
    Pp[1:, :3, 3] += (0.004 * rng.standard_normal((len(kf) - 1, 3))).astype(np.float32)
    g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=cap)
    g.enable_vis(max(64, n_frames))
    for f in frames:
        g.update(*f)
    g.ba_setup(imgs, Pp, kf)
    if ba_it:
        g.ba_optimize(ba_it)
    return seq, vs, T, frames, g, imgs, P, Pp, kf


def _same(a, b):
    """bit for bit, NaN pattern included (a NaN's sign and payload are not compared)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _restate(g, seq, vs, imgs, poses, kf, sample=None, seed=0):
    keys, pay = g.export(sorted=True)
    _, vis = g.export_vis()
    sel = CU.select(keys, pay, vs)
    pick = sel
    if sample is not None and sample < len(sel):
        pick = np.sort(np.random.default_rng(seed).choice(len(sel), sample, replace=False))
        pick = sel[pick]
    _, rows, counts = CU.compute(keys[pick], pay[pick], vis[pick], imgs, poses, kf, np.asarray(seq.K, np.float32), vs)
    # compute() selects again: every picked voxel passes the gate, so its rows follow `pick`
    assert len(rows) == len(pick)
    return keys[sel], keys[pick], rows, counts, vis[pick], np.searchsorted(sel, pick)


def test_gpu_color_parity_every_voxel_small_scene(pkg):
    seq, vs, T, frames, g, imgs, P, Pp, kf = _scene(pkg)
    nv = g.color_compute(len(kf), imgs, Pp, kf)                               # the reference's flow: pre-BA key poses
    k_all, k_pick, rows, counts, vis, _ = _restate(g, seq, vs, imgs, Pp, kf)
    kg, rg = g.color_export()
    assert nv == len(kg) == len(k_all) > 1000 and np.array_equal(kg, k_all)
    assert _same(rg, rows)
    assert np.isnan(rows[:, 13]).any() and not np.isnan(rows[:, 13]).all()    # both kinds occur
    assert g.color_counters() == (len(kg), int(counts.sum()))
    g.close()


def test_gpu_color_parity_c5_sample(pkg):
    """C5 as configured (tools/color_upsample.py): 150 frames fused at 640x480, 1 cm, 50 keyframes, two BA iterations, colours
    from the BA's images (NULL) with the pre-BA poses; the key set whole, d / r / g / b on a seeded sample of 10^5 voxels"""
    seq, vs, T, frames, g, imgs, P, Pp, kf = _scene(pkg, n_frames=150, n_kf=50, W=640, H=480, vs=0.01, trunc=10, cap=22)
    nv = g.color_compute(len(kf), None, Pp, kf)
    k_all, k_pick, rows, counts, vis, at = _restate(g, seq, vs, imgs, Pp, kf, sample=100000, seed=1)
    kg, rg = g.color_export()
    assert nv == len(kg) and np.array_equal(kg, k_all) and len(k_pick) == 100000
    assert np.array_equal(kg[at], k_pick) and _same(rg[at], rows)
    g.close()


def test_gpu_color_arguments(pkg):
    seq, vs, T, frames, g, imgs, P, Pp, kf = _scene(pkg)
    n = len(kf)
    g.color_compute(n, imgs, Pp, kf)
    ref = g.color_export()[1]
    g.color_compute(n, None, Pp, kf)                                          # NULL images: gsdf_ba_setup's
    assert _same(g.color_export()[1], ref)
    g.color_compute(n, imgs, Pp, None)                                        # NULL frame_idx: gsdf_ba_setup's
    assert _same(g.color_export()[1], ref)
    g.color_compute(n, imgs, None, kf)                                        # NULL poses: the BA's current ones
    cur = g.color_export()[1]
    g.color_compute(n, imgs, g.ba_poses(), kf)
    assert _same(g.color_export()[1], cur)
    assert not _same(cur, ref)                                                # the BA moved the poses
    g.color_compute()                                                         # everything PhotoBA's
    assert _same(g.color_export()[1], cur)
    g.close()


def test_gpu_color_leaves_the_table_and_is_a_snapshot(pkg):
    seq, vs, T, frames, g, imgs, P, Pp, kf = _scene(pkg, n_frames=8, n_kf=6)
    k0, p0 = g.export(sorted=True)
    _, v0 = g.export_vis()
    g.color_compute(len(kf), imgs, Pp, kf)
    k1, p1 = g.export(sorted=True)
    _, v1 = g.export_vis()
    assert np.array_equal(k0, k1) and p0.tobytes() == p1.tobytes() and np.array_equal(v0, v1)
    ka, ra = g.color_export()
    ca = g.color_cloud()
    g.update(*seq.frame(3))                                                   # a later fusion, a BA step, a doubling
    g.ba_solve_dist()
    g.grow(21)
    kb, rb = g.color_export()
    assert np.array_equal(ka, kb) and _same(ra, rb) and _same(g.color_cloud(), ca)
    assert not np.array_equal(g.export(sorted=True)[1], p1)
    g.reset()
    for f in (g.color_export, g.color_cloud):
        with pytest.raises(pkg.binding.GsdfError) as e:
            f()
        assert e.value.code == pkg.binding.ERR_INVALID
    g.close()


def test_gpu_color_cloud_matches_restatement(pkg):
    seq, vs, T, frames, g, imgs, P, Pp, kf = _scene(pkg)
    g.color_compute(len(kf), imgs, Pp, kf)
    k_all, k_pick, rows, counts, vis, _ = _restate(g, seq, vs, imgs, Pp, kf)
    ref = CU.cloud(k_pick, rows, vis, kf, vs)
    got = g.color_cloud()
    assert len(ref) > 1000 and _same(got, ref)
    assert CU.ply_text(got) == CU.ply_text(ref)
    g.close()


def test_gpu_color_facade_ply_matches_restatement(pkg, tmp_path):
    """host/color_selftest: MapGradPixelSdf::update, PhotometricOptimizer::optimize, ColorUpsampler with the pre-BA poses,
    computeColor, extractCloud -- its PLY text against one written from the restatement of the map it leaves behind"""
    n, W, H, vsf, trunc = 6, 160, 120, 0.02, 5
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0, noise=False)
    frames = [seq.frame(i) for i in range(n)]
    imgs = np.stack([pkg.synth.render_color_bgr(seq, i) for i in range(n)]).astype(np.float32)
    P = np.stack([pkg.synth.pose16(*seq.pose(i)) for i in range(n)]).astype(np.float32)
    Pp = P.copy()
    Pp[1:, :3, 3] += (0.004 * np.random.default_rng(0).standard_normal((n - 1, 3))).astype(np.float32)
    d = tmp_path
    np.asarray(seq.K, np.float32).reshape(9).tofile(d / "K.bin")
    np.stack([f[0] for f in frames]).astype(np.float32).tofile(d / "depth.bin")
    imgs.tofile(d / "images.bin")
    P.tofile(d / "poses_true.bin")
    Pp.tofile(d / "poses_start.bin")
    out = subprocess.run([os.path.join(HOST, "color_selftest"), str(d), str(W), str(H), str(n), repr(vsf), str(trunc), "2"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "color_selftest: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    keys = np.fromfile(d / "state_keys.bin", np.int32).reshape(-1, 3)
    pay = np.fromfile(d / "state_payload.bin", np.float32).reshape(-1, 5)
    vis = np.fromfile(d / "state_vis.bin", np.uint32).reshape(-1, 2)
    vs = f32(vsf)
    sel, rows, counts = CU.compute(keys, pay, vis, imgs, Pp, np.arange(n), np.asarray(seq.K, np.float32), vs)
    words = dict(zip(out.stdout.split()[0::2], out.stdout.split()[1::2]))
    assert int(words["hr_voxels"]) == len(sel) and int(words["frames"]) == n
    ref = CU.cloud(keys[sel], rows, vis[sel], np.arange(n), vs)
    assert len(ref) > 1000
    assert (d / "cloud.ply").read_text() == CU.ply_text(ref)


def test_gpu_color_contract(pkg):
    E = pkg.binding.GsdfError
    INVALID = pkg.binding.ERR_INVALID
    seq = pkg.synth.Sequence("tum", 160, 120, n_frames=2, seed=0, noise=False)
    vs = f32(0.02)
    T = f32(5) * vs
    imgs = np.stack([pkg.synth.render_color_bgr(seq, i) for i in range(2)]).astype(np.float32)
    P = np.stack([pkg.synth.pose16(*seq.pose(i)) for i in range(2)]).astype(np.float32)
    kf = np.arange(2)

    def invalid(f, *a):
        with pytest.raises(E) as e:
            f(*a)
        assert e.value.code == INVALID

    gb = pkg.GradSdf(vs, T, 160, 120, seq.K, capacity_log2=18, map_type=pkg.MAP_BASE)
    gb.enable_vis(64)
    gb.update(*seq.frame(0))
    invalid(gb.color_compute, 2, imgs, P, kf)                                 # base-sdf context
    gb.close()
    g = pkg.GradSdf(vs, T, 160, 120, seq.K, capacity_log2=18)
    g.update(*seq.frame(0))
    invalid(g.color_compute, 2, imgs, P, kf)                                  # no gsdf_enable_vis
    g.enable_vis(64)
    g.update(*seq.frame(0))
    invalid(g.color_export)                                                   # before a compute
    invalid(g.color_cloud)
    invalid(g.color_compute, 2, None, P, kf)                                  # NULL images without gsdf_ba_setup
    invalid(g.color_compute, 2, imgs, None, kf)
    L = g.L
    for n in (0, 65):                                                         # 1..64 keyframes
        assert L.gsdf_color_compute(g.h, n, None, None, None, None) == INVALID
    big = np.zeros((65, 16), np.float32)
    assert L.gsdf_color_compute(g.h, 65, pkg.binding._fp(np.zeros((65, 120, 160, 3), np.float32)), pkg.binding._fp(big),
                                np.zeros(65, np.int32).ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_int)),
                                None) == INVALID
    nv = g.color_compute(2, imgs, P, kf)
    assert nv > 0 and len(g.color_export()[0]) == nv
    g.close()
