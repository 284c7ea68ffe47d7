"""The gradient-accuracy analysis (gsdf_gradient_angles / gsdf_gradient_stats) without a GPU: the C-ABI exports the entries; the
numpy restatement (tests/gradient_analysis_ref.py) is held to hand-made maps whose answers are known, to a voxel-by-voxel
second statement of the header's rules, to the percentile and threshold rules, to an analytic sphere, and gives the paper's
picture on the committed fixture: the stored gradient beats finite differences."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gradient_analysis_ref as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
VS, T = f32(0.02), f32(0.1)
FAR_Z = np.array([[0.0, 0.0, -50.0, 49.0]], f32)          # on the z axis its analytic gradient is +z exactly


def _map(keys, dist, grad=None):
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    pay = np.zeros((len(keys), 5), f32)
    pay[:, 0] = dist
    pay[:, 1:4] = (0, 0, 1) if grad is None else grad
    pay[:, 4] = 1
    order = np.lexsort((keys[:, 0], keys[:, 1], keys[:, 2]))                   # gsdf_export's sorted order
    return keys[order], pay[order]


def _by_rules(keys, pay, spheres, vs, trunc):
    """the header's rules voxel by voxel (a dictionary and python floats): the second statement the restatement is held to"""
    D = {tuple(k): float(p[0]) for k, p in zip(keys.tolist(), pay)}
    mn, mx = keys.min(0), keys.max(0)
    h, Tt = float(f32(vs)), float(f32(trunc))
    sp = np.asarray(spheres, f32).astype(np.float64)
    rows = np.empty((len(keys), 5), f32)
    for i, (k, p) in enumerate(zip(keys.tolist(), pay)):
        c = (f32(vs) * np.asarray(k, f32)).astype(np.float64)
        m = [s[3] - np.sqrt(((c - s[:3]) ** 2).sum()) for s in sp]
        g = c - sp[int(np.argmax(m)), :3]
        g = g / np.sqrt((g * g).sum()) if (g * g).sum() > 0 else g * np.nan
        est = np.zeros((4, 3))
        est[0] = p[1:4].astype(np.float64)
        for a in range(3):
            lo, hi = k[a] == mn[a], k[a] == mx[a]
            kp, km = list(k), list(k)
            kp[a] += 1
            km[a] -= 1
            d0, dp, dm = D[tuple(k)], D.get(tuple(kp), Tt), D.get(tuple(km), Tt)
            est[1, a] = 0.0 if lo and hi else ((dp - d0) / h if lo else ((d0 - dm) / h if hi else (dp - dm) / (2 * h)))
            est[2, a] = 0.0 if hi else (dp - d0) / h
            est[3, a] = 0.0 if lo else (d0 - dm) / h
        rows[i, 0] = p[0]
        for e in range(4):
            n2 = float((est[e] * est[e]).sum())
            if not (n2 > 0) or not np.isfinite(n2) or np.isnan(g).any():
                rows[i, 1 + e] = np.nan
            else:
                rows[i, 1 + e] = np.degrees(np.arccos(min(abs(float((est[e] / np.sqrt(n2) * g).sum())), 1.0)))
    return rows


def test_abi_exports_the_gradient_entries(pkg):
    so = os.path.join(ROOT, "gradient-sdf_amd", "csrc", "libgsdf.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    for name in ("gsdf_gradient_angles", "gsdf_gradient_stats"):
        assert re.search(r"\bT %s\b" % name, out)
        assert re.search(r"\bint %s\(gsdf_ctx\* c, const float\* spheres4_host, int n_spheres," % name, hdr)
        assert name in pkg.binding.ABI_SYMBOLS
    assert callable(pkg.GradSdf.gradient_angles) and callable(pkg.GradSdf.gradient_stats)


def test_single_voxel_has_only_the_stored_estimator():
    keys, pay = _map([[3, -2, 5]], 0.01, (0, 0, 2))
    rows = G.angles(keys, pay, [[0.06, -0.04, -1.0, 1.0]], VS, T)               # the centre straight below the voxel: g = +z
    assert rows[0, 0] == f32(0.01) and rows[0, 1] < 1e-5 and np.isnan(rows[0, 2:]).all()
    st = G.stats(rows, [0.02, 0.05])
    assert (st[0, :, 0] == 1).all() and (st[1:, :, 0] == 0).all() and np.isnan(st[1:, :, 1:]).all()
    assert np.array_equal(rows.view(np.uint32), _by_rules(keys, pay, [[0.06, -0.04, -1.0, 1.0]], VS, T).view(np.uint32))


def test_column_of_three_voxels():
    """1 x 1 x 3: x and y contribute 0; along z every estimator is +-z (angle 0 to the ground truth) or the zero vector (NaN)"""
    keys, pay = _map([[0, 0, 0], [0, 0, 1], [0, 0, 2]], [0.01, 0.01, 0.03])
    rows = G.angles(keys, pay, FAR_Z, VS, T)
    nan = np.isnan(rows[:, 1:])
    #                          stored central forward backward
    assert nan.tolist() == [[False, True, True, True],           # z = 0: minimal face: central = forward = d1 - d0 = 0; backward 0
                            [False, False, False, True],         # z = 1: central (d2 - d0) / 2h, forward d2 - d1, backward d1 - d0 = 0
                            [False, False, True, False]]         # z = 2: maximal face: central = backward = d2 - d1; forward 0
    assert (rows[:, 1:][~nan] < 1e-5).all()


def test_missing_neighbour_takes_trunc_dist_and_box_faces():
    """a 3 x 3 x 1 plate without its centre voxel, D = 0.01 x: the hole reads trunc_dist, the box's faces difference one-sidedly"""
    ks = [[x, y, 0] for y in range(3) for x in range(3) if (x, y) != (1, 1)]
    keys, pay = _map(ks, [0.01 * k[0] for k in ks])
    sph = [[-40.0, 0.02, 0.0, 39.0]]                                           # g = +x on the row y = 1
    rows = G.angles(keys, pay, sph, VS, T)
    at = {tuple(k): r for k, r in zip(keys.tolist(), rows)}
    h, t = float(VS), float(T)
    # (0, 1, 0): x minimal face -> central x = (T - 0) / h = forward x; backward x = 0; y interior: neighbours equal -> 0
    r = at[(0, 1, 0)]
    assert r[2] < 1e-4 and r[3] < 1e-4 and np.isnan(r[4])
    # (1, 0, 0): y minimal face, its +y neighbour is the hole: central = (0.01 x: (0.02 - 0) / 2h, (T - 0.01) / h, 0)
    v = np.array([0.02 / (2 * h), (t - 0.01) / h, 0.0])
    c = (VS * np.array([1, 0, 0], f32)).astype(np.float64)
    g = c - np.array([-40.0, float(f32(0.02)), 0.0])
    want = np.degrees(np.arccos(abs(v @ g) / np.linalg.norm(v) / np.linalg.norm(g)))
    assert abs(at[(1, 0, 0)][2] - want) < 1e-4 and want > 80
    # forward at (2, 2, 0), the box's maximal corner: 0 in x and y, z one voxel thick -> NaN; backward there is finite
    assert np.isnan(at[(2, 2, 0)][3]) and np.isfinite(at[(2, 2, 0)][4])
    assert np.allclose(rows, _by_rules(keys, pay, sph, VS, T), atol=1e-5, equal_nan=True)


def test_zero_and_nan_gradient_sums_leave_estimator_0_only():
    ks = [[x, 0, 0] for x in range(4)]
    grad = np.array([[1, 0, 0], [0, 0, 0], [np.nan, 0, 0], [np.inf, 0, 0]], f32)
    keys, pay = _map(ks, [0.0, 0.01, 0.02, 0.03], grad)
    rows = G.angles(keys, pay, [[-40.0, 0.0, 0.0, 39.0]], VS, T)
    assert np.isnan(rows[:, 1]).tolist() == [False, True, True, True]
    assert np.isfinite(rows[:, 2]).all() and (rows[:, 2] < 1e-5).all()
    st = G.stats(rows, [0.1])
    assert st[:, 0, 0].tolist() == [1, 4, 3, 3]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_the_rules_voxel_by_voxel(seed):
    """random sparse maps around the origin (negative keys, holes, one-voxel-thick boxes for seed 2)"""
    rng = np.random.default_rng(seed)
    shape = (5, 4, 1) if seed == 2 else (5, 4, 3)
    full = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3) - np.array([2, 1, 1])
    ks = full[rng.random(len(full)) < 0.7]
    keys, pay = _map(ks, (rng.random(len(ks)) * 0.2 - 0.1).astype(f32), rng.normal(size=(len(ks), 3)).astype(f32))
    sph = np.array([[0.3, 0.1, -0.2, 0.25], [-0.2, 0.0, 0.1, 0.12]], f32)
    a, b = G.angles(keys, pay, sph, VS, T), _by_rules(keys, pay, sph, VS, T)
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(a, b, atol=2e-5, equal_nan=True)
    assert np.array_equal(a[:, 0].view(np.uint32), pay[:, 0].view(np.uint32))


def test_percentiles_of_one_and_two_values():
    rows = np.array([[0.001, 10, np.nan, 30, 30], [0.002, 20, np.nan, np.nan, 50]], f32)
    st = G.stats(rows, [0.0015, 0.003])
    assert st[0, 0].tolist() == [1, 10, 10, 10, 10]                             # n = 1: every percentile is the one value
    assert st[0, 1, 0] == 2 and st[0, 1, 2] == 15 and st[0, 1, 4] == 20         # n = 2: the mean of the two; p95 the larger
    assert st[0, 1, 1] == 15 and abs(st[0, 1, 3] - np.sqrt(250.0)) < 1e-12
    assert st[1, :, 0].tolist() == [0, 0] and np.isnan(st[1, :, 1:]).all()
    assert st[2, :, 0].tolist() == [1, 1] and st[3, 1].tolist()[:3] == [2, 40, 40]
    # prctile's positions on 1..20: n p / 100 + 0.5 = 10.5 and 19.5
    r20 = np.zeros((20, 5), f32)
    r20[:, 1] = np.arange(1, 21)
    s20 = G.stats(r20, [1.0])
    assert s20[0, 0, 2] == 10.5 and s20[0, 0, 4] == 19.5


def test_threshold_is_a_strict_float_compare():
    d = f32(0.1)                                                               # 0.1f > 0.1: a double compare would differ
    rows = np.array([[d, 1, 1, 1, 1], [np.nextafter(d, f32(0)), 2, 2, 2, 2], [-d, 3, 3, 3, 3]], f32)
    st = G.stats(rows, [d])
    assert st[0, 0, 0] == 1 and st[0, 0, 1] == 2                               # |dist| == d is outside
    assert G.stats(rows, [np.nextafter(d, f32(1))])[0, 0, 0] == 3
    assert float(d) > 0.1 and G.stats(rows, [0.1])[0, 0, 0] == 1               # the threshold is taken as float32


def test_analytic_sphere():
    """dist = clamp(R - |c|), gradient sum radial, keys on both sides of 0: the stored estimator is exact to rounding, central
    differences to second order (h / R = 0.04: about 0.015 degrees) where all six neighbours exist unclamped"""
    vs, trunc = f32(0.02), f32(0.1)
    keys, pay, sphere = G.sphere_map(25.0, (0.3, -0.2, 0.1), vs, trunc, band_vox=4.0)
    assert (keys.min(0) < 0).all() and (keys.max(0) > 0).all() and len(keys) > 10000
    rows = G.angles(keys, pay, sphere, vs, trunc)
    assert np.nanmax(rows[:, 1]) < 1e-3
    have = {tuple(k) for k in keys.tolist()}
    inner = np.array([all(tuple(np.add(k, o)) in have for o in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)))
                      for k in keys.tolist()])
    print("sphere: voxels %d, with six neighbours %d, central max %.4f deg, stored max %.2e deg"
          % (len(keys), inner.sum(), rows[inner, 2].max(), np.nanmax(rows[:, 1])))
    assert inner.sum() > 5000 and (np.abs(pay[:, 0]) < trunc).all() and rows[inner, 2].max() < 0.1


def test_fixture_stored_gradient_beats_finite_differences(pkg):
    z = np.load(os.path.join(ROOT, "tests", "golden", "spheres_160x120.npz"))
    rows = G.angles(z["keys"], z["payload"], pkg.synth.make_spheres(7), z["voxel_size"], z["trunc_dist"])
    thr = G.ladder(z["trunc_dist"])
    st = G.stats(rows, thr)
    assert len(z["keys"]) == 8324 and len(thr) == 100 and thr[-1] == f32(0.1)
    held = 0
    for k in range(len(thr)):
        if st[:, k, 0].min() >= 100:
            held += 1
            assert st[0, k, 2] < st[1:, k, 2].min(), (thr[k], st[:, k, 2])
    k11, k100 = 10, 99
    print("medians at d = 0.011:", st[:, k11, 2].round(2), "at d = 0.1:", st[:, k100, 2].round(2), "thresholds held:", held)
    assert held >= 90
    assert np.allclose(st[:, k11, 2], [1.69, 9.64, 16.1, 15.9], atol=0.06) and np.allclose(st[:, k100, 2], [4.39, 12.0, 18.7, 19.3], atol=0.06)
