"""The selection entries, gsdf_erase_selected and gsdf_compact on the GPU (include/gsdf.h, "REMOVING VOXELS") against the numpy
restatement tests/erase_ref.py, which evaluates every predicate for EVERY voxel of the map's export by brute force.  Every
comparison is of key sets and bytes.

Maps: Sequence("spheres", 160, 120, n_frames=12, seed=1, step_deg=0.5), voxel size 0.02, truncation 5 voxels, capacity 2^19; map
A = frames 0..7 (the pair of test_gpu_merge_posed.py).  Tests that change a map work on a copy (gsdf_merge_from into an empty
context: 0 + x = x, the bytes of A)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import erase_ref as E
from conftest import ROOT

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, VS, TRUNC, CAP = 160, 120, 0.02, 5, 19
OK, ERR_TABLE_FULL, ERR_KEY_RANGE, ERR_INVALID, ERR_HIP = 0, 1, 2, 3, 4
HOST = os.path.join(ROOT, "gradient-sdf_amd", "host")
INF = f32(np.inf)


def _quat(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([np.sin(h) * a, [np.cos(h)]]).astype(f32)


SKEW = np.concatenate([np.asarray((0.0537, -0.0291, 0.0413), f32), _quat((0.3, -0.5, 0.8), 7.0)]).astype(f32)   # test_gpu_merge_posed.py's


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _fused(pkg, seq, frames=range(8), cap=CAP, **kw):
    vs = f32(VS)
    g = pkg.GradSdf(vs, f32(TRUNC) * vs, W, H, seq.K, capacity_log2=cap, **kw)
    for i in frames:
        g.update(*seq.frame(i))
    return g


@pytest.fixture(scope="module")
def A(pkg):
    """map A, never changed (selections come and go), with its raw export and some of its surface cloud"""
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=12, seed=1, step_deg=0.5)
    g = _fused(pkg, seq)
    k, p = g.export(sorted=True, raw=True)
    cloud = g.surface_cloud()[:, :3]
    m = dict(seq=seq, g=g, k=k, p=p, vs=f32(VS), cloud=np.ascontiguousarray(cloud[::max(1, len(cloud) // 300)][:300]))
    print("map A: %d voxels in %d blocks, %d cloud points used" % (len(k), len(E.blocks(k)), len(m["cloud"])))
    yield m
    g.close()


@pytest.fixture(scope="module")
def Abase(pkg, A):
    g = _fused(pkg, A["seq"], map_type=pkg.MAP_BASE)
    k, p = g.export(sorted=True, raw=True)
    yield dict(seq=A["seq"], g=g, k=k, p=p, vs=f32(VS))
    g.close()


def _copy(pkg, m, cap=CAP, **kw):
    g = pkg.GradSdf(m["vs"], f32(TRUNC) * m["vs"], W, H, m["seq"].K, capacity_log2=cap, map_type=m["g"].map_type, **kw)
    g.merge_from(m["g"])
    assert _same(g.export(sorted=True, raw=True)[1], m["p"])
    return g


def _selection_is(g, m, mask, n=None):
    """the selection's export equals the masked rows of the map's export, in bytes, and the counts agree"""
    k, p = g.select_export(raw=True)
    assert _same(k, m["k"][mask]), "key sets differ: %d exported, %d expected" % (len(k), int(mask.sum()))
    assert _same(p, m["p"][mask])
    assert g.select_count() == (int(mask.sum()), len(E.blocks(m["k"][mask])))
    if n is not None:
        assert n == int(mask.sum())


def _boxes(m):
    k, vs = m["k"], m["vs"]
    q = lambda f: np.quantile(k, f, axis=0).astype(np.int64)
    lo_i, hi_i = q(0.3), q(0.7)
    mid = (vs * q(0.5).astype(f32)).astype(f32)
    blo, bhi = (q(0.25) >> 2) << 2, ((q(0.75) >> 2) << 2) + 3
    half = f32(vs / 2)
    return {
        "faces": (vs * lo_i.astype(f32), vs * hi_i.astype(f32)),                      # faces ON voxel centres
        "cut": (mid - np.array([0.1137, 0.0731, 0.0913], f32), mid + np.array([0.0977, 0.1219, 0.1051], f32)),
        "blocks": (vs * blo.astype(f32) - half, vs * bhi.astype(f32) + half),          # whole 4x4x4 blocks
        "outside": (np.array([100, 100, 100], f32), np.array([101, 101, 101], f32)),
        "inverted": (np.array([-INF, 1.0, -INF], f32), np.array([INF, -1.0, INF], f32)),
        "all": (np.array([-INF] * 3, f32), np.array([INF] * 3, f32)),
    }


def _check_boxes(m):
    g = m["g"]
    for name, (lo, hi) in _boxes(m).items():
        mask = E.box(m["k"], m["vs"], lo, hi)
        n = g.select_box(lo, hi)
        print("box %-8s %6d of %d voxels" % (name, n, len(m["k"])))
        _selection_is(g, m, mask, n)
        if name == "faces":                                    # premise: voxels sit ON the faces, so the closed comparison decides
            c = E.centres(m["k"], m["vs"])
            assert (mask & (c[:, 0] == f32(lo[0]))).any() and (mask & (c[:, 0] == f32(hi[0]))).any()
        elif name in ("outside", "inverted"):
            assert n == 0
        elif name == "all":
            assert n == len(m["k"])
        else:
            assert 0 < n < len(m["k"])
    g.select_clear()


# ---- 1. box -------------------------------------------------------------------------------------------------------------------
def test_box(A):
    _check_boxes(A)


# ---- 2. weight ----------------------------------------------------------------------------------------------------------------
def test_weight(A):
    g, p = A["g"], A["p"]
    low, high = E.weight(p, 0, 5), E.weight(p, 5, np.inf)
    assert low.any() and high.any() and (low ^ high).all()     # the two halves partition the map
    _selection_is(g, A, low, g.select_weight(0, 5))
    _selection_is(g, A, high, g.select_weight(5, np.inf))
    w = p[len(p) // 2, 4]
    one = E.weight(p, w, np.nextafter(w, INF))
    assert one.any() and (p[one, 4] == w).all()
    _selection_is(g, A, one, g.select_weight(w, np.nextafter(w, INF)))
    assert g.select_weight(5, 5) == 0 and g.select_weight(7, 3) == 0
    g.select_clear()


# ---- 3. points: the equality case ---------------------------------------------------------------------------------------------
def test_points_equality(A):
    g, k, vs, cloud = A["g"], A["k"], A["vs"], A["cloud"]
    r25 = f32(2.5) * vs
    mask = E.points(k, vs, cloud, r25)
    print("300 cloud points at 2.5 voxels: %d voxels" % mask.sum())
    assert 1000 < mask.sum() < len(k)
    _selection_is(g, A, mask, g.select_points(cloud, r25))
    # a voxel (i, j, kk) with (i + 2, j, kk) in the map too, both far from every cloud point: only the added point decides
    packed = E.pack(k)
    has = np.isin(E.pack(k + np.array([2, 0, 0], np.int32)), packed)
    pick = None
    for idx in np.nonzero(has)[0][::97]:
        c2 = E.centres(k[idx] + np.array([2, 0, 0], np.int32), vs)
        if np.sqrt(((cloud.astype(np.float64) - c2.astype(np.float64)) ** 2).sum(axis=1)).min() > 4 * float(vs):
            pick = idx
            break
    assert pick is not None, "premise: a voxel pair away from the cloud"
    i = int(k[pick, 0])
    pt = E.centres(k[pick], vs)
    r = f32(f32(vs * f32(i + 2)) - pt[0])
    target = packed == E.pack(k[pick] + np.array([2, 0, 0], np.int32))
    pts = np.concatenate([cloud, pt[None, :]])
    for radius, inside in ((r, True), (np.nextafter(r, f32(0)), False)):
        mask = E.points(k, vs, pts, radius)
        assert bool(mask[target][0]) == inside, "premise: the restatement puts voxel i + 2 %s" % ("in" if inside else "out")
        _selection_is(g, A, mask, g.select_points(pts, radius))
    g.select_clear()


# ---- 4. points: the other edges -----------------------------------------------------------------------------------------------
def test_points_edges(pkg, O, A):
    g, k, vs, cloud = A["g"], A["k"], A["vs"], A["cloud"]
    r = f32(2.5) * vs
    base = E.points(k, vs, cloud[:50], r)
    n1 = g.select_points(cloud[:50], r)
    assert g.select_points(np.concatenate([cloud[:50]] * 3), r) == n1 == base.sum()           # duplicates: a voxel counts once
    bad = np.array([[np.nan, 0, 1], [0, np.inf, 1], [-np.inf, 0, 0]], f32)
    _selection_is(g, A, base, g.select_points(np.concatenate([bad, cloud[:50], bad]), r))      # skipped
    assert g.select_points(bad, r) == 0
    assert g.select_points(np.zeros((0, 3), f32), r) == 0 and g.select_count() == (0, 0)       # n = 0
    on = E.centres(k[::1013], vs)                                                              # radius 0: the voxels the points sit on
    m0 = E.points(k, vs, on, 0)
    assert m0.sum() == len(on)
    _selection_is(g, A, m0, g.select_points(on, 0))
    _selection_is(g, A, E.points(k, vs, cloud, 0), g.select_points(cloud, 0))
    big = E.points(k, vs, cloud[[0, 150, 299]], f32(16) * vs)                                  # the largest radius
    print("3 points at 16 voxels: %d voxels" % big.sum())
    assert big.sum() > 3000
    _selection_is(g, A, big, g.select_points(cloud[[0, 150, 299]], f32(16) * vs))
    lim = float(vs) * 2 ** 20                                                                  # beyond the packable range: nothing, no wrap
    far = np.array([[lim + 0.01, 0, 1], [-lim - 0.3, 0, 1], [0, 2 * lim + 5, 1], [0, 0, -3e30], [lim - 0.01, 0.1, 1.5]], f32)
    assert not E.points(k, vs, far, f32(16) * vs).any()
    assert g.select_points(far, f32(16) * vs) == 0 and g.select_count() == (0, 0)
    posed = E.points(k, vs, cloud, r, SKEW, O)                                                  # a pose: R x + t as the registration forms it
    assert posed.any() and not np.array_equal(posed, E.points(k, vs, cloud, r))
    _selection_is(g, A, posed, g.select_points(cloud, r, pose7=SKEW))
    dev = g.upload(cloud)                                                                      # the _dev variant: the same set
    _selection_is(g, A, posed, g.select_points_dev(dev, len(cloud), r, pose7=SKEW))
    _selection_is(g, A, E.points(k, vs, cloud, r), g.select_points_dev(dev, len(cloud), r))
    cap = int(posed.sum())                                                                     # ... and the export into device buffers
    g.select_points_dev(dev, len(cloud), r, pose7=SKEW)
    kd, pd = g.upload(np.zeros((cap, 3), np.int32)), g.upload(np.zeros((cap, 5), f32))
    assert g.select_export_raw_dev(None, None, 0) == cap                                       # the sizing call
    assert g.select_export_raw_dev(kd.value, pd.value, cap) == cap
    kk, pp = g.download(kd, (cap, 3), np.int32), g.download(pd, (cap, 5), f32)
    order = np.argsort(E.pack(kk))
    assert _same(kk[order], k[posed]) and _same(pp[order], A["p"][posed])                       # each member exactly once
    with pytest.raises(pkg.GsdfError) as e:
        g.select_export_raw_dev(kd.value, pd.value, cap - 1)
    assert e.value.code == ERR_INVALID
    g.select_clear()


# ---- 5. ops -------------------------------------------------------------------------------------------------------------------
def test_ops_and_invert(pkg, A):
    g, k, vs, cloud = A["g"], A["k"], A["vs"], A["cloud"]
    lo, hi = _boxes(A)["cut"]
    B = E.box(k, vs, lo, hi)
    r = f32(2.5) * vs
    P = E.points(k, vs, cloud, r)
    assert (B & P).any() and (B & ~P).any() and (~B & P).any()
    for op in (pkg.SEL_ADD, pkg.SEL_INTERSECT, pkg.SEL_SUBTRACT, pkg.SEL_REPLACE):
        g.select_box(lo, hi)
        _selection_is(g, A, E.combine(op, B, P), g.select_points(cloud, r, op=op))
        g.select_clear()                                        # from none the combining ops start from the empty set
        _selection_is(g, A, E.combine(op, None, P), g.select_points(cloud, r, op=op))
    g.select_box(lo, hi)
    _selection_is(g, A, E.combine(E.SUBTRACT, B, E.weight(A["p"], 0, 5)), g.select_weight(0, 5, op=pkg.SEL_SUBTRACT))
    _selection_is(g, A, E.combine(E.ADD, E.combine(E.SUBTRACT, B, E.weight(A["p"], 0, 5)), P), g.select_points(cloud, r, op=pkg.SEL_ADD))
    g.select_box(lo, hi)
    _selection_is(g, A, E.invert(B, len(k)), g.select_invert())
    _selection_is(g, A, B, g.select_invert())
    g.select_clear()
    _selection_is(g, A, E.invert(None, len(k)), g.select_invert())
    g.select_clear()


# ---- 6. states and refusals ---------------------------------------------------------------------------------------------------
def _refused(pkg, call, word=None):
    with pytest.raises(pkg.GsdfError) as e:
        call()
    assert e.value.code == ERR_INVALID
    if word:
        assert word in str(e.value)


def test_states(pkg, A):
    g = _copy(pkg, A)
    try:
        lo, hi = _boxes(A)["cut"]
        n = g.select_box(lo, hi)
        assert n > 0 and g.select_count()[0] == n
        g.grow(CAP + 1)                                         # slots move: lost
        for call in (g.select_count, g.select_export, g.erase_selected, g.select_invert, lambda: g.select_export_raw_dev(None, None, 0),
                     lambda: g.select_weight(0, 5, op=pkg.SEL_ADD), lambda: g.select_box(lo, hi, op=pkg.SEL_INTERSECT),
                     lambda: g.select_points(A["cloud"], 0.05, op=pkg.SEL_SUBTRACT)):
            _refused(pkg, call, "lost")
        assert _same(g.export(sorted=True, raw=True)[1], A["p"])
        assert g.select_box(lo, hi) == n                        # REPLACE starts over
        g.grow(CAP + 2)
        g.select_clear()                                       # ... and so does clear: none
        assert g.select_count() == (0, 0) and len(g.select_export()[0]) == 0 and g.erase_selected() == (0, 0)
        assert _same(g.export(sorted=True, raw=True)[1], A["p"])
        assert g.select_box(lo, hi) == n
        assert g.erase_selected()[0] == n                       # erase leaves none
        assert g.select_count() == (0, 0) and g.erase_selected() == (0, 0)
        left = g.count()
        g.select_weight(0, np.inf)
        g.compact()                                             # compact leaves none
        assert g.select_count() == (0, 0) and g.erase_selected() == (0, 0) and g.count() == left
        g.select_weight(0, np.inf)
        g.reset()                                               # reset leaves none
        assert g.select_count() == (0, 0) and g.count() == 0
    finally:
        g.close()


def test_refusals_leave_the_map_alone(pkg, A):
    g, cloud, vs = A["g"], A["cloud"], A["vs"]
    lo, hi = _boxes(A)["cut"]
    n = g.select_box(lo, hi)
    nan = f32(np.nan)
    bad_q = SKEW.copy(); bad_q[3:] *= f32(1.01)
    nan_pose = SKEW.copy(); nan_pose[1] = nan
    L = g.L
    for call in (lambda: g.select_box([nan, 0, 0], hi), lambda: g.select_box(lo, [0, 0, nan]),
                 lambda: g.select_weight(nan, 5), lambda: g.select_weight(0, nan),
                 lambda: g.select_points(cloud, -0.01), lambda: g.select_points(cloud, np.inf), lambda: g.select_points(cloud, nan),
                 lambda: g.select_points(cloud, np.nextafter(f32(16) * vs, INF)),
                 lambda: g.select_points(cloud, 0.05, pose7=bad_q), lambda: g.select_points(cloud, 0.05, pose7=nan_pose),
                 lambda: g.select_box(lo, hi, op=4), lambda: g.select_weight(0, 5, op=-1), lambda: g.select_points(cloud, 0.05, op=7),
                 lambda: g._chk(L.gsdf_select_points(g.h, None, 5, None, f32(0.05), 0, None)),
                 lambda: g._chk(L.gsdf_select_points(g.h, None, -1, None, f32(0.05), 0, None)),
                 lambda: g.compact(9), lambda: g.compact(31)):
        _refused(pkg, call)
    assert g.select_count()[0] == n                             # the selection is as it was
    assert _same(g.export(sorted=True, raw=True)[0], A["k"]) and _same(g.export(sorted=True, raw=True)[1], A["p"])
    g.select_clear()


# ---- 7. erase -----------------------------------------------------------------------------------------------------------------
def _check_erase(pkg, m, cloud=None):
    g = _copy(pkg, m)
    try:
        lo, hi = _boxes(m)["blocks"]
        S = E.box(m["k"], m["vs"], lo, hi)
        g.select_box(lo, hi)
        if cloud is not None:
            S = S | E.points(m["k"], m["vs"], cloud, f32(2.5) * m["vs"])
            g.select_points(cloud, f32(2.5) * m["vs"], op=pkg.SEL_ADD)
        ek, ep, nv, nb = E.erase(m["k"], m["p"], S)
        assert nv > 0 and nb > 0 and len(ek) > 0, "premise: the erase empties whole blocks and leaves others"
        assert g.erase_selected() == (nv, nb)
        k, p = g.export(sorted=True, raw=True)
        assert _same(k, ek) and _same(p, ep)                    # the remaining records keep their bytes
        assert g.count() == len(ek)
        print("erase: %d voxels, %d blocks emptied, %d voxels left" % (nv, nb, len(ek)))
    finally:
        g.close()


def test_erase(pkg, A):
    _check_erase(pkg, A, A["cloud"])


# ---- 8. take out, compact, put back -------------------------------------------------------------------------------------------
def _check_round_trip(pkg, m):
    g = _copy(pkg, m)
    try:
        lo, hi = _boxes(m)["blocks"]
        S = E.box(m["k"], m["vs"], lo, hi)
        g.select_box(lo, hi)
        tk, tp = g.select_export(raw=True)
        assert _same(tk, m["k"][S]) and _same(tp, m["p"][S])
        blocks_before = g.block_keys_dev(None, 0)
        nv, nb = g.erase_selected()
        assert nb > 0 and blocks_before == len(E.blocks(m["k"]))
        assert g.block_keys_dev(None, 0) == blocks_before      # erase keeps the keys
        kept = g.export(sorted=True, raw=True)
        assert g.compact() == nb
        assert g.block_keys_dev(None, 0) == blocks_before - nb
        k, p = g.export(sorted=True, raw=True)
        assert _same(k, kept[0]) and _same(p, kept[1]) and _same(k, m["k"][~S])
        g.merge_raw(tk, tp)
        k, p = g.export(sorted=True, raw=True)
        assert _same(k, m["k"])
        assert np.array_equal(p, m["p"])                        # equal as floats ...
        diff = p.view(np.uint32) ^ m["p"].view(np.uint32)
        assert ((diff == 0) | ((diff == 0x80000000) & (m["p"] == 0))).all()     # ... and in bits except the sign of a zero
        print("round trip: %d voxels out and back, %d blocks dropped, %d zero signs changed" % (nv, nb, int((diff != 0).sum())))
    finally:
        g.close()


def test_take_out_compact_put_back(pkg, A):
    _check_round_trip(pkg, A)


# ---- 9. erase leaves nothing behind -------------------------------------------------------------------------------------------
def test_erase_leaves_nothing_behind(pkg, A):
    seq = A["seq"]
    a, b = _fused(pkg, seq), _fused(pkg, seq)
    try:
        fresh = a.export(sorted=True, raw=True)
        assert _same(fresh[0], b.export(sorted=True, raw=True)[0]) and _same(fresh[1], b.export(sorted=True, raw=True)[1])   # premise
        assert b.select_box([-INF] * 3, [INF] * 3) == len(fresh[0])
        assert b.erase_selected()[0] == len(fresh[0]) and b.count() == 0
        for i in range(8):
            b.update(*seq.frame(i))
        again = b.export(sorted=True, raw=True)
        assert _same(again[0], fresh[0]) and _same(again[1], fresh[1])
    finally:
        a.close()
        b.close()


def test_erase_leaves_nothing_behind_with_vis(pkg, A):
    """With gsdf_enable_vis(8) (one 32-bit word per voxel).  gsdf_erase_selected leaves Sdf::counter_ alone, so the second run of
    frames 0..7 is integrated as frames 8..15 and sets bits 8..15 where the fresh context has bits 0..7: the vis_ words must be
    the fresh ones shifted by 8 bits EXACTLY -- a word that kept a stale bit 0..7 through the erase differs."""
    seq = A["seq"]
    vs = f32(VS)

    def fused_vis():
        g = pkg.GradSdf(vs, f32(TRUNC) * vs, W, H, seq.K, capacity_log2=CAP)
        g.enable_vis(8)
        for i in range(8):
            g.update(*seq.frame(i))
        return g
    a, b = fused_vis(), fused_vis()
    try:
        fresh, fresh_vis = a.export(sorted=True, raw=True), a.export_vis()
        assert _same(fresh_vis[1], b.export_vis()[1]) and _same(fresh[1], b.export(sorted=True, raw=True)[1])               # premise
        assert fresh_vis[1].any()
        b.select_weight(0, np.inf)
        assert b.erase_selected()[0] == len(fresh[0])
        assert int(b.stats()["frames"]) == 8
        for i in range(8):
            b.update(*seq.frame(i))
        again = b.export(sorted=True, raw=True)
        assert _same(again[0], fresh[0]) and _same(again[1], fresh[1])
        kv, got = b.export_vis()
        assert _same(kv, fresh_vis[0]) and (fresh_vis[1] < 256).all()
        assert _same(got, fresh_vis[1] << np.uint32(8))
    finally:
        a.close()
        b.close()


# ---- 10. compact to a smaller table ---------------------------------------------------------------------------------------------
def test_compact_to_a_smaller_table(pkg, O, A):
    g = _copy(pkg, A)
    try:
        k, vs, seq = A["k"], A["vs"], A["seq"]
        all_blocks = len(E.blocks(k))
        mid = np.quantile(k, 0.5, axis=0).astype(np.int64)
        half = 6
        while True:                                             # a box around the middle that keeps under a fifth of the blocks
            lo, hi = vs * (mid - half).astype(f32), vs * (mid + half).astype(f32)
            S = E.box(k, vs, lo, hi)
            if len(E.blocks(k[S])) * 5 < all_blocks and S.sum() > 500:
                break
            half -= 1
            assert half > 1
        erased = g.crop(lo, hi)
        live = len(E.blocks(k[S]))
        assert erased == int((~S).sum()) and g.count() == int(S.sum())
        kept = g.export(sorted=True, raw=True)
        assert _same(kept[0], k[S]) and _same(kept[1], A["p"][S])
        need = 10
        while live * 100 > (2 ** need // 64) * 45:
            need += 1
        print("crop keeps %d of %d blocks (%d voxels): smallest capacity_log2 the 45 %% rule admits: %d" % (live, all_blocks, S.sum(), need))
        assert need <= 17
        if need > 10:
            with pytest.raises(pkg.GsdfError) as e:
                g.compact(need - 1)
            assert e.value.code == ERR_TABLE_FULL and g.capacity_log2() == CAP
            now = g.export(sorted=True, raw=True)
            assert _same(now[0], kept[0]) and _same(now[1], kept[1])
        assert g.compact(need) == 0 and g.capacity_log2() == need
        now = g.export(sorted=True, raw=True)
        assert _same(now[0], kept[0]) and _same(now[1], kept[1])
        assert g.block_keys_dev(None, 0) == live
        # the map works: mesh, cloud, raycast, one tracked frame
        assert len(g.extract_mesh()) > 0 and len(g.surface_cloud()) > 0
        d, R, t = seq.frame(8)
        depth, _ = g.raycast(R, t)
        assert (depth > 0).any()
        # pixels whose ray stays outside the crop box grown by the truncation distance see nothing
        T = f32(TRUNC) * vs
        K = np.asarray(seq.K, np.float64).reshape(3, 3)
        ys, xs = np.mgrid[0:H, 0:W]
        dirs = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs, np.float64)], -1) @ np.asarray(R, np.float64).T
        blo, bhi = lo.astype(np.float64) - float(T), hi.astype(np.float64) + float(T)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0 = (blo - np.asarray(t, np.float64)) / dirs
            t1 = (bhi - np.asarray(t, np.float64)) / dirs
        tn, tf = np.minimum(t0, t1).max(-1), np.maximum(t0, t1).min(-1)
        misses = ~((tn <= tf) & (tf >= 0.5) & (tn <= 3.5))
        print("raycast: %d pixels hit, %d rays miss the grown box" % ((depth > 0).sum(), misses.sum()))
        assert misses.any() and (depth[misses] == 0).all()
        pose0 = np.concatenate([np.asarray(seq.frame(7)[2], f32), O.R_to_quat(seq.frame(7)[1])]).astype(f32)
        conv, pose, passes = g.track(d, pose0)
        assert passes > 0 and np.isfinite(pose).all()
        g.grow(CAP)                                             # (a whole frame needs more blocks than the smallest table holds)
        assert _same(g.export(sorted=True, raw=True)[1], kept[1])
        g.update(d, R, t)
        assert g.count() > int(S.sum())
    finally:
        g.close()


# ---- 11. the other map type -----------------------------------------------------------------------------------------------------
def test_base_map_box_erase_round_trip(pkg, Abase):
    assert Abase["g"].map_type == pkg.MAP_BASE
    _check_boxes(Abase)
    _check_erase(pkg, Abase)
    _check_round_trip(pkg, Abase)


# ---- 12. Scan3D --crop, the facade ----------------------------------------------------------------------------------------------
def _ply_points(path):
    rows, n, body = [], 0, False
    for line in open(path):
        if body:
            v = line.split()
            if len(v) >= 3:
                rows.append([float(v[0]), float(v[1]), float(v[2])])
        elif line.startswith("element vertex"):
            n = int(line.split()[2])
        elif line.startswith("end_header"):
            body = True
    return np.asarray(rows[:n], np.float64).reshape(-1, 3)


def test_scan3d_crop_and_prune(pkg, tmp_path):
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=12, seed=1, step_deg=0.5)
    ds = pkg.synth.write_dataset(seq, str(tmp_path / "ds"), layout="synth")
    res = {}

    def run(name, extra):
        r = str(tmp_path / name) + "/"
        os.makedirs(r)
        cmd = [os.path.join(HOST, "Scan3D"), "--input", ds, "--results", r, "--scan-type", "grad-sdf", "--data-type", "synth",
               "--voxel-size", "0.02", "--trunc", "5", "--width", str(W), "--height", str(H), "--hash-capacity", "19"]
        out = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert ("Voxels: " in out.stdout) == bool(extra)
        res[name] = _ply_points(r + "gradient_sdf_cloud_final.ply")

    run("plain", [])
    assert len(res["plain"]) > 1000
    lo, hi = np.quantile(res["plain"], 0.25, axis=0).astype(f32), np.quantile(res["plain"], 0.75, axis=0).astype(f32)
    run("crop", ["--crop"] + [repr(float(v)) for v in np.concatenate([lo, hi])])
    run("prune", ["--prune-weight", "5"])
    n_plain, pts = len(res["plain"]), res["crop"]
    print("Scan3D: %d points, %d with --crop, %d with --prune-weight 5" % (n_plain, len(pts), len(res["prune"])))
    assert 0 < len(pts) < n_plain
    # extract_pc keeps |dist * 1.2 g^| < vs / 2 per axis, so a point lies within vs / 2 of its voxel's centre; the ASCII file
    # holds 6 significant digits (coordinates below 10 m: 5e-6)
    half = VS / 2 + 1e-5
    assert (pts >= lo.astype(np.float64) - half).all() and (pts <= hi.astype(np.float64) + half).all()
    assert len(res["prune"]) == n_plain                         # extract_pc itself asks for weight >= 5
    bad = subprocess.run([os.path.join(HOST, "Scan3D"), "--input", ds, "--crop", "0", "0"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "--crop" in bad.stderr


@pytest.mark.parametrize("kind", ["grad", "base"])
def test_erase_selftest_binary(pkg, tmp_path, kind):
    n = 3
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=n, seed=4, step_deg=2.0)
    d = tmp_path
    np.asarray(seq.K, f32).reshape(9).tofile(d / "K.bin")
    np.stack([seq.frame(i)[0] for i in range(n)]).astype(f32).tofile(d / "depth.bin")
    np.stack([pkg.synth.pose16(*seq.pose(i)) for i in range(n)]).astype(f32).tofile(d / "poses.bin")
    out = subprocess.run([os.path.join(HOST, "erase_selftest"), str(d), str(W), str(H), str(n), repr(float(f32(VS))), "5"]
                         + (["base"] if kind == "base" else []), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "erase_selftest: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
