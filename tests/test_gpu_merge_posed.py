"""gsdf_merge_from_posed on the GPU (include/gsdf.h) against the numpy restatement tests/merge_posed_ref.py, which evaluates
steps 1-7 of the definition for EVERY key of an integer box around the image of src (no blocks, no enumeration), with the
engine's own gsdf_query / gsdf_get_voxels of src as its readers.

Maps: Sequence("spheres", 160, 120, n_frames=12, seed=1, step_deg=0.5); map A = frames 0..7, map B = frames 4..11 (the pair of
test_gpu_align_points.py).  B is always the source."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import merge_posed_ref as ref
from conftest import ROOT, pose7_from

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, VS, TRUNC, CAP = 160, 120, 0.02, 5, 19
MAX_BOX = 10 ** 7
OK, ERR_TABLE_FULL, ERR_KEY_RANGE, ERR_INVALID, ERR_HIP = 0, 1, 2, 3, 4
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], f32)


def _quat(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([np.sin(h) * a, [np.cos(h)]]).astype(f32)


def _pose(axis, deg, t):
    return np.concatenate([np.asarray(t, f32), _quat(axis, deg)]).astype(f32)


SKEW = _pose((0.3, -0.5, 0.8), 7.0, (0.0537, -0.0291, 0.0413))        # 2.685, -1.455, 2.065 voxels
NEAR = _pose((0.3, -0.5, 0.8), 1.0, (0.01, -0.008, 0.006))            # the displacement of the registration tests


def _pair(pkg):
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=12, seed=1, step_deg=0.5)
    vs = f32(VS)
    T = f32(TRUNC) * vs
    ga = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=CAP)
    gb = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=CAP)
    for i in range(8):
        ga.update(*seq.frame(i))
    for i in range(4, 12):
        gb.update(*seq.frame(i))
    return dict(seq=seq, vs=vs, T=T, ga=ga, gb=gb)


@pytest.fixture(scope="module")
def pair(pkg):
    p = _pair(pkg)
    p["bk"], p["bp"] = p["gb"].export(sorted=True, raw=True)
    yield p
    p["ga"].close()
    p["gb"].close()


def _fresh(pkg, pair, cap=CAP, lib=None, vs=None, T=None, **kw):
    return pkg.GradSdf(pair["vs"] if vs is None else vs, pair["T"] if T is None else T, W, H, pair["seq"].K, capacity_log2=cap, lib=lib, **kw)


def _frames(g):
    return int(g.stats()["frames"])


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _expect(O, pair, src, src_keys, dst, pose7):
    """the restatement's result for dst += src under pose7, from dst's export as it is now"""
    box = ref.box_of(src_keys, pose7, pair["vs"], O)
    assert ref.box_size(box) <= MAX_BOX, ref.box_size(box)
    return ref.expected(dst.export(sorted=True, raw=True), src.query, src.get_voxels, pose7, pair["vs"], pair["T"], box, O)


def _merge_equals_restatement(O, pair, dst, pose7, src=None, src_keys=None):
    src = pair["gb"] if src is None else src
    src_keys = pair["bk"] if src_keys is None else src_keys
    ek, ep, ck, cc = _expect(O, pair, src, src_keys, dst, pose7)
    nv, nb = dst.merge_from_posed(src, pose7)
    k, p = dst.export(sorted=True, raw=True)
    print("pose %s: %d contributions in %d blocks, %d voxels afterwards" % (np.array2string(np.asarray(pose7), precision=4), len(ck), ref.n_blocks(ck), len(k)))
    assert len(ck) > 0, "premise: the merge moves something"
    missed = np.setdiff1d(ref.pack(ek), ref.pack(k))
    extra = np.setdiff1d(ref.pack(k), ref.pack(ek))
    assert len(missed) == 0 and len(extra) == 0, "key sets differ: %d missed by the kernel, %d not in the restatement" % (len(missed), len(extra))
    assert _same(k, ek)
    assert _same(p, ep), "%d records differ in bits" % int((p.view(np.uint32) != ep.view(np.uint32)).any(axis=1).sum())
    assert (nv, nb) == (len(ck), ref.n_blocks(ck))
    return k, p, ck, cc


# ---- 1. bit-exact into an empty dst -------------------------------------------------------------------------------------------
def test_empty_dst_equals_the_restatement_in_bits(pkg, O, pair):
    """7 degrees about (0.3, -0.5, 0.8) and a translation of (2.685, -1.455, 2.065) voxels into an empty map: key set and all
    five raw sums equal to the brute force over the whole box, n_voxels and n_blocks exact.  A key the enumeration missed would
    be a key-set difference."""
    dst = _fresh(pkg, pair)
    try:
        _merge_equals_restatement(O, pair, dst, SKEW)
        assert _frames(dst) == _frames(pair["gb"]) == 8
    finally:
        dst.close()


# ---- 2. / 10. bit-exact into map A; afterwards the map works -------------------------------------------------------------------
@pytest.fixture(scope="module")
def merged_into_a(pkg, O, pair):
    dst = _fresh(pkg, pair)
    dst.merge_from(pair["ga"])                                       # dst = map A (the module's A stays as it is)
    old = dst.export(sorted=True, raw=True)
    tris_a = len(dst.extract_mesh())
    k, p, ck, cc = _merge_equals_restatement(O, pair, dst, NEAR)
    yield dict(dst=dst, old=old, k=k, p=p, ck=ck, tris_a=tris_a)
    dst.close()


def test_nonempty_dst_is_old_plus_contribution_in_bits(pair, merged_into_a):
    """dst = map A: every record equals old + contribution in bits (asserted against the restatement when the fixture merged),
    records of A that receive nothing keep their bytes, Sdf::counter_ = frames of both"""
    m = merged_into_a
    ok, op = m["old"]
    untouched = ~np.isin(ref.pack(ok), ref.pack(m["ck"]))
    assert untouched.any() and (~untouched).any(), "premise: A has records that receive and records that do not"
    at = np.searchsorted(ref.pack(m["k"]), ref.pack(ok[untouched]))
    assert _same(m["p"][at], op[untouched])
    assert _frames(m["dst"]) == 16


def test_merged_map_works(O, pair, merged_into_a):
    """one tracked frame, extract_mesh, surface_cloud and a raycast on the merged map; the mesh has at least A's triangles"""
    dst, seq = merged_into_a["dst"], pair["seq"]
    d, R, t = seq.frame(8)
    _, R7, t7 = seq.frame(7)
    _, pose, passes = dst.track(d, pose7_from(O, R7, t7), iters=5)
    assert passes >= 1 and np.isfinite(pose).all()
    tris = dst.extract_mesh()
    assert len(tris) >= merged_into_a["tris_a"] > 0
    cloud = dst.surface_cloud()
    assert len(cloud) > 0 and np.isfinite(cloud).all()
    depth, _ = dst.raycast(R, t)
    assert (depth > 0).sum() > 1000


# ---- 3. poses that stress the enumeration --------------------------------------------------------------------------------------
STRESS = {
    "x45": _pose((1, 0, 0), 45.0, (0, 0, 0)),
    "y45": _pose((0, 1, 0), 45.0, (0, 0, 0)),
    "z45": _pose((0, 0, 1), 45.0, (0, 0, 0)),
    "z180": _pose((0, 0, 1), 180.0, (0, 0, 0)),
    "far": np.array([0, f32(1000.37) * f32(VS), 0, 0, 0, 0, 1], f32),          # coordinates of ~20 m: coarser float spacing
    "borders": np.array([f32(0.5) * f32(VS)] * 3 + [0, 0, 0, 1], f32),         # q on the borders between voxels
}


@pytest.mark.parametrize("name", sorted(STRESS))
def test_stress_poses_equal_the_restatement_in_bits(pkg, O, pair, name):
    dst = _fresh(pkg, pair)
    try:
        _merge_equals_restatement(O, pair, dst, STRESS[name])
    finally:
        dst.close()


# ---- 4. identity --------------------------------------------------------------------------------------------------------------
def test_identity_equals_merge_from_up_to_the_round_trip_of_s(pkg, pair):
    """Pose identity: q = c_K exactly (R = I in bits), so V = K and phi = dist_V: keys, w and the gradient sums are bit-equal to
    gsdf_merge_from's.  s' = S_w * truncate(S_s / S_w, T):
      - where |S_s / S_w| <= T the clamp does nothing and s' is the round trip S_w * (S_s / S_w), within 1 ulp of S_s (a correctly
        rounded quotient and a correctly rounded product: the exact product lies within 2^-24 |s| < 1 ulp of s, its rounding
        within another half);
      - a voxel all of whose samples were truncated holds S_s = sum(w_i T) rounded term by term, and its float quotient can exceed
        T by an ulp or two; step 6 of the definition clamps it, so there s' = S_w * (+-T) in bits.  (Measured: 1065 of 14743
        records differ from S_s at all; 4 records are clamped, at most 2 ulp from S_s; the others at most 1 ulp.)
    Every record falls under one of the two."""
    a, b = _fresh(pkg, pair), _fresh(pkg, pair)
    try:
        nv, nb = a.merge_from_posed(pair["gb"], IDENTITY)
        b.merge_from(pair["gb"])
        ka, pa = a.export(sorted=True, raw=True)
        kb, pb = b.export(sorted=True, raw=True)
        assert _same(ka, kb) and nv == len(kb) > 0 and nb == ref.n_blocks(kb)
        assert _same(pa[:, 1:], pb[:, 1:])
        T = pair["T"]
        dist = (pb[:, 0] / pb[:, 4]).astype(f32)                     # the correctly rounded float quotient, as the kernel's
        clamped = np.abs(dist) > T
        ulp = np.spacing(np.maximum(np.abs(pa[:, 0]), np.abs(pb[:, 0])))
        ulps = np.abs(pa[:, 0].astype(np.float64) - pb[:, 0].astype(np.float64)) / ulp
        print("identity: s differs in %d of %d records; %d records clamped (at most %.1f ulp there), the others at most %.1f ulp" % (
            int((ulps > 0).sum()), len(ulps), int(clamped.sum()), float(ulps[clamped].max(initial=0.0)), float(ulps[~clamped].max())))
        assert ulps[~clamped].max() <= 1.0
        assert _same(pa[clamped, 0], (pb[clamped, 4] * np.copysign(T, dist[clamped])).astype(f32))
    finally:
        a.close()
        b.close()


# ---- 5. integer-voxel translation -----------------------------------------------------------------------------------------------
def test_integer_translation_shifts_the_keys(pkg, pair):
    """R = I, t = vs * (3, -5, 2): the keys are src's shifted by exactly (3, -5, 2), w and the gradient sums bit-equal (up to the
    sign of a zero: 1 * (-0) + (0 + 0) = +0), and |dist' - dist| <= 1.2 sqrt(3) B.
    B bounds |c_V - q| per axis: q = fl(fl(vs i) - fl(vs 3)) against c_V = fl(vs (i - 3)) -- four roundings (two products, the
    subtraction, c_V's product) of values no larger than C = the largest coordinate involved, each at most ulp(C) / 2, so
    B = 2 ulp(C); the kernel's own c_V - q is then exact (Sterbenz).  phi = dist + 1.2 g^ . (c_V - q), |g^| = 1, so
    |phi - dist| <= 1.2 |c_V - q|_2 <= 1.2 sqrt(3) B."""
    vs = pair["vs"]
    shift = np.array([3, -5, 2], np.int32)
    pose = np.concatenate([(vs * shift.astype(f32)).astype(f32), [0, 0, 0, 1]]).astype(f32)
    dst = _fresh(pkg, pair)
    try:
        nv, _ = dst.merge_from_posed(pair["gb"], pose)
        k, p = dst.export(sorted=True, raw=True)
        sk = pair["bk"] + shift[None, :]
        order = np.argsort(ref.pack(sk))
        assert _same(k, sk[order]) and nv == len(k)
        want = pair["bp"][order]
        assert _same(p[:, 1:], (want[:, 1:] + f32(0)).astype(f32))
        Cmax = f32(max(np.abs(vs * k.astype(f32)).max(), np.abs(vs * pair["bk"].astype(f32)).max(), np.abs(pose[:3]).max()))
        B = 2.0 * float(np.spacing(Cmax))
        dd = np.abs((p[:, 0] / p[:, 4]).astype(np.float64) - (want[:, 0] / want[:, 4]).astype(np.float64))
        print("integer shift: C = %.4f m, B = %.3e m, bound %.3e, max |dist' - dist| = %.3e" % (float(Cmax), B, 1.2 * np.sqrt(3) * B, float(dd.max())))
        assert dd.max() <= 1.2 * np.sqrt(3) * B
    finally:
        dst.close()


# ---- 6. a designed plane ---------------------------------------------------------------------------------------------------------
PLANE_N = np.array([0.48, -0.6, 0.64])                                # unit
PLANE_LO = np.array([10, -7, 40], np.int32)


def _plane_src(pkg, pair, lib=None):
    """24^3 voxels holding f(p) = d0 - n . p, clamped to +-T, with gradient sum w n, w = 3: the sign for which tsdf()'s
    dist + 1.2 g^ . (c_V - p) continues f off the voxel centre (f(p) = f(c_V) + n . (c_V - p))"""
    vs, T = pair["vs"], pair["T"]
    i = np.arange(24, dtype=np.int32)
    keys = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3) + PLANE_LO[None, :]
    c = keys.astype(np.float64) * float(vs)
    d0 = float(PLANE_N @ ((PLANE_LO + 11.5) * float(vs)))
    f = np.clip(d0 - c @ PLANE_N, -float(T), float(T)).astype(f32)
    w = f32(3)
    pay = np.concatenate([(w * f)[:, None], np.tile((w * PLANE_N.astype(f32))[None, :], (len(keys), 1)), np.full((len(keys), 1), w)], 1).astype(f32)
    g = _fresh(pkg, pair, cap=16, lib=lib)
    g.merge_raw(keys, pay)
    return g, keys, d0


def test_designed_plane(pkg, O, pair):
    """An oblique plane through a 24^3 box, merged under an oblique pose.  tsdf() continues a plane with slope 1.2 instead of 1,
    so the whole error of a value taken at distance r from its voxel centre is 0.2 |n . (c_V - p)| <= 0.2 (sqrt(3) / 2) vs --
    provided voxel V itself is not clamped, which holds wherever |f(p)| < T - (sqrt(3) / 2) vs (f changes by at most
    (sqrt(3) / 2) vs between p and c_V).  Where only |f(p)| < T is known, V may hold +-T instead of f(c_V), and the error is
    bounded by 1.2 (sqrt(3) / 2) vs (the whole off-centre term) -- both are asserted, the first is the one the test is about.
    Rounding: coordinates of magnitude C carry about 25 C 2^-24 per axis into q (gsdf_posed.h), 1.2 sqrt(3) times that into phi:
    64 C 2^-24 covers it."""
    vs, T = float(pair["vs"]), float(pair["T"])
    src, skeys, d0 = _plane_src(pkg, pair)
    dst = _fresh(pkg, pair, cap=17)
    try:
        half = np.sqrt(3) / 2 * vs
        rng = np.random.default_rng(5)
        # the premise, on src: gsdf_query at 10^4 random off-centre points inside the box
        pts = ((PLANE_LO + rng.uniform(0.5, 22.5, (10000, 3))) * vs).astype(f32)
        phi, _, w = src.query(pts)
        assert (w > 0).all()
        fp = d0 - pts.astype(np.float64) @ PLANE_N
        rnd = 64 * float(np.abs(pts).max()) * 2.0 ** -24
        inner = np.abs(fp) < T - half
        err = np.abs(phi.astype(np.float64) - fp)
        print("plane premise: %d of 10000 points unclamped, max err %.3e, bound %.3e" % (int(inner.sum()), float(err[inner].max()), 0.2 * half + rnd))
        assert inner.sum() > 1000 and (err[inner] <= 0.2 * half + rnd).all()
        pose = _pose((0.6, 0.3, -0.74), 23.0, (0.1234, -0.0567, 0.0891))
        nv, nb = dst.merge_from_posed(src, pose)
        k, p = dst.export(sorted=True, raw=True)
        assert nv == len(k) > 5000
        R = O.quat_to_R(pose[3:]).astype(np.float64)
        t = pose[:3].astype(np.float64)
        # f_P(x) = f(R^T (x - t)) = d0 + (R n) . t - (R n) . x
        Rn = R @ PLANE_N
        cK = k.astype(np.float64) * vs
        fK = d0 + Rn @ t - cK @ Rn
        dist = (p[:, 0] / p[:, 4]).astype(np.float64)
        rnd = 64 * max(float(np.abs(cK).max()), float(np.abs(skeys).max()) * vs) * 2.0 ** -24
        errK = np.abs(dist - fK)
        inner = np.abs(fK) < T - half
        edge = (np.abs(fK) < T) & ~inner
        print("plane: %d dst voxels, %d unclamped (max err %.3e, bound %.3e), %d near +-T (max err %.3e, bound %.3e)" % (
            len(k), int(inner.sum()), float(errK[inner].max()), 0.2 * half + rnd, int(edge.sum()), float(errK[edge].max(initial=0.0)), 1.2 * half + rnd))
        assert inner.sum() > 3000
        assert (errK[inner] <= 0.2 * half + rnd).all()
        assert (errK[edge] <= 1.2 * half + rnd).all()
        g = p[:, 1:4].astype(np.float64)
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        assert np.abs(g - (Rn / np.linalg.norm(Rn))[None, :]).max() <= 1e-6
    finally:
        src.close()
        dst.close()


# ---- 7. same call, same bytes ----------------------------------------------------------------------------------------------------
def test_same_call_same_bytes(pkg, pair):
    """twice into fresh contexts; with a source that was grown first; with a dst that has to grow inside the call"""
    gb = pair["gb"]
    outs = []
    ctxs = [_fresh(pkg, pair), _fresh(pkg, pair), _fresh(pkg, pair), _fresh(pkg, pair, cap=14), _fresh(pkg, pair, cap=CAP + 1)]
    try:
        a, b, c, small, src2 = ctxs
        src2.merge_raw(pair["bk"], pair["bp"])                       # B again (0 + x = x), in a table of twice the entries ...
        src2.grow(CAP + 2)                                           # ... and grown once more
        k2, p2 = src2.export(sorted=True, raw=True)
        assert _same(k2, pair["bk"]) and np.array_equal(p2, pair["bp"])
        small.set_auto_grow(22)
        for dst, src in ((a, gb), (b, gb), (c, src2), (small, gb)):
            counts = dst.merge_from_posed(src, SKEW)
            outs.append((counts,) + dst.export(sorted=True, raw=True))
        assert small.capacity_log2() > 14, "premise: the small dst grew inside the call"
        for o in outs[1:]:
            assert o[0] == outs[0][0] and _same(o[1], outs[0][1]) and _same(o[2], outs[0][2])
    finally:
        for g in ctxs:
            g.close()


# ---- 8. room ---------------------------------------------------------------------------------------------------------------------
def test_table_full_leaves_dst_unchanged(pkg, pair):
    dst = _fresh(pkg, pair, cap=14)                                  # 256 block entries
    try:
        dst.merge_raw(pair["bk"][:500], pair["bp"][:500])
        before = dst.export(sorted=True, raw=True)
        with pytest.raises(pkg.binding.GsdfError) as e:
            dst.merge_from_posed(pair["gb"], SKEW)
        assert e.value.code == ERR_TABLE_FULL and e.value.counts == (0, 0)
        after = dst.export(sorted=True, raw=True)
        assert _same(after[0], before[0]) and _same(after[1], before[1])
        assert _frames(dst) == 0 and dst.capacity_log2() == 14
    finally:
        dst.close()


def test_every_allocation_failing_in_turn_leaves_dst_unchanged(pkg, pair):
    """test library: the n-th owned allocation of the call fails, n = 1, 2, ... until the call succeeds; every failure is
    GSDF_ERR_HIP with dst's export unchanged in bytes, and the call that succeeds gives what a clean context gives"""
    L = pkg.binding.load_test_lib()
    src = _fresh(pkg, pair, lib=L)
    dst = _fresh(pkg, pair, lib=L)
    clean = _fresh(pkg, pair, lib=L)
    try:
        src.merge_raw(pair["bk"], pair["bp"])
        for g in (dst, clean):
            g.merge_raw(pair["bk"][:500], pair["bp"][:500])
        before = dst.export(sorted=True, raw=True)
        want_counts = clean.merge_from_posed(src, SKEW)
        want = clean.export(sorted=True, raw=True)
        failures = 0
        for n in range(1, 64):
            L.gsdf_debug_fail_alloc(n)
            try:
                counts = dst.merge_from_posed(src, SKEW)
                break
            except pkg.binding.GsdfError as e:
                L.gsdf_debug_fail_alloc(0)
                assert e.code == ERR_HIP, (n, e)
                failures += 1
                now = dst.export(sorted=True, raw=True)
                assert _same(now[0], before[0]) and _same(now[1], before[1]), n
                assert _frames(dst) == 0
        else:
            pytest.fail("the call never succeeded")
        L.gsdf_debug_fail_alloc(0)
        print("gsdf_merge_from_posed makes %d owned allocations" % failures)
        assert failures >= 5
        got = dst.export(sorted=True, raw=True)
        assert counts == want_counts and _same(got[0], want[0]) and _same(got[1], want[1])
    finally:
        L.gsdf_debug_fail_alloc(0)
        for g in (src, dst, clean):
            g.close()


# ---- 9. refusals and degenerate calls ----------------------------------------------------------------------------------------------
def test_refusals(pkg, pair):
    """every GSDF_ERR_INVALID case of the header that one device can show (two devices are not available to the suite)"""
    gb, L = pair["gb"], pair["gb"].L
    dst = _fresh(pkg, pair)
    others = []
    try:
        dst.merge_raw(pair["bk"][:500], pair["bp"][:500])
        before = dst.export(sorted=True, raw=True)
        p = SKEW.copy()
        fp = p.ctypes.data_as(C.POINTER(C.c_float))
        assert L.gsdf_merge_from_posed(None, gb.h, fp, None, None) == ERR_INVALID
        assert L.gsdf_merge_from_posed(dst.h, None, fp, None, None) == ERR_INVALID
        assert L.gsdf_merge_from_posed(dst.h, dst.h, fp, None, None) == ERR_INVALID
        assert L.gsdf_merge_from_posed(dst.h, gb.h, None, None, None) == ERR_INVALID

        def refused(d, s, pose=SKEW):
            with pytest.raises(pkg.binding.GsdfError) as e:
                d.merge_from_posed(s, pose)
            assert e.value.code == ERR_INVALID, e.value
        others.append(_fresh(pkg, pair, vs=f32(0.025)))
        refused(dst, others[-1])
        refused(others[-1], gb)
        others.append(_fresh(pkg, pair, T=f32(4) * pair["vs"]))
        refused(dst, others[-1])
        others.append(_fresh(pkg, pair, map_type=pkg.binding.MAP_BASE))
        refused(dst, others[-1])
        refused(others[-1], gb)
        others.append(_fresh(pkg, pair))
        others[-1].enable_vis(32)
        refused(dst, others[-1])
        refused(others[-1], gb)
        for i in range(7):
            for bad in (np.nan, np.inf, -np.inf):
                q = SKEW.copy()
                q[i] = bad
                refused(dst, gb, q)
        for scale in (np.sqrt(1 + 2e-4), np.sqrt(1 - 2e-4), 0.0):
            q = SKEW.copy()
            q[3:] = (q[3:].astype(np.float64) * scale).astype(f32)
            refused(dst, gb, q)
        q = SKEW.copy()
        q[3:] = (q[3:].astype(np.float64) * np.sqrt(1 + 5e-5)).astype(f32)      # inside the tolerance: accepted
        probe = _fresh(pkg, pair)
        others.append(probe)
        assert probe.merge_from_posed(gb, q)[0] > 0
        after = dst.export(sorted=True, raw=True)
        assert _same(after[0], before[0]) and _same(after[1], before[1]) and _frames(dst) == 0
    finally:
        dst.close()
        for g in others:
            g.close()


def test_empty_source(pkg, pair):
    dst, src = _fresh(pkg, pair), _fresh(pkg, pair)
    try:
        dst.merge_from(pair["ga"])
        before = dst.export(sorted=True, raw=True)
        assert dst.merge_from_posed(src, SKEW) == (0, 0)
        after = dst.export(sorted=True, raw=True)
        assert _same(after[0], before[0]) and _same(after[1], before[1]) and _frames(dst) == 8
    finally:
        dst.close()
        src.close()


def test_key_range(pkg, O, pair):
    """a translation that carries half of a small source across +2^20 voxels on x: GSDF_ERR_KEY_RANGE, the packable part merged and
    equal to the restatement (whose box ends at the range), the counts those of the packable part; dst is usable afterwards"""
    src, skeys, _ = _plane_src(pkg, pair)
    dst = _fresh(pkg, pair)
    try:
        vs = pair["vs"]
        pose = np.array([f32(2 ** 20 - 12 - int(PLANE_LO[0])) * vs, 0, 0, 0, 0, 0, 1], f32)    # x = 10 .. 33 -> 2^20 - 12 .. 2^20 + 11
        ek, ep, ck, cc = _expect(O, pair, src, skeys, dst, pose)
        assert 0 < len(ck) < len(skeys), "premise: part of the source stays packable"
        with pytest.raises(pkg.binding.GsdfError) as e:
            dst.merge_from_posed(src, pose)
        assert e.value.code == ERR_KEY_RANGE
        assert e.value.counts == (len(ck), ref.n_blocks(ck))
        k, p = dst.export(sorted=True, raw=True)
        assert _same(k, ek) and _same(p, ep)
        assert k[:, 0].max() == 2 ** 20 - 1
        d0, R0, t0 = pair["seq"].frame(0)
        dst.update(d0, R0, t0)
        _, _, w = dst.query((vs * k[:4].astype(f32)).astype(f32))
        assert (w > 0).all() and dst.count() > len(k)
    finally:
        src.close()
        dst.close()


# ---- 11. facade ---------------------------------------------------------------------------------------------------------------------
def test_merge_posed_selftest_matches_the_python_path(pkg, O, tmp_path):
    """host/merge_posed_selftest (MapGradPixelSdf::surface_cloud, RigidPointOptimizer::optimize_points,
    MapGradPixelSdf::merge_from(other, pose)) on the dumped stream of the 160x120 pair: counts and count() equal to the Python path
    under the pose the program recovered"""
    host = os.path.join(ROOT, "gradient-sdf_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "merge_posed_selftest"])
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=12, seed=1, step_deg=0.5)
    vs = f32(VS)
    T = f32(TRUNC) * vs
    frames = [seq.frame(i) for i in range(12)]
    np.asarray(seq.K, f32).reshape(9).tofile(tmp_path / "K.bin")
    np.stack([np.asarray(f[0], f32) for f in frames]).tofile(tmp_path / "depth.bin")
    P = np.zeros((12, 4, 4), f32)
    for i, (_, R, t) in enumerate(frames):
        P[i, :3, :3] = np.asarray(R, f32).reshape(3, 3)
        P[i, :3, 3] = t
        P[i, 3, 3] = 1
    P.tofile(tmp_path / "poses.bin")
    NEAR.tofile(tmp_path / "displace.bin")
    r = subprocess.run([os.path.join(host, "merge_posed_selftest"), str(tmp_path), str(W), str(H), "12", "0.02", "5", "0", "8", "4", "12", "1e-2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "merge_posed_selftest: OK" in r.stdout, r.stdout + r.stderr
    nv, nb, before, after = (int(v) for v in open(tmp_path / "merge.txt").read().split())
    pose = np.fromfile(tmp_path / "pose.bin", f32)
    assert pose.shape == (7,)
    # the Python path on the same stream: the facade hands over SE3(Matrix4f).rotationMatrix(), i.e. quaternion and back
    ga = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=CAP)
    gb = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=CAP)
    try:
        for i in range(8):
            d, R, t = frames[i]
            ga.update(d, O.quat_to_R(O.R_to_quat(R)), t)
        for i in range(4, 12):
            d, R, t = frames[i]
            gb.update(d, O.quat_to_R(O.R_to_quat(R)), t)
        assert ga.count() == before
        assert ga.merge_from_posed(gb, pose) == (nv, nb)
        assert ga.count() == after
    finally:
        ga.close()
        gb.close()
