"""gsdf_align_points_multi / gsdf_align_starts / gsdf_align_best without a GPU: the entries are declared, bound and exported; the
two host-only ones are run against the numpy restatement tests/align_multi_ref.py; and the premise of the GPU basin test
(tests/test_gpu_align_multi.py) is shown on the CPU oracle: a displacement a single start does not recover, and a 27-start
grid whose pick does."""
import ctypes as C
import os

import numpy as np
import pytest

import align_multi_ref as mref
import align_points_ref as ref
from conftest import ROOT

f32 = np.float32
NEW = ("gsdf_align_points_multi", "gsdf_align_points_multi_dev", "gsdf_align_starts", "gsdf_align_best")
CENTER = np.array([0.3, -0.2, 0.1, 0.1, -0.2, 0.3, 0.9], f32)          # |q| = 0.9747: normalised by the call
CENTER[3:] /= f32(np.sqrt((CENTER[3:].astype(np.float64) ** 2).sum()))
PIVOT = np.array([0.4, 0.1, 1.7], f32)
fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))                    # noqa: E731
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                    # noqa: E731


def test_entries_are_declared_bound_and_exported(pkg):
    L = pkg.binding.load()
    T = pkg.binding.load_test_lib()
    for name in NEW:
        assert name in pkg.binding.ABI_SYMBOLS
        assert hasattr(L, name) and hasattr(T, name)
        assert getattr(L, name).argtypes is not None
    for m in ("align_points_multi", "align_points_multi_dev"):
        assert callable(getattr(pkg.GradSdf, m))
    assert callable(pkg.binding.align_starts) and callable(pkg.binding.align_best)
    header = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    assert "#define GSDF_ALIGN_MAX_STARTS 1024" in header
    for name in NEW:
        assert "int %s(" % name in header


def test_null_context_is_refused(pkg):
    L = pkg.binding.load()
    for name in NEW[:2]:
        assert getattr(L, name)(None, None, 0, None, 1, 1, f32(1e-3), f32(1), None, None, None, None) == pkg.binding.ERR_INVALID


# ---- gsdf_align_starts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot_k,trans_k", [(0, 0), (0, 1), (1, 0), (1, 1), (2, 0)])
def test_starts_match_the_restatement(pkg, rot_k, trans_k):
    """count and index order exact; every value within one float ulp, 2^-23 max(1, |v|): both sides compute in double and round
    once, and libm's sin / cos may differ from numpy's in a last double bit"""
    rs, ts = f32(np.deg2rad(1.5)), f32(0.1)
    got = pkg.binding.align_starts(CENTER, PIVOT, rs, rot_k, ts, trans_k)
    want = mref.starts(CENTER, PIVOT, rs, rot_k, ts, trans_k)
    Rn, Tn = 2 * rot_k + 1, 2 * trans_k + 1
    assert got.shape == want.shape == (Rn ** 3 * Tn ** 3, 7)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = 2.0 ** -23 * np.maximum(1.0, np.abs(want.astype(np.float64)))
    print("(%d, %d): %d starts, %d values differ, worst err / bound %.3f" % (rot_k, trans_k, len(got), int((got != want).sum()),
                                                                             float((err / bound).max())))
    assert (err <= bound).all()
    # the middle index is the normalised centre
    mid = got[(len(got) - 1) // 2]
    qn = CENTER[3:].astype(np.float64)
    qn = (qn / np.sqrt((qn * qn).sum())).astype(f32)
    assert mid[:3].tobytes() == CENTER[:3].tobytes() and mid[3:].tobytes() == qn.tobytes()
    # the index order, from the definition: the offset of start h against the first start of its rotation
    h = np.arange(len(got))
    f, e, d = h % Tn, (h // Tn) % Tn, (h // Tn ** 2) % Tn
    off = got[:, :3].astype(np.float64) - got[(h // Tn ** 3) * Tn ** 3, :3]
    assert np.abs(off - float(ts) * np.stack([d, e, f], 1)).max() <= 1e-6
    assert all((got[i, 3:] == got[(i // Tn ** 3) * Tn ** 3, 3:]).all() for i in h)
    rot = got[::Tn ** 3, 3:]
    assert len({r.tobytes() for r in rot}) == Rn ** 3 and (rot[:, 3] > 0).all()


def test_starts_rotate_about_the_pivot(pkg):
    """every start maps the pivot to centre(pivot) + offset: the rotation is about the pivot"""
    got = pkg.binding.align_starts(CENTER, PIVOT, f32(0.05), 1, f32(0.2), 1).astype(np.float64)
    Rc = mref._quat_R(CENTER[3:].astype(np.float64))
    want0 = Rc @ PIVOT.astype(np.float64) + CENTER[:3]
    offs = set()
    for p in got:
        img = mref._quat_R(p[3:] / np.linalg.norm(p[3:])) @ PIVOT.astype(np.float64) + p[:3]
        o = img - want0
        assert np.abs(o / 0.2 - np.round(o / 0.2)).max() <= 1e-5 and np.abs(o).max() <= 0.2 + 1e-5
        offs.add(tuple(int(v) for v in np.round(o / 0.2)))
    assert len(offs) == 27


def test_starts_sizing_short_buffer_and_refusals(pkg):
    L = pkg.binding.load()
    INV = pkg.binding.ERR_INVALID
    m = C.c_int(-1)
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 1, f32(0.1), 1, None, 0, C.byref(m)) == 0 and m.value == 729
    buf = np.full((729, 7), 7.0, f32)
    m = C.c_int(-1)
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 1, f32(0.1), 1, fp(buf), 0, C.byref(m)) == 0 and m.value == 729
    assert (buf == 7.0).all()                                                   # max_m == 0: the sizing call
    m = C.c_int(-1)
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 1, f32(0.1), 1, fp(buf), 728, C.byref(m)) == INV
    assert m.value == 729 and (buf == 7.0).all()                                # one short: the need reported, nothing written
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 1, f32(0.1), 1, fp(buf), 729, C.byref(m)) == 0 and not (buf == 7.0).any()
    buf[:] = 7.0
    # 3^3 x 5^3 = 3 375 > GSDF_ALIGN_MAX_STARTS: refused, the count still reported
    m = C.c_int(-1)
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 1, f32(0.1), 2, None, 0, C.byref(m)) == INV and m.value == 3375
    # 2^3 ... the largest grid of one kind that fits: 5^3 x 1 = 125, 1 x 9^3 = 729, 1 x 11^3 = 1 331 does not
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 0, f32(0.1), 4, None, 0, C.byref(m)) == 0 and m.value == 729
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 0, f32(0.1), 5, None, 0, C.byref(m)) == INV and m.value == 1331
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 2 ** 30, f32(0.1), 2 ** 30, None, 0, C.byref(m)) == INV
    for bad in [dict(rot_k=-1), dict(trans_k=-1), dict(rs=np.nan), dict(ts=np.inf), dict(c=3, cv=np.nan), dict(c=0, cv=np.inf),
                dict(p=1, pv=-np.inf), dict(c=6, cv=0.95), dict(c=6, cv=0.90)]:         # the last two: |q| = 1.012, 0.990
        c, p = CENTER.copy(), PIVOT.copy()
        if "c" in bad:
            c[bad["c"]] = bad["cv"]
        if "p" in bad:
            p[bad["p"]] = bad["pv"]
        m = C.c_int(-1)
        rc = L.gsdf_align_starts(fp(c), fp(p), f32(bad.get("rs", 0.1)), bad.get("rot_k", 0), f32(bad.get("ts", 0.1)), bad.get("trans_k", 1),
                                 fp(buf), 729, C.byref(m))
        assert rc == INV and (buf == 7.0).all(), bad
    assert L.gsdf_align_starts(None, fp(PIVOT), f32(0.1), 0, f32(0.1), 0, fp(buf), 729, C.byref(m)) == INV
    assert L.gsdf_align_starts(fp(CENTER), None, f32(0.1), 0, f32(0.1), 0, fp(buf), 729, C.byref(m)) == INV
    assert L.gsdf_align_starts(fp(CENTER), fp(PIVOT), f32(0.1), 0, f32(0.1), 0, fp(buf), 729, None) == INV
    assert (buf == 7.0).all()
    # a norm 1e-4 off is still inside: |q| = 1 + 5e-5
    c = CENTER.copy()
    c[3:] *= f32(1.00005)
    assert L.gsdf_align_starts(fp(c), fp(PIVOT), f32(0.1), 0, f32(0.1), 0, fp(buf), 729, C.byref(m)) == 0 and m.value == 1


# ---- gsdf_align_best ----------------------------------------------------------------------------------------------------------
def _table(rows):
    """rows of (converged, passes, E, count)"""
    fl = np.array([r[0] for r in rows], np.int32)
    ps = np.array([r[1] for r in rows], np.int32)
    last = np.zeros((len(rows), 36), f32)
    last[:, 0] = [r[2] for r in rows]
    last[:, 28] = [r[3] for r in rows]
    return fl, ps, last


@pytest.mark.parametrize("rows,min_count,req,want", [
    # the smallest E / count among the eligible
    ([(1, 4, 8.0, 100), (1, 5, 3.0, 100), (1, 6, 5.0, 100)], 1, 1, 1),
    # a tie: the lowest index (2.0 / 100 == 4.0 / 200 in double)
    ([(1, 4, 9.0, 100), (1, 5, 4.0, 200), (1, 6, 2.0, 100), (1, 6, 2.0, 100)], 1, 1, 1),
    # min_count cuts the smallest score
    ([(1, 4, 0.001, 10), (1, 5, 3.0, 100), (1, 6, 2.0, 100)], 50, 1, 2),
    ([(1, 4, 0.001, 10), (1, 5, 3.0, 100), (1, 6, 2.0, 100)], 10, 1, 0),           # count == min_count is enough
    # require_converged on and off
    ([(0, 25, 1.0, 100), (1, 5, 3.0, 100)], 1, 1, 1),
    ([(0, 25, 1.0, 100), (1, 5, 3.0, 100)], 1, 0, 0),
    # E not finite; passes == 0
    ([(1, 4, np.nan, 100), (1, 5, np.inf, 100), (1, 0, 0.0, 100), (1, 6, 7.0, 100)], 1, 1, 3),
    # none eligible: -1, GSDF_OK
    ([(0, 25, 1.0, 100), (1, 0, 1.0, 100), (1, 3, np.nan, 100), (1, 3, 1.0, 5)], 50, 1, -1),
    ([(1, 3, 0.0, 0)], 0, 0, -1),                                                   # no hit: no score
    ([(1, 3, 0.0, 1)], 1, 1, 0),                                                    # E == 0 is a score
])
def test_best_on_hand_made_tables(pkg, rows, min_count, req, want):
    fl, ps, last = _table(rows)
    L = pkg.binding.load()
    best = C.c_int(-7)
    assert L.gsdf_align_best(len(rows), ip(fl), ip(ps), fp(last), min_count, req, C.byref(best)) == 0
    assert best.value == want
    assert pkg.binding.align_best(fl, ps, last, min_count, bool(req)) == want
    assert mref.best(fl, ps, last, min_count, bool(req)) == want


def test_best_refusals(pkg):
    L = pkg.binding.load()
    INV = pkg.binding.ERR_INVALID
    fl, ps, last = _table([(1, 4, 8.0, 100)])
    best = C.c_int(-7)
    assert L.gsdf_align_best(0, ip(fl), ip(ps), fp(last), 1, 1, C.byref(best)) == INV
    assert L.gsdf_align_best(1, None, ip(ps), fp(last), 1, 1, C.byref(best)) == INV
    assert L.gsdf_align_best(1, ip(fl), None, fp(last), 1, 1, C.byref(best)) == INV
    assert L.gsdf_align_best(1, ip(fl), ip(ps), None, 1, 1, C.byref(best)) == INV
    assert L.gsdf_align_best(1, ip(fl), ip(ps), fp(last), 1, 1, None) == INV
    assert best.value == -7


# ---- the premise of the GPU basin test, on the oracle ---------------------------------------------------------------------------
def test_single_start_misses_and_the_27_start_pick_recovers_on_the_oracle(pkg, O):
    """The 320x240 pair (1 cm, trunc 10; A = frames 0..7, B = frames 4..11) fused by the oracle; B's extract_pc cloud displaced
    by 2 degrees about (0.3, -0.5, 0.8) and (0.2, 0.2, -0.2) m.  Measured: the single start from the identity ends 17.3 degrees /
    68 mm off (with the converged flag set); of the 27 starts on the 0.1 m offset grid the pick is index 15, 0.19 degrees /
    1.3 mm off."""
    W, H = 320, 240
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=12, seed=1, step_deg=0.5)
    vs = f32(0.01)
    T = f32(10) * vs
    oa, ob = O.Oracle(vs, T, W, H, seq.K), O.Oracle(vs, T, W, H, seq.K)
    for i in range(8):
        oa.update(*seq.frame(i))
    for i in range(4, 12):
        ob.update(*seq.frame(i))
    cloud = ob.extract_pc()
    src, Rd, td = ref.displace(cloud[:, :3], rot_deg=2.0, tr=(0.2, 0.2, -0.2))
    n = len(src)
    assert 4000 < n < 10000
    c1, p1, u1, _ = ref.align(src, ref.IDENTITY, oa.query, O)
    ang1, terr1 = ref.pose_error(p1, Rd, td, O)
    print("single start: converged %s after %d passes, %.2f deg / %.1f mm off" % (c1, u1, ang1, 1e3 * terr1))
    assert ang1 > 5.0
    st = pkg.binding.align_starts(ref.IDENTITY, src.astype(np.float64).mean(axis=0), 0.0, 0, 0.1, 1)
    assert st.shape == (27, 7) and st[13].tobytes() == ref.IDENTITY.tobytes()
    runs = [ref.align(src, s, oa.query, O) for s in st]
    fl = np.array([r[0] for r in runs], np.int32)
    ps = np.array([r[2] for r in runs], np.int32)
    last = np.array([r[3][-1] for r in runs], f32)
    best = pkg.binding.align_best(fl, ps, last, n // 2, True)
    assert best == mref.best(fl, ps, last, n // 2, True) and best >= 0
    ang, terr = ref.pose_error(runs[best][1], Rd, td, O)
    print("27 starts: %d converged with >= n / 2 hits, pick %d: %.3f deg / %.2f mm off, %d hits of %d, %d passes" % (
        int(((fl != 0) & (last[:, 28] >= n // 2)).sum()), best, ang, 1e3 * terr, int(last[best, 28]), n, int(ps[best])))
    assert ang <= 0.3 and terr <= 0.5 * float(vs)
