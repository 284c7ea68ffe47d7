"""The restatement tests/erase_ref.py on hand-made maps of a few voxels, and the new entries' presence in header, library and
binding (no GPU): closed box faces, the half-open weight interval, the equality case of the points predicate, the four ops,
invert, erase's counts."""
import os
import re

import numpy as np

import erase_ref as E
from conftest import ROOT

f32 = np.float32
VS = f32(0.02)
NEW = ["gsdf_select_box", "gsdf_select_weight", "gsdf_select_points", "gsdf_select_points_dev", "gsdf_select_invert",
       "gsdf_select_clear", "gsdf_select_count", "gsdf_select_export", "gsdf_select_export_raw_dev", "gsdf_erase_selected",
       "gsdf_compact"]


def _map(keys, w=None):
    keys = np.asarray(keys, np.int32).reshape(-1, 3)
    pay = np.zeros((len(keys), 5), f32)
    pay[:, 4] = 1 if w is None else np.asarray(w, f32)
    order = np.argsort(E.pack(keys))
    return keys[order], pay[order]


def test_entries_are_declared_exported_and_bound(pkg):
    L, T = pkg.binding.load(), pkg.binding.load_test_lib()
    header = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    for name in NEW:
        assert name in pkg.binding.ABI_SYMBOLS
        assert hasattr(L, name) and hasattr(T, name)
        assert getattr(L, name).argtypes is not None
        assert "int %s(" % name in header
    for i, op in enumerate(("REPLACE", "ADD", "INTERSECT", "SUBTRACT")):
        assert re.search(r"#define GSDF_SEL_%s\s+%d\b" % (op, i), header)
        assert getattr(pkg.binding, "SEL_" + op) == i == getattr(E, op) == getattr(pkg, "SEL_" + op)
    for m in ("select_box", "select_weight", "select_points", "select_points_dev", "select_invert", "select_clear", "select_count",
              "select_export", "select_export_raw_dev", "erase_selected", "compact", "crop", "prune"):
        assert callable(getattr(pkg.GradSdf, m))


def test_null_context_is_refused(pkg):
    L, INV = pkg.binding.load(), pkg.binding.ERR_INVALID
    assert L.gsdf_select_box(None, None, None, 0, None) == INV
    assert L.gsdf_select_weight(None, f32(0), f32(1), 0, None) == INV
    assert L.gsdf_select_points(None, None, 0, None, f32(0), 0, None) == INV
    assert L.gsdf_select_points_dev(None, None, 0, None, f32(0), 0, None) == INV
    assert L.gsdf_select_invert(None, None) == INV and L.gsdf_select_clear(None) == INV
    assert L.gsdf_select_count(None, None, None) == INV
    assert L.gsdf_select_export(None, None, None, 0, None, 0) == INV
    assert L.gsdf_select_export_raw_dev(None, None, None, 0, None) == INV
    assert L.gsdf_erase_selected(None, None, None) == INV and L.gsdf_compact(None, 0, None) == INV


def test_box_faces_are_closed():
    keys, _ = _map([[i, 0, 0] for i in range(-3, 8)])
    lo = [VS * f32(-1), VS * f32(0), VS * f32(0)]                 # faces ON voxel centres: the closed comparison decides
    hi = [VS * f32(5), VS * f32(0), VS * f32(0)]
    m = E.box(keys, VS, lo, hi)
    assert keys[m][:, 0].tolist() == [-1, 0, 1, 2, 3, 4, 5]
    below, above = np.nextafter(f32(lo[0]), f32(1)), np.nextafter(f32(hi[0]), f32(-1))
    assert keys[E.box(keys, VS, [below, lo[1], lo[2]], [above, hi[1], hi[2]])][:, 0].tolist() == [0, 1, 2, 3, 4]
    assert not E.box(keys, VS, hi, lo).any()                      # inverted on x: empty
    inf = f32(np.inf)
    assert E.box(keys, VS, [-inf] * 3, [inf] * 3).all()


def test_weight_interval_is_half_open():
    keys, pay = _map([[i, 1, -2] for i in range(5)], w=[0.5, 4.9999995, 5, 7, 5])
    assert E.weight(pay, 0, 5).tolist() == [True, True, False, False, False]
    assert E.weight(pay, 5, np.inf).tolist() == [False, False, True, True, True]
    assert (E.weight(pay, 0, 5) ^ E.weight(pay, 5, np.inf)).all()
    w = f32(7)
    assert E.weight(pay, w, np.nextafter(w, f32(np.inf))).tolist() == [False, False, False, True, False]


def test_points_equality_case():
    """the point sits on voxel i, the radius is the float distance to voxel i + 2: that voxel is at exact equality and in; with
    the next float below it is out"""
    i = 37
    keys, _ = _map([[i + d, -4, 9] for d in range(-4, 5)])
    p = np.array([VS * f32(i), VS * f32(-4), VS * f32(9)], f32)
    r = f32(f32(VS * f32(i + 2)) - p[0])
    assert r > 0
    m = E.points(keys, VS, [p], r)
    assert m[keys[:, 0] == i + 2].all() and not m[keys[:, 0] == i + 3].any()
    m = E.points(keys, VS, [p], np.nextafter(r, f32(0)))
    assert not m[keys[:, 0] == i + 2].any() and m[keys[:, 0] == i + 1].all()
    assert E.points(keys, VS, [p], 0).sum() == 1                  # radius 0: the voxel the point sits on


def test_points_skip_nonfinite_and_count_once(O):
    keys, _ = _map([[x, y, 0] for x in range(4) for y in range(4)])
    p = np.array([[0.02, 0.02, 0], [0.02, 0.02, 0], [np.nan, 0, 0], [np.inf, 0, 0]], f32)
    m = E.points(keys, VS, p, VS)
    assert m.sum() == 5 and m.dtype == bool                       # the centre and its four axis neighbours, once
    assert not E.points(keys, VS, np.zeros((0, 3), f32), VS).any()
    ident = np.array([0, 0, 0, 0, 0, 0, 1], f32)
    assert np.array_equal(E.points(keys, VS, p, VS, ident, O), m)
    shift = np.array([0.02, 0, 0, 0, 0, 0, 1], f32)
    assert keys[E.points(keys, VS, p[:1], 0, shift, O)].tolist() == [[2, 1, 0]]


def test_ops_invert_and_erase():
    keys, pay = _map([[x, 0, z] for x in range(8) for z in range(2)])
    A = keys[:, 0] < 5
    B = keys[:, 0] >= 3
    assert np.array_equal(E.combine(E.REPLACE, A, B), B)
    assert np.array_equal(E.combine(E.ADD, A, B), A | B) and E.combine(E.ADD, A, B).all()
    assert keys[E.combine(E.INTERSECT, A, B)][:, 0].tolist() == [3, 4, 3, 4]
    assert sorted(set(keys[E.combine(E.SUBTRACT, A, B)][:, 0].tolist())) == [0, 1, 2]
    for op in (E.INTERSECT, E.SUBTRACT):
        assert not E.combine(op, None, B).any()                   # no selection: the empty set
    assert np.array_equal(E.combine(E.ADD, None, B), B)
    assert np.array_equal(E.invert(A, len(keys)), ~A) and E.invert(None, len(keys)).all()
    k2, p2, nv, nb = E.erase(keys, pay, keys[:, 0] < 4)           # block (0, 0, 0) goes, block (1, 0, 0) stays
    assert (nv, nb) == (8, 1) and np.array_equal(k2, keys[keys[:, 0] >= 4]) and len(p2) == 8
    k3, _, nv, nb = E.erase(keys, pay, keys[:, 0] < 3)            # block (0, 0, 0) keeps x = 3
    assert (nv, nb) == (6, 0) and len(k3) == 10
    assert len(E.blocks(keys)) == 2 and len(E.blocks([[-1, 0, 0], [-4, 3, 3], [-5, 0, 0]])) == 2
