"""The robust registration without a GPU (include/gsdf.h: gsdf_align_loss_weight, gsdf_align_points_robust[_dev],
gsdf_align_points_multi_robust[_dev], gsdf_align_best_robust, gsdf_align_residuals[_dev]): the entries are declared, bound and
exported; the weight function equals the numpy restatement (tests/align_robust_ref.py) in bits; the pick equals a numpy pick;
with loss = 0 the restatement is tests/align_points_ref.py's in bytes; and on a pair of sessions in which one sphere moved the
Tukey run ends at most half as far off as the plain one."""
import ctypes as C

import numpy as np
import pytest

import align_points_ref as ref
import align_robust_ref as rref
from conftest import pose7_from

f32 = np.float32
NEW = ("gsdf_align_loss_weight", "gsdf_align_points_robust", "gsdf_align_points_robust_dev", "gsdf_align_points_multi_robust",
       "gsdf_align_points_multi_robust_dev", "gsdf_align_best_robust", "gsdf_align_residuals", "gsdf_align_residuals_dev")


# ---- 1. declared, bound, exported ---------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported(pkg):
    L = pkg.binding.load()
    T = pkg.binding.load_test_lib()
    for name in NEW:
        assert name in pkg.binding.ABI_SYMBOLS
        assert hasattr(L, name) and hasattr(T, name)
        assert getattr(L, name).argtypes is not None
    for m in ("align_points_robust", "align_points_robust_dev", "align_points_multi_robust", "align_points_multi_robust_dev",
              "align_residuals", "align_residuals_dev"):
        assert callable(getattr(pkg.GradSdf, m))
    assert callable(pkg.binding.align_loss_weight) and callable(pkg.binding.align_best_robust)


def test_null_arguments_are_refused(pkg):
    L, INV = pkg.binding.load(), pkg.binding.ERR_INVALID
    for name in NEW[1:3]:
        assert getattr(L, name)(None, None, 0, None, 1, f32(1e-3), f32(1), 3, f32(0.02), None, None, None) == INV
    for name in NEW[3:5]:
        assert getattr(L, name)(None, None, 0, None, 1, 1, f32(1e-3), f32(1), 3, f32(0.02), None, None, None, None) == INV
    for name in NEW[6:]:
        assert getattr(L, name)(None, None, 0, None, None, None) == INV
    assert L.gsdf_align_loss_weight(3, f32(0.02), f32(0.01), None) == INV
    one, best = np.ones(1, np.int32), C.c_int(7)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                  # noqa: E731
    row = np.ones(38, f32)
    fp = row.ctypes.data_as(C.POINTER(C.c_float))
    assert L.gsdf_align_best_robust(0, ip(one), ip(one), fp, f32(1), 1, C.byref(best)) == INV
    assert L.gsdf_align_best_robust(1, None, ip(one), fp, f32(1), 1, C.byref(best)) == INV
    assert L.gsdf_align_best_robust(1, ip(one), None, fp, f32(1), 1, C.byref(best)) == INV
    assert L.gsdf_align_best_robust(1, ip(one), ip(one), None, f32(1), 1, C.byref(best)) == INV
    assert L.gsdf_align_best_robust(1, ip(one), ip(one), fp, f32(1), 1, None) == INV
    assert best.value == 7


# ---- 2. the weight function ---------------------------------------------------------------------------------------------------
def _phis(k, T):
    """about 1e5 distances: a dense random set over +-2 T, and the values at which a branch or a rounding can go wrong"""
    rng = np.random.default_rng(11)
    k = f32(k)
    edge = [0.0, -0.0, k, -k, np.nextafter(k, f32(0)), np.nextafter(k, f32(np.inf)), -np.nextafter(k, f32(0)),
            -np.nextafter(k, f32(np.inf)), T, -T, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, 1.17549435e-38,
            3.4028235e38, -3.4028235e38, 1e19, 1e20]
    dense = rng.uniform(-2 * float(T), 2 * float(T), 90000)
    near = float(k) * (1 + rng.uniform(-1e-5, 1e-5, 5000)) * rng.choice([-1.0, 1.0], 5000)
    tiny = rng.uniform(-1, 1, 5000) * 10.0 ** rng.uniform(-44, -30, 5000)
    return np.concatenate([np.array(edge, f32), dense.astype(f32), near.astype(f32), tiny.astype(f32)]).astype(f32)


@pytest.mark.parametrize("loss", [0, 1, 2, 3, 4])
def test_loss_weight_equals_the_restatement_in_bits(pkg, loss):
    vs = f32(0.01)
    T = f32(10) * vs
    for k in (f32(0.5) * vs, f32(2) * vs, T):
        phi = _phis(k, T)
        got = pkg.binding.align_loss_weight(loss, k, phi)
        want = rref.weight(loss, k, phi)
        same = got.view(np.uint32) == want.view(np.uint32)
        assert same.all(), (loss, float(k), phi[~same][:5], got[~same][:5], want[~same][:5])
        assert len(phi) > 100000 - 1 and np.isfinite(got[np.isfinite(phi)]).all()
    if loss in (3, 4):                                                     # the cut is at |phi| = k exactly, k itself outside
        w = pkg.binding.align_loss_weight(loss, f32(0.02), np.array([f32(0.02), np.nextafter(f32(0.02), f32(0))], f32))
        assert w[0] == 0 and w[1] > 0
    # NaN in, per the table: NaN for CAUCHY and HUBER, 0 for TUKEY and TRUNC_L2, 1 for L2
    w = pkg.binding.align_loss_weight(loss, f32(0.02), np.array([np.nan], f32))[0]
    assert (w == 1) if loss == 0 else (np.isnan(w) if loss in (1, 2) else w == 0)


def test_loss_weight_refuses_bad_loss_and_scale(pkg):
    L, INV = pkg.binding.load(), pkg.binding.ERR_INVALID
    w = C.c_float(7)
    for loss in (-1, 5, 100):
        assert L.gsdf_align_loss_weight(loss, f32(0.02), f32(0.01), C.byref(w)) == INV
    for loss in (1, 2, 3, 4):
        for scale in (0.0, -0.02, np.nan, np.inf, -np.inf):
            assert L.gsdf_align_loss_weight(loss, f32(scale), f32(0.01), C.byref(w)) == INV, (loss, scale)
    assert w.value == 7
    for scale in (0.0, -1.0, np.nan, np.inf):                              # L2 ignores the scale
        assert L.gsdf_align_loss_weight(0, f32(scale), f32(0.01), C.byref(w)) == 0 and w.value == 1


# ---- 3. the pick --------------------------------------------------------------------------------------------------------------
def test_best_robust_against_a_numpy_pick(pkg):
    def rows(*ew):
        r = np.zeros((len(ew), 38), f32)
        for h, (E, wsum) in enumerate(ew):
            r[h, 0], r[h, 36], r[h, 28] = E, wsum, 1000.0
        return r
    pick = pkg.binding.align_best_robust
    cases = [
        # (converged, passes, rows, min_wsum, require_converged)
        ([1, 1, 1], [4, 4, 4], rows((2.0, 100), (1.0, 100), (3.0, 100)), 50, True),
        ([1, 1, 1], [4, 4, 4], rows((2.0, 100), (1.0, 50), (4.0, 200)), 50, True),          # a tie of 0.02: the lowest index
        ([1, 1, 1], [4, 4, 4], rows((2.0, 100), (0.1, 49.5), (3.0, 100)), 50, True),        # the best score below the floor
        ([1, 1, 1], [4, 4, 4], rows((np.inf, 100), (np.nan, 100), (3.0, 100)), 50, True),   # E not finite
        ([0, 1, 0], [25, 4, 25], rows((0.1, 100), (1.0, 100), (0.2, 100)), 50, True),       # not converged
        ([0, 1, 0], [25, 4, 25], rows((0.1, 100), (1.0, 100), (0.2, 100)), 50, False),
        ([1, 1], [0, 4], rows((0.1, 100), (1.0, 100)), 50, True),                           # no pass executed
        ([1, 1], [4, 4], rows((1.0, 0.0), (1.0, np.nan)), 0, True),                         # no weight at all: none eligible
        ([0, 0], [25, 25], rows((1.0, 100), (1.0, 100)), 50, True),                         # none eligible
        ([1, 1], [4, 4], rows((1.0, 10), (1.0, 20)), 50, True),                             # none eligible: all below the floor
    ]
    want = [1, 0, 0, 2, 1, 0, 1, -1, -1, -1]
    for (c, p, r, floor, req), w in zip(cases, want):
        got = pick(c, p, r, floor, req)
        assert got == rref.best(c, p, r, floor, req) == w, (c, p, floor, req, got, w)


# ---- 4. loss = 0 is the plain restatement -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame8(pkg, O):
    """test_align_points.py's set: oracle map of frames 0..7 (160x120 spheres, 2 cm, trunc 5), frame 8's depth, frame 7's pose"""
    W, H = 160, 120
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=12, seed=1, step_deg=0.5)
    vs = f32(0.02)
    o = O.Oracle(vs, f32(5) * vs, W, H, seq.K)
    for i in range(8):
        o.update(*seq.frame(i))
    d8, _, _ = seq.frame(8)
    _, R7, t7 = seq.frame(7)
    return o, seq.K, d8, pose7_from(O, R7, t7)


@pytest.mark.parametrize("iters", [1, 3, 25])
def test_loss_0_restatement_is_the_plain_restatement_in_bytes(O, frame8, iters):
    o, K, d8, p0 = frame8
    P = ref.backproject(d8, K)
    c1, q1, u1, tr1 = ref.align(P, p0, o.query, O, iters=iters)
    c2, q2, u2, tr2 = rref.align(P, p0, o.query, O, loss=0, scale=0.0, iters=iters)
    assert (c1, u1) == (c2, u2) and q1.tobytes() == q2.tobytes()
    assert tr2.shape == (u2, 38) and tr2[:, :36].tobytes() == tr1.tobytes()
    assert (tr2[:, 36] == tr2[:, 28]).all() and (tr2[:, 37] == tr2[:, 28]).all() and tr2[0, 28] > 1000
    S1, A1, t1 = ref.pass_sums(P, p0, o.query, O)
    S2, A2, t2 = rref.pass_sums(P, p0, o.query, O)
    assert np.array_equal(S1, S2[:29]) and np.array_equal(A1, A2[:29]) and t1.tobytes() == t2[:29].tobytes()


# ---- 5. the demonstration scene -----------------------------------------------------------------------------------------------
def test_tukey_halves_the_error_when_a_sphere_moved(pkg, O):
    """Sessions A (frames 0..7) and B (frames 4..11) of the 320x240 spheres stream at 1 cm voxels, trunc 10; in session B the third
    sphere stands (0.04, -0.02, 0.012) m elsewhere.  B's cloud, displaced by align_points_ref.displace's defaults, is registered
    against A from the identity with default arguments: the Tukey run at 2 cm converges, and its rotation and translation errors
    are each at most half the plain run's."""
    W, H = 320, 240
    args = dict(n_frames=12, seed=1, step_deg=0.5)
    seq_a = pkg.synth.Sequence("spheres", W, H, **args)
    seq_b = pkg.synth.Sequence("spheres", W, H, **args)
    seq_b.spheres = np.array(seq_b.spheres, np.float64).copy()
    seq_b.spheres[2, :3] += (0.04, -0.02, 0.012)
    vs = f32(0.01)
    T = f32(10) * vs
    A, B = O.Oracle(vs, T, W, H, seq_a.K), O.Oracle(vs, T, W, H, seq_b.K)
    for i in range(8):
        A.update(*seq_a.frame(i))
    for i in range(4, 12):
        B.update(*seq_b.frame(i))
    cloud = B.extract_pc()
    src, Rd, td = ref.displace(cloud[:, :3])
    c2, p2, u2, _ = ref.align(src, ref.IDENTITY, A.query, O)
    ct, pt, ut, trt = rref.align(src, ref.IDENTITY, A.query, O, loss=rref.TUKEY, scale=0.02)
    a2, t2 = ref.pose_error(p2, Rd, td, O)
    at, tt = ref.pose_error(pt, Rd, td, O)
    print("%d points.  L2: converged %s after %d passes, %.3f deg / %.2f mm off.  Tukey 2 cm: converged %s after %d passes, "
          "%.3f deg / %.2f mm off, %d of %d hits with weight > 0" % (len(src), c2, u2, a2, 1e3 * t2, ct, ut, at, 1e3 * tt,
                                                                      int(trt[-1, 37]), int(trt[-1, 28])))
    assert ct
    assert at <= 0.5 * a2 and tt <= 0.5 * t2
