"""gsdf_align_points / gsdf_surface_cloud without a GPU: the four entries are declared, bound and exported, and the numpy
restatement the GPU tests compare against (tests/align_points_ref.py) is pinned to the CPU oracle: over the back-projected
pixels of a depth frame the point loop IS the tracker's image loop (RigidPointOptimizer.cpp:62-69 make the points, :70-82 never
look at the image again)."""
import numpy as np
import pytest

import align_points_ref as ref
from conftest import pose7_from

NEW = ("gsdf_align_points", "gsdf_align_points_dev", "gsdf_surface_cloud", "gsdf_surface_cloud_dev")


def test_entries_are_declared_bound_and_exported(pkg):
    L = pkg.binding.load()
    T = pkg.binding.load_test_lib()
    for name in NEW:
        assert name in pkg.binding.ABI_SYMBOLS
        assert hasattr(L, name) and hasattr(T, name)
        assert getattr(L, name).argtypes is not None
    for m in ("align_points", "align_points_dev", "surface_cloud", "surface_cloud_dev"):
        assert callable(getattr(pkg.GradSdf, m))


def test_null_context_is_refused(pkg):
    L = pkg.binding.load()
    for name in NEW[:2]:
        assert getattr(L, name)(None, None, 0, None, 1, np.float32(1e-3), np.float32(1), None, None, None) == pkg.binding.ERR_INVALID
    for name in NEW[2:]:
        assert getattr(L, name)(None, None, 0, None) == pkg.binding.ERR_INVALID


@pytest.fixture(scope="module")
def frame8(pkg, O):
    """oracle map of frames 0..7 (160x120 spheres, 2 cm, trunc 5), frame 8's depth, frame 7's pose"""
    W, H = 160, 120
    seq = pkg.synth.Sequence("spheres", W, H, n_frames=12, seed=1, step_deg=0.5)     # 12: the stream the GPU tests take maps A and B from
    vs = np.float32(0.02)
    o = O.Oracle(vs, np.float32(5) * vs, W, H, seq.K)
    for i in range(8):
        o.update(*seq.frame(i))
    d8, _, _ = seq.frame(8)
    _, R7, t7 = seq.frame(7)
    return o, seq.K, d8, pose7_from(O, R7, t7)


@pytest.mark.parametrize("iters", [1, 3, 25])
def test_restatement_over_backprojected_pixels_is_the_oracle_tracker(O, frame8, iters):
    o, K, d8, p0 = frame8
    P = ref.backproject(d8, K)
    c1, q1, u1, tr1 = ref.align(P, p0, o.query, O, iters=iters)
    c2, q2, u2, tr2, hits = o.track(d8, p0, iters=iters)
    assert int(tr1[0, 28]) == int(hits[0]) > 1000                      # the same pixels hit the same voxels from the same pose
    assert (c1, u1) == (c2, u2), (c1, u1, c2, u2)
    print("iters %d: converged %s after %d passes, pose |d|max %.2e" % (iters, c1, u1, float(np.abs(q1 - q2).max())))
    assert np.abs(q1 - q2).max() <= 1e-4
    assert tr1.shape == (u1, 36)


def test_restatement_edge_rules(O, frame8):
    o, K, d8, p0 = frame8
    # no point: H = 0, xi NaN, never converged, the pose stays bit for bit
    c, q, u, tr = ref.align(np.zeros((0, 3), np.float32), p0, o.query, O, iters=4)
    assert not c and u == 4 and q.tobytes() == p0.tobytes() and np.isnan(tr[:, 29:35]).all() and (tr[:, 28] == 0).all()
    # rows that are not finite, far away or beyond the key range change nothing but n
    P = ref.backproject(d8, K)[::7]
    rng = np.random.default_rng(0)
    junk = np.concatenate([rng.uniform(-5, 5, (50, 3)) + 100.0, np.full((3, 3), 3e4), [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf]]]).astype(np.float32)
    S0, A0, t0 = ref.pass_sums(P, p0, o.query, O)
    S1, A1, t1 = ref.pass_sums(np.concatenate([junk, P]), p0, o.query, O)
    assert t0.tobytes() == t1.tobytes() and np.array_equal(S0, S1)
    # iters = 0
    c, q, u, tr = ref.align(P, p0, o.query, O, iters=0)
    assert not c and u == 0 and tr.shape == (0, 36)
