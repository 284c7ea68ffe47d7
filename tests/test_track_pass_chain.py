"""k_track_pass with the short tail: the folding wave reduction (wave_sum_fold, one LDS write per wave) against the reduction of
rounds 1-6, which the test build keeps behind tracker debug bit 8 (wave_sum_to_lane63 + 29 LDS writes of lane 63).

CPU: the lane-level model of both reduction trees (track_reduce_model.py) -- the same additions on the same operand pairs, so the
same float32 words.  GPU: frame-log rows and poses of tracked streams, old route against new, as float32 words.  The frames are
small on purpose: up to 16 workgroups, one per group row of partial sums, so that no sum depends on the order of atomics and
a run is reproducible to the bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_reduce_model as M  # noqa: E402
from conftest import pose7_from  # noqa: E402

OLD_ROUTE = 8 << 16                  # tracker debug bit: the reduction of rounds 1-6
FEW_BLOCKS = 32 << 16                # at most 4 tracker workgroups: a workgroup loops over several batches of pixels


def _adversarial(rng):
    """64-lane vectors of mixed magnitudes, signed zeros, denormals, inf and NaN; 29 values per case"""
    f = np.float32
    den = f(1e-45)
    picks = np.array([0.0, -0.0, den, -den, f(1.2e-38), f(-3e-39), 1.0, -1.0, f(1 + 2 ** -23), f(16777216.0), f(-16777217.0),
                      f(3.4e38), f(-3.4e38), f(1e-30), f(1e30), f(-1e30), np.inf, -np.inf, np.nan], np.float32)
    cases = []
    cases.append(picks[rng.integers(0, len(picks), (200, 29, 64))])                      # everything, inf - inf and NaN included
    cases.append(picks[rng.integers(0, 16, (200, 29, 64))])                              # finite only: cancellation, overflow to inf
    cases.append(picks[rng.integers(0, 6, (100, 29, 64))])                               # zeros and denormals only
    big = np.zeros((64, 29, 64), np.float32)                                             # one large value in lane l, ones elsewhere
    big[:] = 1.0
    big[np.arange(64), :, np.arange(64)] = f(16777216.0)
    cases.append(big)
    one_nan = rng.standard_normal((64, 29, 64)).astype(np.float32)                       # one NaN / one inf per vector, every lane once
    one_nan[np.arange(64), ::2, np.arange(64)] = np.nan
    one_nan[np.arange(64), 1::2, np.arange(64)] = np.inf
    cases.append(one_nan)
    alt = np.where(np.arange(64) % 2 == 0, f(1e8), f(-1e8)) + rng.standard_normal((50, 29, 64)).astype(np.float32)
    cases.append(alt.astype(np.float32))
    return cases


def test_fold_tree_is_the_lane63_tree_bit_for_bit():
    """wave_sum_fold performs the additions of wave_sum_to_lane63: the balanced tree over adjacent lanes of a row of 16, then
    row 0 + row 1 and row 2 + row 3, then those two.  >= 1e5 random 64-lane vectors of widely mixed magnitudes plus the
    adversarial ones; equal as float32 words (a NaN for a NaN)."""
    rng = np.random.default_rng(7)
    v = (rng.standard_normal((4000, 29, 64)) * np.exp(rng.uniform(-30, 30, (4000, 29, 64)))).astype(np.float32)
    assert v.shape[0] * v.shape[1] >= 100000
    a, b = M.wave_sum_to_lane63(v), M.wave_sum_fold(v)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the tree itself, written out for one vector per value
    x = v[0]
    y = x.reshape(29, 4, 16)
    while y.shape[-1] > 1:
        y = (y[..., 0::2] + y[..., 1::2]).astype(np.float32)
    y = y[..., 0]
    ref = ((y[:, 0] + y[:, 1]).astype(np.float32) + (y[:, 2] + y[:, 3]).astype(np.float32)).astype(np.float32)
    assert np.array_equal(ref.view(np.uint32), a[0].view(np.uint32))
    for c in _adversarial(rng):
        a, b = M.wave_sum_to_lane63(c), M.wave_sum_fold(c)
        assert M.same_bits(a, b)
        fin = np.isfinite(c).all(axis=-1)                     # finite inputs: no NaN to be lenient about
        assert np.array_equal(a[fin].view(np.uint32), b[fin].view(np.uint32))
    # fewer than 29 values, and exactly 32
    for n in (1, 3, 17, 32):
        w = rng.standard_normal((50, n, 64)).astype(np.float32)
        assert np.array_equal(M.wave_sum_to_lane63(w).view(np.uint32), M.wave_sum_fold(w).view(np.uint32))


def test_fold_totals_land_in_the_lanes_the_kernel_writes_from():
    """lane l < 32 ends with value bitrev5(l): the index k_track_pass writes wsum[wave][.] at"""
    v = np.zeros((1, 29, 64), np.float32)
    v[0, :, :] = (np.arange(29, dtype=np.float32) + 1)[:, None] / 64
    tot = M.wave_sum_fold(v)[0]
    assert np.array_equal(tot, np.arange(29, dtype=np.float32) + 1)
    assert sorted(M.bitrev5(l) for l in range(32)) == list(range(32))


# ---------------------------------------------------------------------------------------------------------------------------------
def _frames(pkg, W, H, n, holes_at=None):
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=1)
    frames = [seq.frame(i) for i in range(n)]
    if holes_at is not None:                                   # depth 0, NaN, below zmin, above zmax
        d = frames[holes_at][0].copy().reshape(H, W)
        flat = d.reshape(-1)
        flat[0::7] = 0.0
        flat[3::11] = 0.1
        flat[5::13] = 9.0
        flat[(W * H) // 2 + 1] = np.nan
        flat[W * H - 1] = np.nan
        frames[holes_at] = (d, frames[holes_at][1], frames[holes_at][2])
    return seq, frames


def _run_stream(pkg, O, L, seq, frames, flags, ahead=False, vs=0.04, conv=0.02):
    """first frame fused at its pose, the others tracked and fused: (frame-log rows, final pose, keys, payloads)"""
    vs = np.float32(vs)
    g = pkg.GradSdf(vs, np.float32(5) * vs, seq.W, seq.H, seq.K, capacity_log2=18, lib=L)
    g.debug_flags(flags)
    d0, R0, t0 = frames[0]
    p = pose7_from(O, R0, t0)
    g.update(d0, O.quat_to_R(p[3:]), t0)
    g.set_pose(p)
    dev = [g.upload(f[0]) for f in frames]
    for i in range(1, len(frames)):
        if ahead:
            g.track_and_fuse_ahead_dev(dev[i], dev[i + 1] if i + 1 < len(frames) else None, conv=conv)
        else:
            g.track_and_fuse_dev(dev[i], conv=conv)
    g.sync()
    log = g.frame_log().copy()
    pose = g.get_pose().copy()
    keys, pay = g.export(sorted=True)
    g.close()
    return log, pose, keys, pay


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# (voxel size: about a pixel's footprint, so that the tracked points find voxels; threshold: where the CPU oracle's optimize() ends
# within a few passes on some of these frames and not at all on others)
CASES = {
    "48x36": dict(W=48, H=36, vs=0.06, conv=0.03),             # width below a wave's row of 64: x / y stepping wraps inside a batch
    "100x75": dict(W=100, H=75, vs=0.04, conv=0.02),           # N no multiple of 64 or 1280: last workgroup partly empty, waves without a pixel
    "64x1": dict(W=64, H=1, vs=0.06, conv=0.03),
    "160x120-few-blocks": dict(W=160, H=120, vs=0.02, conv=0.01, extra=FEW_BLOCKS),   # 15 chunks on 4 workgroups: the loop over batches
    "100x75-holes": dict(W=100, H=75, vs=0.04, conv=0.02, holes_at=5),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_new_route_gives_the_old_route_words(pkg, O, case):
    """Frame-log rows (pose7, converged, passes, n_hit) and gsdf_get_pose after a tracked stream of 12 frames: the folding
    reduction against wave_sum_to_lane63, as float32 words."""
    c = CASES[case]
    L = pkg.binding.load_test_lib()
    seq, frames = _frames(pkg, c["W"], c["H"], 13, c.get("holes_at"))
    extra = c.get("extra", 0)
    kw = dict(vs=c["vs"], conv=c["conv"])
    old = _run_stream(pkg, O, L, seq, frames, OLD_ROUTE | extra, **kw)
    new = _run_stream(pkg, O, L, seq, frames, extra, **kw)
    print("MEASURED %s: passes %s, converged %s, n_hit %s" % (case, old[0][:, 8].astype(int).tolist(), old[0][:, 7].astype(int).tolist(),
                                                              old[0][:, 9].astype(int).tolist()))
    assert old[0].shape == (12, 10)
    assert np.array_equal(_words(old[0]), _words(new[0])), (old[0], new[0])
    assert np.array_equal(_words(old[1]), _words(new[1]))
    assert (old[0][:, 9] > 0).any(), "the stream should track: pixels that find a voxel"


@pytest.mark.gpu
def test_exact_head_paths_old_route_against_new(pkg, O):
    """The out-of-line exact forms of the head: an empty map (every pivot zero: the exact llt) and a start pose 0.2 rad off (a
    rotation step above 0.1 rad: the exact SE3::exp), one and three passes each, and a full optimize(): old route against new as
    float32 words, in ONE context (the routes are switched between the calls), so both see the same map to the bit."""
    L = pkg.binding.load_test_lib()
    seq, frames = _frames(pkg, 100, 75, 2)
    vs = np.float32(0.04)
    g = pkg.GradSdf(vs, np.float32(5) * vs, seq.W, seq.H, seq.K, capacity_log2=18, lib=L)
    d0, R0, t0 = frames[0]
    p0 = pose7_from(O, R0, t0)
    start = O.se3_exp_mul(np.array([0.01, -0.01, 0.0, 0.0, 0.2, 0.0], np.float32), p0)

    def both(depth, pose, iters):
        res = []
        for flags in (OLD_ROUTE, 0):
            g.debug_flags(flags)
            res.append(g.track(depth, pose, iters=iters))
        (ca, pa, na), (cb, pb, nb) = res
        assert (ca, na) == (cb, nb) and np.array_equal(_words(pa), _words(pb)), (iters, pa, pb)
        return res[0]

    both(d0, p0, 1)                                                             # empty map: zero pivots
    g.update(d0, O.quat_to_R(p0[3:]), t0)
    _, moved, _ = both(d0, start, 1)
    assert not np.array_equal(moved, start)                                     # the 0.2 rad start did move the pose
    both(d0, start, 3)
    both(frames[1][0], p0, 25)
    g.debug_flags(0)
    g.close()


@pytest.mark.gpu
def test_plain_and_hinted_route_agree(pkg, O):
    """gsdf_track_and_fuse_dev and ..._ahead_dev on 100 x 75: the closing head inside k_fuse<.., HEAD> is the head of
    k_track_pass -- same log rows, same map.  "Same" between two RUNS of the frame loop is what the suite's other tests of the two
    routes take it to be (test_next_depth_hint_is_invisible_except_in_time): pass counts, flags and keys identical, poses within
    1e-6 and sums within 1e-5 of the largest -- the deferred contributions of a fusion launch are float atomics in free order, so
    two runs of one and the same route already differ in the last bits of a few voxels (measured here: poses and rows identical
    words in both of two runs, payloads in one of them)."""
    L = pkg.binding.load_test_lib()
    seq, frames = _frames(pkg, 100, 75, 13)
    (la, pa7, ka, pa) = _run_stream(pkg, O, L, seq, frames, 0)
    (lb, pb7, kb, pb) = _run_stream(pkg, O, L, seq, frames, 0, ahead=True)
    print("MEASURED plain vs hinted: rows identical %s, payload words identical %s, max |d payload| %.3g" % (
        np.array_equal(_words(la), _words(lb)), np.array_equal(_words(pa), _words(pb)), float(np.abs(pa - pb).max())))
    assert np.array_equal(la[:, 7:], lb[:, 7:])                                 # converged flags, pass counts, n_hit
    assert np.abs(la[:, :7] - lb[:, :7]).max() <= 1e-6 and np.abs(pa7 - pb7).max() <= 1e-6
    assert np.array_equal(ka, kb)
    assert np.abs(pa - pb).max() <= 1e-5 * max(1.0, float(np.abs(pa).max()))
    assert (la[:, 7] != 0).any(), "some frame should converge and be fused"
