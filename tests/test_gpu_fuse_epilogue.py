"""What a k_fuse launch does behind a workgroup's last band (csrc/gsdf_kernels.hip, the end of k_fuse): the frame's log row, which
is written at the FRONT of the launch from the head's result; the per-tile counters and their running totals; the
deferred list, added by the launch's last workgroup; that workgroup's bookkeeping, whose loads are requested together.
None of it feeds a voxel: rows, poses and counters must be what they were, at every loop length of the add."""
import ctypes

import numpy as np
import pytest

from conftest import pose7_from

VS = np.float32(0.01)
T = np.float32(10) * VS
N_FRAMES = 13              # frame 0 at its ground-truth pose, 12 tracked
BAD = 7                    # the tracked frame that cannot converge: a plane at 3.4 m, behind every voxel of the map (the scene ends at 2.4 m)
# 3 x 3 and 7 x 5 tiles of 16 x 16: the right and the bottom ones are not whole.  At 1 cm voxels a pixel of these images is 3 - 5 cm
# wide, the tracked points fall between the map's rays and NO frame converges (measured: 25 passes on every frame of all four
# streams): those streams test the rows of launches whose gate stays closed.  The `coarse` streams -- voxels of about a pixel's
# footprint and the thresholds of tests/test_track_pass_chain.py, where optimize() ends within a few passes on some frames and not
# at all on others -- test the launches that fuse.
STREAMS = {
    "48x36": dict(W=48, H=36, vs=0.01, trunc=10, conv=None),
    "100x75": dict(W=100, H=75, vs=0.01, trunc=10, conv=None),
    "48x36-coarse": dict(W=48, H=36, vs=0.06, trunc=5, conv=0.03),
    "100x75-coarse": dict(W=100, H=75, vs=0.04, trunc=5, conv=0.02),
}


def _quat_to_R_f32(q):
    """Eigen's toRotationMatrix in float32, operation by operation as the library's gsdf_quat_to_R (csrc/gsdf_math.h) does it"""
    f = np.float32
    x, y, z, w = (f(v) for v in q)
    tx, ty, tz = f(2) * x, f(2) * y, f(2) * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = f(1)
    return np.array([one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, one - (txx + tyy)], np.float32).reshape(3, 3)


def _words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _frames(pkg, W, H):
    seq = pkg.synth.Sequence("tum", W, H, n_frames=N_FRAMES, seed=1)
    frames = [seq.frame(i) for i in range(N_FRAMES)]
    d = np.full_like(frames[BAD][0], 3.4)            # inside the depth range (0.5 .. 3.5 m); no tracked point finds a voxel
    frames[BAD] = (d, frames[BAD][1], frames[BAD][2])
    return seq, frames


_streams = {}


def _tracked_stream(pkg, O, name, hint):
    """the stream through gsdf_track_and_fuse_dev, production library, synchronised after every frame; checks every frame's row
    against the state read after that frame and returns (log, stats after the last frame).  Run once per (stream, hint)."""
    key = (name, hint)
    if key in _streams:
        return _streams[key]
    c = STREAMS[name]
    W, H = c["W"], c["H"]
    vs = np.float32(c["vs"])
    kw = {} if c["conv"] is None else {"conv": c["conv"]}
    seq, frames = _frames(pkg, W, H)
    g = pkg.GradSdf(vs, np.float32(c["trunc"]) * vs, W, H, seq.K, capacity_log2=21)
    d0, R0, t0 = frames[0]
    p = pose7_from(O, R0, t0)
    g.update(d0, _quat_to_R_f32(p[3:]), t0)
    g.set_pose(p)
    dev = [g.upload(f[0]) for f in frames]
    fused = 1
    for i in range(1, N_FRAMES):
        if hint and i + 1 < N_FRAMES:
            g.track_and_fuse_ahead_dev(dev[i], dev[i + 1], **kw)
        else:
            g.track_and_fuse_dev(dev[i], **kw)
        g.sync()
        log = g.frame_log()
        assert log.shape == (i, 10), (i, log.shape)                      # exactly one row per tracked frame, in order
        row = log[-1]
        st = g.stats()
        assert np.array_equal(_words(row[:7]), _words(g.get_pose())), (i, row[:7], g.get_pose())
        assert int(row[7]) == st["converged"] and int(row[8]) == st["track_passes"], (i, row, st)
        fused += int(row[7])
        assert st["frames"] == fused, (i, st["frames"], fused)           # a frame that did not converge is logged and not fused
        if i == BAD:
            assert int(row[7]) == 0
    log = g.frame_log().copy()
    st = g.stats()
    g.close()
    print("MEASURED %s hint=%s: converged %s, passes %s" % (name, hint, log[:, 7].astype(int).tolist(), log[:, 8].astype(int).tolist()))
    _streams[key] = (log, st)
    return _streams[key]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STREAMS))
@pytest.mark.parametrize("hint", [False, True])
def test_one_log_row_per_tracked_frame_written_from_the_front(pkg, O, name, hint):
    """one row per tracked frame, equal to gsdf_get_pose / stats() read after that frame -- the frame that cannot converge
    included, which is logged and leaves Sdf::counter_ alone"""
    log, st = _tracked_stream(pkg, O, name, hint)
    assert log.shape == (N_FRAMES - 1, 10)
    assert int(log[BAD - 1, 7]) == 0
    if name.endswith("coarse"):
        assert log[:, 7].sum() >= 1                   # (a stream on which nothing converges does not test the launches that fuse)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STREAMS))
def test_hinted_and_unhinted_logs_are_the_same_words(pkg, O, name):
    a, sa = _tracked_stream(pkg, O, name, False)
    b, sb = _tracked_stream(pkg, O, name, True)
    assert np.array_equal(_words(a), _words(b))
    assert sa["n_upd"] == sb["n_upd"] and sa["n_valid"] == sb["n_valid"] and sa["frames"] == sb["frames"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STREAMS))
@pytest.mark.parametrize("hint", [False, True])
def test_counters_of_the_tracked_stream_equal_the_oracles(pkg, O, name, hint):
    """n_upd / n_valid (the sums of the per-tile running totals) against the oracle fusing the same frames at
    the logged poses: every sample and every valid pixel of every fused frame counted exactly once"""
    log, st = _tracked_stream(pkg, O, name, hint)
    c = STREAMS[name]
    W, H = c["W"], c["H"]
    vs = np.float32(c["vs"])
    seq, frames = _frames(pkg, W, H)
    o = O.Oracle(vs, np.float32(c["trunc"]) * vs, W, H, seq.K)
    d0, R0, t0 = frames[0]
    p = pose7_from(O, R0, t0)
    nu, nv = o.update(d0, _quat_to_R_f32(p[3:]), t0)
    for i in range(1, N_FRAMES):
        row = log[i - 1]
        if int(row[7]):
            a, b = o.update(frames[i][0], _quat_to_R_f32(row[3:7]), row[:3].copy())
            nu += a; nv += b
    assert st["n_upd"] == nu and st["n_valid"] == nv, (st["n_upd"], nu, st["n_valid"], nv)


def _tile_counters(L, g, n_tiles):
    buf = (ctypes.c_ulonglong * (4 * n_tiles))()
    assert L.gsdf_debug_tile_counters(g.h, buf, n_tiles) == 0
    return np.array(list(buf), dtype=np.int64).reshape(n_tiles, 4)


@pytest.mark.gpu
def test_cumulative_tile_counters_are_the_sum_of_the_launches(pkg):
    """gsdf_debug_tile_counters (test build): columns 2, 3 (running totals) equal columns 0, 1 (this launch) summed over the
    launches, tile by tile"""
    W, H, n = 100, 75, 5
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=1)
    L = pkg.binding.load_test_lib()
    g = pkg.GradSdf(VS, T, W, H, seq.K, capacity_log2=20, lib=L)
    n_tiles = ((W + 15) // 16) * ((H + 15) // 16)
    tot = np.zeros((n_tiles, 2), np.int64)
    for i in range(n):
        g.update(*seq.frame(i))
        g.sync()
        c = _tile_counters(L, g, n_tiles)
        tot += c[:, :2]
        assert np.array_equal(c[:, 2:], tot), i
    st = g.stats()
    assert st["n_upd"] == tot[:, 0].sum() and st["n_valid"] == tot[:, 1].sum()
    assert tot[:, 0].min() > 0                                         # every tile, the partial ones at the edges included, counted
    g.close()


# one launch's deferred list: shorter than the workgroup that adds it (512 threads: some add nothing), up to four entries per
# thread (the reach of one trip of the unrolled add in tools/experiments/k_fuse_deferred_add_unrolled_r08.patch), longer.  Lengths
# from the CPU oracle (distinct voxels of the frame): 8 x 8 with only its middle 4 x 4 pixels ~ 330, 8 x 8 1 311, 16 x 16 5 037,
# 48 x 36 (nine tiles) 19 883
TRIP = 4 * 512
DEFER_CASES = {
    "8x8-middle": dict(W=8, H=8, keep=(2, 6), lo=1, hi=511),
    "8x8": dict(W=8, H=8, keep=None, lo=512, hi=TRIP),
    "16x16": dict(W=16, H=16, keep=None, lo=TRIP + 1, hi=None),
    "48x36": dict(W=48, H=36, keep=None, lo=TRIP + 1, hi=None, cap=21),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(DEFER_CASES))
def test_deferred_add_at_every_loop_length(pkg, case):
    """every tile defers (test build, debug bit 4): the launch's last workgroup adds the whole frame.  The map must be the plain
    path's (bar of test_fusion_handoff_loses_nothing_at_full_size: same keys, sums within 1e-5 relative), and n_deferred must grow
    by the number of entries the tiles appended -- counted where they are appended (debug bit 64: the tile word of the trace
    carries the length of the list a tile's flush hands over, dbg[6] counts the entries the walk appends one by one when a voxel
    finds no room in the LDS table)."""
    c = DEFER_CASES[case]
    W, H = c["W"], c["H"]
    seq = pkg.synth.Sequence("tum", W, H, n_frames=3, seed=1)
    frames = [seq.frame(i) for i in range(3)]
    if c["keep"]:
        a, b = c["keep"]
        for i, (d, R, t) in enumerate(frames):
            m = np.zeros_like(d)
            m[a:b, a:b] = d[a:b, a:b]
            frames[i] = (m, R, t)
    L = pkg.binding.load_test_lib()
    n_tiles = ((W + 15) // 16) * ((H + 15) // 16)
    plain = pkg.GradSdf(VS, T, W, H, seq.K, capacity_log2=c.get("cap", 18))
    g = pkg.GradSdf(VS, T, W, H, seq.K, capacity_log2=c.get("cap", 18), lib=L)
    g.debug_flags(4 | 64)
    seen = walk_seen = 0
    lens = []
    dbg = (ctypes.c_ulonglong * 24)()
    for d, R, t in frames:
        plain.update(d, R, t)
        g.update(d, R, t)
        g.sync()
        buf = (ctypes.c_ulonglong * (2048 * 16))()
        assert L.gsdf_debug_trace(g.h, buf, 2048) == 0
        rows = np.array(list(buf), dtype=np.int64).reshape(2048, 16)
        assert L.gsdf_debug_read(g.h, dbg) == 0
        appended = int(((rows[:n_tiles, 15] >> 36) & 0xFFFFF).sum()) + int(dbg[6]) - walk_seen
        walk_seen = int(dbg[6])
        st = g.stats()
        added = st["n_deferred"] - seen
        seen = st["n_deferred"]
        lens.append(added)
        assert added == appended, (added, appended)
        assert int(rows[2047, 5]) == appended                          # ... and it is the length the last workgroup read
        assert added >= c["lo"] and (c["hi"] is None or added <= c["hi"]), (case, added)
    print("MEASURED %s: deferred list per launch %s" % (case, lens))
    assert st["fuse_timeouts"] == 0
    ka, pa = plain.export(sorted=True, raw=True)
    kb, pb = g.export(sorted=True, raw=True)
    assert np.array_equal(ka, kb)
    assert ka.shape[0] >= lens[0] // 2
    scale = np.maximum(1.0, np.abs(pb[:, 4:5]))
    assert (np.abs(pa - pb) / scale).max() < 1e-5
    sp = plain.stats()
    assert sp["n_upd"] == st["n_upd"] and sp["n_valid"] == st["n_valid"]
    plain.close()
    g.close()
