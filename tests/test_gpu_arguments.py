"""GPU parity at the arguments the other parity tests leave at the reference's defaults: the depth range (Sdf::set_zmin /
set_zmax, Sdf.h:123-129; defaults 0.5 / 3.5), the tracker's damping and convergence threshold (RigidOptimizer.h:85-97;
defaults 1 and 1e-3) -- and the host state that depends on them: next-frame normals computed ahead under an old range or for
a freed buffer, and the fusion kernel's LDS table chosen per frame.  Every comparison is against the CPU oracle at the bars of
tests/test_gpu_parity.py: keys and occupancy bit-exact, counters exact, SDF / pose <= 1e-4."""
import ctypes

import numpy as np
import pytest

from conftest import pose7_from
from test_gpu_parity import TOL, _cmp_tables, _mk

pytestmark = pytest.mark.gpu

W, H = 640, 480
VS = np.float32(0.01)
CUT = (0.8, 2.2)             # the tum room's back wall lies at 2.28 .. 2.33 m: every wall tile is outside, tiles at its edge straddle zmax


def _room(pkg, scale=1.0, n=4, seed=0, pose_rows=None):
    """the "tum" room scaled by `scale` about the camera's rest position: frame depths scale by the same factor"""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=seed, pose_rows=pose_rows)
    c = np.array([0.0, -0.65, 0.0])
    seq.box = (c + scale * (seq.box[0] - c), c + scale * (seq.box[1] - c))
    sp = seq.spheres.copy()
    sp[:, :3] = c + scale * (sp[:, :3] - c)
    sp[:, 3] *= scale
    seq.spheres = sp
    return seq


def _receding_rows(pkg, n, start=-0.70, step=0.012):
    """TUM-format pose rows: the tum room's camera looking at the back wall and moving straight back, `step` m per frame"""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=1)
    q = pkg.synth.R_to_quat_np(seq.pose(0)[0])
    return np.array([[i, 0.0, start - step * i, 0.0, *q] for i in range(n)])


def _clean(trace, conv):
    """the premise of a deterministic frame: every pass's |xi|^2 at least 10 % off the threshold (test_tracker_sampled_matches_oracle)"""
    return bool((np.abs(trace[:, 35] / np.float32(conv * conv) - 1.0) >= 0.1).all())


# ---- the oracle's and the library's frame loop ---------------------------------------------------------------------------

def oracle_check(O, seq, frames, log, ranges=None, conv=1e-3, damping=1.0, min_frames=8):
    """The library's frame loop (its frame log) against the oracle's main_scan_3d.cpp:255-266, kept in step the way
    tests/lockstep.py keeps the tracker: frame i of the oracle starts from the pose the library ended frame i - 1 with, and the
    oracle's map takes the frames the library fused, at the library's pose -- so every frame starts from the same pose on maps that
    differ in the last bits only, and one frame that cycles for 25 passes (its last iterate amplifies those bits) does not decide
    the rest of the stream.  On every frame the oracle ends within 6 passes with |xi|^2 at least 10 % off the threshold at every
    pass (the premise of test_tracker_sampled_matches_oracle): the same converged flag, the same pass count, and the pose within
    TOL * i (the drift rule of test_track_and_fuse_stream_matches_oracle_loop).  At least min_frames frames must be such frames.
    ranges: {frame index: (zmin, zmax)} applied before that frame.  Returns the oracle."""
    ranges = ranges or {}
    zr = ranges.get(0, (0.5, 3.5))
    o = O.Oracle(VS, np.float32(10) * VS, W, H, seq.K, zmin=zr[0], zmax=zr[1])
    d0, R0, t0 = frames[0]
    p = pose7_from(O, R0, t0)
    o.update(d0, O.quat_to_R(p[3:]), t0)
    n = 0
    for i in range(1, len(frames)):
        if i in ranges:
            o.set_zrange(*ranges[i])
        co, po, used, trace, _ = o.track(frames[i][0], p, conv=conv, damping=damping)
        if used <= 6 and _clean(trace, conv):
            assert bool(log[i - 1, 7]) == co and int(log[i - 1, 8]) == used, (i, log[i - 1, 7:9], co, used)
            assert np.abs(log[i - 1, :7] - po).max() <= TOL * i, (i, float(np.abs(log[i - 1, :7] - po).max()))
            n += 1
        p = log[i - 1, :7].copy()
        if log[i - 1, 7]:
            o.update(frames[i][0], O.quat_to_R(p[3:]), p[:3])
    print("MEASURED %d of %d frames held to the oracle (ended within 6 passes, |xi|^2 >= 10 %% off the threshold)" % (n, len(frames) - 1))
    assert n >= min_frames, (n, len(frames) - 1)
    return o


def gpu_loop(pkg, O, seq, frames, ranges=None, hint=False, conv=1e-3, damping=1.0, lib=None):
    """the same loop through gsdf_track_and_fuse_dev (a next-frame hint before every frame when `hint`)"""
    ranges = ranges or {}
    zr = ranges.get(0, (0.5, 3.5))
    g = pkg.GradSdf(VS, np.float32(10) * VS, W, H, seq.K, capacity_log2=22, zmin=zr[0], zmax=zr[1], lib=lib)
    d0, R0, t0 = frames[0]
    p = pose7_from(O, R0, t0)
    g.update(d0, O.quat_to_R(p[3:]), t0)
    g.set_pose(p)
    dev = [g.upload(f[0]) for f in frames]
    for i in range(1, len(frames)):
        if i in ranges:
            g.set_zrange(*ranges[i])           # after frame i - 1's call, which was told (hint) that frame i comes next
        if hint and i + 1 < len(frames):
            g.hint_next_depth(dev[i + 1])
        g.track_and_fuse_dev(dev[i], conv=conv, damping=damping)
    g.sync()
    log = g.frame_log().copy()
    st = g.stats()
    return g, log, st


def _same_stream(a, b):
    """two library runs of one stream that must agree (hint or not): flags, passes, poses to the last bits, the same key set"""
    (la, ka, pa), (lb, kb, pb) = a, b
    assert np.array_equal(la[:, 7:9], lb[:, 7:9])
    assert np.abs(la[:, :7] - lb[:, :7]).max() <= 1e-6
    assert ka.shape == kb.shape, (ka.shape, kb.shape)
    assert np.array_equal(ka, kb)
    assert np.abs(pa - pb).max() <= 1e-5 * max(1.0, float(np.abs(pa).max()))


def _keys_near(g, o):
    kg, _ = g.export()
    ko, _ = o.export()
    inter = len(set(map(tuple, kg)) & set(map(tuple, ko)))
    assert inter / max(len(kg), len(ko)) > 0.97      # poses differ in the last bits -> keys near-identical


# ---- 2. fusion at non-default depth ranges ---------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,zr,what", [
    (1.0, CUT, "back wall cut: tiles straddle zmax, fewer bands"),
    (1.0, (1.0, 3.0), "range inside the default, nothing cut"),
    (0.3, (0.3, 3.5), "room at 0.37 .. 0.70 m: near tiles fail the ordered test and defer"),
    (2.0, (0.5, 6.0), "room at 2.5 .. 4.6 m: beyond the default zmax, far tiles"),
])
def test_fusion_at_a_depth_range_matches_oracle(pkg, O, scale, zr, what):
    seq = _room(pkg, scale, n=3)
    g = pkg.GradSdf(VS, np.float32(10) * VS, W, H, seq.K, capacity_log2=23, zmin=zr[0], zmax=zr[1])
    o = O.Oracle(VS, np.float32(10) * VS, W, H, seq.K, zmin=zr[0], zmax=zr[1])
    nu = nv = 0
    depths = []
    for i in range(seq.n):
        d, R, t = seq.frame(i)
        depths.append(d)
        g.update(d, R, t)
        a, b = o.update(d, R, t)
        nu += a; nv += b
    g.sync()
    d = np.stack(depths)
    inside = (d > zr[0]) & (d < zr[1])
    default = (d > 0.5) & (d < 3.5)
    print("MEASURED %s: %.3f of the pixels inside the range, %.3f inside the default one" % (what, inside.mean(), default.mean()))
    assert _cmp_tables(g, o) > 10000
    st = g.stats()
    assert st["n_upd"] == nu and st["n_valid"] == nv
    if zr == CUT:
        assert 0.2 < inside.mean() < 0.8                      # the premise: the range cuts
    if scale == 0.3:
        assert ((d > 0.3) & (d <= 0.5)).mean() > 0.2 and st["n_deferred"] > 10000   # pixels the default range drops; deferred tiles
    if scale == 2.0:
        assert (d > 3.5).mean() > 0.3 and st["far_tiles"] * 16 > st["fuse_blocks"]
    g.close()


@pytest.mark.parametrize("flags", [0, 4, 512, 256, 512 + 4, 8192, 1024, 1024 + 512, 1024 + 4])
def test_fusion_forced_paths_at_a_cutting_range(pkg, O, flags):
    """the nine path-forcing flag sets of test_fusion_forced_paths_match_oracle (test library) at zmax 2.2, which cuts the back wall"""
    seq, g, o = _mk(pkg, O, kind="tum", W=320, H=240, vs=0.01, trunc=10, cap=21, n=3, lib=pkg.binding.load_test_lib())
    g.set_zrange(*CUT)
    o.set_zrange(*CUT)
    g.debug_flags(flags)
    nu = nv = 0
    for i in range(seq.n):
        d, R, t = seq.frame(i)
        g.update(d, R, t)
        a, b = o.update(d, R, t)
        nu += a; nv += b
    g.sync()
    assert _cmp_tables(g, o) > 5000
    st = g.stats()
    assert st["n_upd"] == nu and st["n_valid"] == nv
    if flags == 8192:
        assert st["fuse_timeouts"] > 50
    else:
        assert st["fuse_timeouts"] == 0
    g.close()


# ---- 3. tracking at a non-default range -------------------------------------------------------------------------------------

def _two_frame_map(pkg, O, zr=(0.5, 3.5)):
    seq = pkg.synth.Sequence("tum", W, H, n_frames=3, seed=0)
    g = pkg.GradSdf(VS, np.float32(10) * VS, W, H, seq.K, capacity_log2=21, zmin=zr[0], zmax=zr[1])
    o = O.Oracle(VS, np.float32(10) * VS, W, H, seq.K, zmin=zr[0], zmax=zr[1])
    for i in range(2):
        d, R, t = seq.frame(i)
        g.update(d, R, t)
        o.update(d, R, t)
    d2, _, _ = seq.frame(2)
    _, R1, t1 = seq.frame(1)
    return seq, g, o, d2, pose7_from(O, R1, t1)


@pytest.mark.parametrize("sampling", [None, 2])
def test_tracker_at_a_cutting_range_matches_oracle(pkg, O, sampling):
    seq, g, o, d2, p0 = _two_frame_map(pkg, O, CUT)
    n0 = g.stats()["n_hit"]
    cg, pg, passes = g.track(d2, p0, iters=1, sampling=sampling)
    co, po, used, trace, hits = o.track(d2, p0, iters=1, sampling=sampling or 1)
    assert g.stats()["n_hit"] - n0 == int(hits[0]) > 1000         # the same pixels pass the range gate
    assert np.abs(pg - po).max() <= TOL
    co, po, used, trace, hits = o.track(d2, p0, sampling=sampling or 1)
    assert _clean(trace, 1e-3), trace[:, 35]
    print("MEASURED sampling %s: the oracle ends after %d passes" % (sampling, used))
    # a run of more than 6 passes cycles at |xi|^2 ~ 5e-6 and amplifies the last bits pass after pass (tests/lockstep.py): its
    # first 4 passes are compared, the whole run where it is short
    k = used if used <= 6 else 4
    cg, pg, passes = g.track(d2, p0, sampling=sampling, iters=k)
    co, po, used_k, _, _ = o.track(d2, p0, sampling=sampling or 1, iters=k)
    assert cg == co and passes == used_k, (cg, co, passes, used_k)
    assert np.abs(pg - po).max() <= TOL
    g.close()


def test_raycast_at_a_non_default_range_matches_oracle(pkg, O):
    """the bar of test_raycast_matches_definition_and_input_depth, with the ray range (1.5, 2.25): the spheres in front are skipped
    by rays that start behind them, the back wall at 2.28 m is beyond the far end"""
    seq, g, o = _mk(pkg, O, kind="tum", W=320, H=240, vs=0.01, trunc=10, cap=21, n=4)
    for i in range(seq.n):
        d, R, t = seq.frame(i)
        g.update(d, R, t)
        o.update(d, R, t)
    d, R, t = seq.frame(1)
    zg, ng = g.raycast(R, t, zmin=1.5, zmax=2.25)
    zo, no = o.raycast(R, t, zmin=1.5, zmax=2.25)
    zd, _ = o.raycast(R, t)
    hit_g, hit_o = zg > 0, zo > 0
    assert (hit_g == hit_o).mean() > 0.999
    both = hit_g & hit_o
    assert 0.05 < both.mean() < (zd > 0).mean() - 0.05            # the range removes hits the default range has
    assert zg[hit_g].min() >= 1.5 - 0.02 and zg.max() <= 2.25 + 0.02
    dz = np.abs(zg - zo)[both]
    assert np.percentile(dz, 99.9) <= TOL and np.median(dz) <= 1e-6
    assert np.percentile(np.abs(ng - no)[:, both], 99.9) <= 1e-3
    g.close()


@pytest.mark.parametrize("hint", [False, True])
def test_track_and_fuse_stream_at_a_cutting_range(pkg, O, hint):
    seq = pkg.synth.Sequence("tum", W, H, n_frames=17, seed=0)
    frames = [seq.frame(i) for i in range(seq.n)]
    g, log, st = gpu_loop(pkg, O, seq, frames, {0: CUT}, hint=hint)
    o = oracle_check(O, seq, frames, log, {0: CUT}, min_frames=6)     # measured on MI355X: 7 of 16
    _keys_near(g, o)
    g.close()


# ---- 4. the range changed mid-stream; 5. a hinted buffer freed ------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["widen", "narrow"])
def test_range_changed_mid_stream_with_hints(pkg, O, schedule):
    """set_zrange between two frames of a hinted stream.  The hint of frame 6 was given before frame 5's call, whose fusion computed
    frame 6's normals AND tile statistics under the old range.  Widening: a back-wall tile that had no pixel inside (0.8, 2.2) would
    count no valid pixel and never be walked under (0.5, 3.5) unless the change withdraws the hint."""
    # (frames 4 and 5 converge within the first batch at either range: frame 5's fusion runs on the new route and computes frame 6's
    # normals in its tail)
    ranges = {0: CUT, 6: (0.5, 3.5)} if schedule == "widen" else {0: (0.5, 3.5), 6: CUT}
    seq = pkg.synth.Sequence("tum", W, H, n_frames=17, seed=0)
    frames = [seq.frame(i) for i in range(seq.n)]
    runs = []
    for hint in (False, True):
        g, log, st = gpu_loop(pkg, O, seq, frames, ranges, hint=hint)
        keys, pay = g.export(sorted=True)
        runs.append((log, keys, pay))
        print("MEASURED %s, hint %d: %d voxels, n_valid %d" % (schedule, hint, keys.shape[0], st["n_valid"]))
        if not hint:
            g_plain = g
        else:
            g.close()
    _same_stream(runs[0], runs[1])
    o = oracle_check(O, seq, frames, runs[0][0], ranges)             # measured on MI355X: 9 of 16 either way
    _keys_near(g_plain, o)
    g_plain.close()


def test_hinted_buffer_freed_and_reallocated(pkg, O):
    """hint(B) + track_and_fuse(A) computes B's normals ahead; then B is freed, a buffer of the same size allocated (often at B's
    address) and filled by a device-to-device copy of ANOTHER frame -- not through gsdf_dev_upload*, which withdraws hints by
    itself -- and that buffer is the next frame.  The result must be the unhinted run's.  (Never calls a frame entry on a freed
    buffer.)"""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=6, seed=0)
    frames = [seq.frame(i) for i in range(seq.n)]
    nbytes = W * H * 4
    out = []
    for hint in (False, True):
        g = pkg.GradSdf(VS, np.float32(10) * VS, W, H, seq.K, capacity_log2=22)
        d0, R0, t0 = frames[0]
        p = pose7_from(O, R0, t0)
        g.update(d0, O.quat_to_R(p[3:]), t0)
        g.set_pose(p)
        dev = [g.upload(f[0]) for f in frames]
        g.track_and_fuse_dev(dev[1])
        B = ctypes.c_void_p()
        g._chk(g.L.gsdf_dev_alloc(g.h, ctypes.byref(B), nbytes))
        g._chk(g.L.gsdf_dev_upload(g.h, B, np.ascontiguousarray(frames[5][0]).ctypes.data_as(ctypes.c_void_p), nbytes))
        if hint:
            g.hint_next_depth(B)                                    # B (frame 5's depth) announced as the next frame ...
        g.track_and_fuse_dev(dev[2])                               # ... its normals computed in the tail of frame 2's fusion
        b_addr = B.value
        g._chk(g.L.gsdf_dev_free(g.h, B))
        C = ctypes.c_void_p()
        g._chk(g.L.gsdf_dev_alloc(g.h, ctypes.byref(C), nbytes))
        g._dev.append(C)
        print("MEASURED hint %d: the reallocated buffer %s the freed one's address" % (hint, "has" if C.value == b_addr else "does NOT have"))
        # frame 3's depth, copied on the device: what the library sees at that address now is another image than the hinted one
        hip = pkg.binding._hip
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        g.sync()
        assert hip.hipMemcpy(C, dev[3], nbytes, 3) == 0            # hipMemcpyDeviceToDevice
        assert hip.hipDeviceSynchronize() == 0                     # (the library's stream is not ordered behind the null stream)
        g.track_and_fuse_dev(C)
        g.track_and_fuse_dev(dev[4])
        g.sync()
        log = g.frame_log().copy()
        keys, pay = g.export(sorted=True)
        out.append((log, keys, pay))
        g.close()
    _same_stream(out[0], out[1])


# ---- 6. the fusion's LDS table chosen across its threshold --------------------------------------------------------------------

def test_far_table_flips_mid_stream(pkg, O):
    """A camera backing away from the room's back wall (2.35 -> 2.64 m, zmax 6): the count of tiles too big for the small LDS table
    crosses fuse_blocks / 16 and the frame entries switch to the kernel with the larger table mid-stream -- production library,
    nothing forced.  Hinted and unhinted streams must agree with each other and with the oracle."""
    n = 25
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=0, pose_rows=_receding_rows(pkg, n))
    frames = [seq.frame(i) for i in range(seq.n)]
    ranges = {0: (0.5, 6.0)}
    runs, stats = [], []
    for hint in (False, True):
        g, log, st = gpu_loop(pkg, O, seq, frames, ranges, hint=hint)
        print("MEASURED hint %d: far_tiles %d of %d tiles at the end, %d of %d fusion launches with the larger table"
              % (hint, st["far_tiles"], st["fuse_blocks"], st["far_table_launches"], st["fuse_launches"]))
        o = oracle_check(O, seq, frames, log, ranges, min_frames=7)    # measured on MI355X: 8 of 24
        keys, pay = g.export(sorted=True)
        runs.append((log, keys, pay))
        stats.append(st)
        if hint:
            _keys_near(g, o)
        g.close()
    _same_stream(runs[0], runs[1])
    for st in stats:
        assert st["far_tiles"] * 16 > st["fuse_blocks"]                               # far at the end ...
        assert 0 < st["far_table_launches"] < st["fuse_launches"]                     # ... and not from the start: it flipped


# ---- 7. damping and convergence threshold -------------------------------------------------------------------------------------

SOLVER = [(0.5, 1e-3), (1.0, 1e-2), (1.0, 1e-4)]


@pytest.mark.parametrize("damping,conv", SOLVER)
def test_tracker_damping_and_threshold_match_oracle(pkg, O, damping, conv):
    seq, g, o, d2, p0 = _two_frame_map(pkg, O)
    cg, pg, passes = g.track(d2, p0, conv=conv, damping=damping)
    co, po, used, trace, _ = o.track(d2, p0, conv=conv, damping=damping)
    print("MEASURED damping %g conv %g: oracle converged %d after %d passes" % (damping, conv, co, used))
    assert _clean(trace, conv), trace[:, 35]
    assert cg == co and passes == used, (cg, co, passes, used)
    assert np.abs(pg - po).max() <= TOL
    g.close()


@pytest.mark.parametrize("head", ["1", "0"])
@pytest.mark.parametrize("damping,conv", SOLVER[:2])
def test_track_and_fuse_stream_damping_and_threshold(pkg, O, monkeypatch, damping, conv, head):
    """the solve inside k_fuse<.., HEAD> (GSDF_FUSE_HEAD=1, the default) and the tracker launch's own (0) at non-default arguments"""
    monkeypatch.setenv("GSDF_FUSE_HEAD", head)
    seq = pkg.synth.Sequence("tum", W, H, n_frames=17, seed=0)
    frames = [seq.frame(i) for i in range(seq.n)]
    g, log, st = gpu_loop(pkg, O, seq, frames, hint=True, conv=conv, damping=damping)
    o = oracle_check(O, seq, frames, log, conv=conv, damping=damping)   # measured on MI355X: 12 (damping 0.5), 16 (conv 1e-2) of 16
    _keys_near(g, o)
    g.close()


# ---- 9. what the direction rule of _cmp_tables leaves out ---------------------------------------------------------------------

def test_direction_rule_exclusion_is_bounded(pkg, O):
    seq, g, o = _mk(pkg, O, kind="tum", W=W, H=H, vs=0.01, trunc=10, cap=22, n=4, seed=0)
    for i in range(seq.n):
        d, R, t = seq.frame(i)
        g.update(d, R, t)
        o.update(d, R, t)
    ex = {}
    assert _cmp_tables(g, o, exclusion=ex) > 100000
    print("MEASURED excluded fraction %.4f, largest excluded direction error %.3e" % (ex["fraction"], ex["max_dir_err"]))
    # measured on MI355X: 0.0155 of the voxels excluded, largest direction error among them 7.2e-2 (the 640x480 tum case, 4 frames)
    assert ex["fraction"] <= 0.02 and ex["max_dir_err"] <= 0.1
    g.close()
