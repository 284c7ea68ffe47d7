"""Inputs the C-ABI accepts and no other test visits, HIP path against the CPU oracle:

  A. the normals window: every odd win from 1 to 15 but the reference's 11 (k_ncache_rows / k_ncache_cols, normals_tile in its three
     carriers -- k_normals, the tail of the previous k_fuse, the riders of the first tracker launches -- and the tile statistics
     they hand to k_fuse), frames narrower than the window (reflect101 reflects more than once) and smaller than a tile;
  B. the edge of the packable key range (21 biased bits per axis, +-2^20 voxels): a frame next to it (k_fuse's tile-wide range_ok
     sends every sample through the deferred route), frames that straddle it (GSDF_ERR_KEY_RANGE and what it leaves behind,
     include/gsdf.h), and a designed map with voxels on the edge through every reader;
  C. depth pixels that are neither a finite positive number nor 0: negative, +-inf, huge, denormal, -0 (and NaN for the normals).

What the oracle defines and the comparison has to respect.  A pixel whose NORMAL is not finite still passes the gates of
MapGradPixelSdf::update (:95, :98 are `<` comparisons, false for NaN): the reference fuses it, distance and weight as usual, and
its voxels' gradient sums become NaN.  That is every window around a denormal depth pixel (1 / z = inf), and three quarters of the
frame at win = 1 (a one-pixel moment matrix is singular: Q is inf * 0).  _cmp_maps below therefore asks for the same non-finite
gradients voxel by voxel, holds distance and weight of those voxels to the bars of _cmp_tables, and hands the voxels with a finite
gradient to _cmp_tables itself, whole: its cap on the voxels without a stable direction (5 %) is met by the oracle's map alone
on every input here, win = 1 included (at least 0.976 of the finite-gradient voxels have one).

A NaN DEPTH pixel is left out of every fusion and tracker test: it passes the reference's range gate (:87, comparisons again), and
float2vox then converts NaN to int -- undefined behaviour in the reference, so there is nothing to compare with (include/gsdf.h)."""
import numpy as np
import pytest

import base_sdf_ref as B
from conftest import pose7_from
from test_gpu_parity import TOL, _cmp_tables, _quat_to_R_f32

pytestmark = pytest.mark.gpu

f32 = np.float32
VS = f32(0.02)
T5 = f32(5) * VS
OFF = 1 << 20
EDGE = 20971.52                       # 2^20 voxels of 2 cm, in metres


class _Rows:
    """exported rows with the export() of a context (what _cmp_tables reads)"""

    def __init__(self, keys, pay):
        self.keys, self.pay = keys, pay

    def export(self, sorted=True):
        return self.keys, self.pay


def _cmp_maps(kg, pg, ko, po):
    """the parity bar on two exported maps (z, y, x order) whose oracle side may hold non-finite gradients; returns the voxel count"""
    assert kg.shape == ko.shape, (kg.shape, ko.shape)
    assert np.array_equal(kg, ko), "voxel key sets differ"
    assert np.isfinite(po[:, 0]).all() and np.isfinite(po[:, 4]).all()
    assert np.array_equal(np.isfinite(pg[:, 1:4]), np.isfinite(po[:, 1:4])), "non-finite gradients differ"
    fin = np.isfinite(po[:, 1:4]).all(axis=1)
    if (~fin).any():
        assert np.abs(pg[~fin, 0] - po[~fin, 0]).max() <= TOL
        assert (np.abs(pg[~fin, 4] - po[~fin, 4]) / np.maximum(1.0, po[~fin, 4])).max() <= TOL
    if fin.any():
        _cmp_tables(_Rows(kg[fin], pg[fin]), _Rows(ko[fin], po[fin]))
    return kg.shape[0]


def _in_range(keys):
    return ((keys >= -OFF) & (keys < OFF)).all(axis=1)


def _bits_equal_where_finite(a, b):
    """a (engine) against b (oracle): the same non-finite mask, the same bits elsewhere"""
    m = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), m)
    assert np.array_equal(a[m].view(np.uint32), b[m].view(np.uint32))


def _fuse_carriers_against_oracle(pkg, O, W, H, K, win, frames, lib=None, flags=0, cap=18):
    """the frames through gsdf_update (k_normals computes the normals) and through a run of gsdf_update_dev (the tail of the previous
    k_fuse does, from the second frame on), each against the oracle: keys, counters, sums"""
    o = O.Oracle(VS, T5, W, H, K, win=win)
    nu = nv = 0
    for d, R, t in frames:
        a, b = o.update(d, R, t)
        nu += a; nv += b
    ko, po = o.export()
    g = pkg.GradSdf(VS, T5, W, H, K, win=win, capacity_log2=cap, lib=lib)
    if flags:
        g.debug_flags(flags)
    for carrier in ("update", "update_dev"):
        g.reset()
        if carrier == "update":
            for d, R, t in frames:
                g.update(d, R, t)
        else:
            dev = [g.upload(f[0]) for f in frames]
            for p, (d, R, t) in zip(dev, frames):
                g.update_dev(p, R, t)
            g.sync()
        st = g.stats()
        assert st["n_upd"] == nu and st["n_valid"] == nv and st["frames"] == len(frames), (carrier, st, nu, nv)
        kg, pg = g.export(sorted=True)
        assert _cmp_maps(kg, pg, ko, po) == o.count()
    g.close()
    return nu, nv


def _frame_loop_equals_two_calls(pkg, O, W, H, K, win, frames, cap=18, conv=1e3):
    """gsdf_track_and_fuse_dev after one set-up frame (the normals ride in the first tracker launches) against gsdf_track +
    gsdf_update from identical state (k_normals): flags, pass counts, pose and map bit for bit, as
    test_gpu_parity.test_frame_loop_call_equals_optimize_then_update; returns the convergence flags.  Frames of a few hundred
    pixels do not track (Gauss-Newton wanders for all 25 passes and the frame is not fused), so the stop threshold is set to where
    the first pass ends optimize() wherever its system can be solved: the frame is then fused, at the start pose, with the normals
    that rode in that pass' launches"""
    res = []
    for one_call in (True, False):
        g = pkg.GradSdf(VS, T5, W, H, K, win=win, capacity_log2=cap)
        g.update(*frames[0])
        pose = pose7_from(O, frames[0][1], frames[0][2])
        g.set_pose(pose)
        flags = []
        for d, _, _ in frames[1:]:
            if one_call:
                g.track_and_fuse_dev(g.upload(d), conv=conv)
                g.sync()
                row = g.frame_log()[-1]
                flags.append((int(row[7]), int(row[8])))
                pose = g.get_pose()
            else:
                done, pose, passes = g.track(d, pose, conv=conv)
                flags.append((int(done), int(passes)))
                if done:
                    g.update(d, _quat_to_R_f32(pose[3:]), pose[:3])
        k, p = g.export(sorted=True)
        res.append((flags, np.array(pose, f32), k, p, g.stats()))
        g.close()
    (f1, p1, k1, v1, s1), (f2, p2, k2, v2, s2) = res
    assert f1 == f2, (f1, f2)
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32))
    assert np.array_equal(k1, k2) and np.array_equal(v1.view(np.uint32), v2.view(np.uint32))
    assert s1["n_upd"] == s2["n_upd"] and s1["n_valid"] == s2["n_valid"] and s1["frames"] == s2["frames"]
    return [c for c, _ in f1]


# ---- A. the normals window ------------------------------------------------------------------------------------------------------

WINDOWS = [1, 3, 5, 9, 13, 15]
SIZES = [(45, 29), (33, 17)]          # two normals tiles and a ragged one / two ragged tiles in x, one and a pixel in y


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("win", WINDOWS)
def test_window_cache_and_normals_bit_exact(pkg, O, win, W, H):
    """gsdf_normals_init(.., win): the eleven cached planes are the oracle's bit for bit (k_ncache_rows / k_ncache_cols keep
    OpenCV's running sums at every window), and so are the normals of a frame where they are finite, with the same non-finite
    mask.  At win = 1 a quarter of the oracle's normals at most are finite: that is the reference."""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=1, seed=1)
    g = pkg.GradSdf(VS, T5, W, H, seq.K, win=win, capacity_log2=14)
    o = O.Oracle(VS, T5, W, H, seq.K, win=win)
    _bits_equal_where_finite(g.normals_cache(), o.normals_cache())
    d, _, _ = seq.frame(0)
    n_o = o.normals(d)
    assert np.isfinite(n_o).all() if win >= 3 else np.isfinite(n_o).all(axis=0).mean() < 0.3
    _bits_equal_where_finite(g.normals(d), n_o)
    g.close()


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("win", WINDOWS)
def test_window_fusion_through_every_normals_carrier(pkg, O, win, W, H):
    """The same frames fused with their normals computed by k_normals (gsdf_update), by the tail of the previous k_fuse (a run of
    gsdf_update_dev) and by the riders of the first tracker launches (gsdf_track_and_fuse_dev).
    A limit at win = 1: the set-up frame leaves NaN gradients in the map, the tracker's system is NaN and no tracked frame is fused,
    so there the third carrier is held to equal flags, pose and (untouched) map only -- the normals that rode are not read by a
    fusion.  A context has one window, so the map cannot be set up at another one."""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=3, seed=1)
    frames = [seq.frame(i) for i in range(3)]
    nu, nv = _fuse_carriers_against_oracle(pkg, O, W, H, seq.K, win, frames[:2])
    assert nv > 200 and nu > 2000
    conv = _frame_loop_equals_two_calls(pkg, O, W, H, seq.K, win, frames)
    print("MEASURED converged flags of the tracked frames:", conv)
    assert win == 1 or any(conv)                          # (win 1: the map's gradients are NaN, nothing can be solved)


@pytest.mark.parametrize("win", [11, 15])
@pytest.mark.parametrize("W,H,n_valid,n_vox", [(7, 5, 35, 369), (3, 40, 27, 289), (1, 1, 1, 11)])
def test_frames_smaller_than_the_window_and_a_tile(pkg, O, W, H, n_valid, n_vox, win):
    """7 x 5, 3 x 40 and 1 x 1 at windows of 11 and 15: the window is wider than the frame, BORDER_REFLECT_101 folds it over more
    than once (and onto the single pixel of a 1 x 1 frame, whose normal is 0 / 0 in the reference).  Cache, normals, fusion."""
    seq = pkg.synth.Sequence("tum", W, H, n_frames=2, seed=1)
    g = pkg.GradSdf(VS, T5, W, H, seq.K, win=win, capacity_log2=14)
    o = O.Oracle(VS, T5, W, H, seq.K, win=win)
    _bits_equal_where_finite(g.normals_cache(), o.normals_cache())
    d, R, t = seq.frame(0)
    _bits_equal_where_finite(g.normals(d), o.normals(d))
    g.close()
    # the premise, on the CPU oracle alone after the first frame: the valid pixels (all 35 of 7 x 5; 27 of the 120 of 3 x 40, whose
    # upper rows are nearer than zmin) and the voxels they leave, the same at both windows (the issue's 360 and 277 voxels were not
    # reproduced: its valid-pixel counts are these)
    o1 = O.Oracle(VS, T5, W, H, seq.K, win=win)
    a, b = o1.update(d, R, t)
    assert b == n_valid and o1.count() == n_vox and a >= n_vox
    _fuse_carriers_against_oracle(pkg, O, W, H, seq.K, win, [seq.frame(0), seq.frame(1)], cap=14)


def test_window_argument_check(pkg, O):
    """win of 0, 2, 17 and -1 is GSDF_ERR_INVALID -- and, as gsdf_normals_init checks its arguments before it lets go of anything,
    the context keeps the frame set-up it had (include/gsdf.h): same planes, and a frame still fuses."""
    W, H = 33, 17
    seq = pkg.synth.Sequence("tum", W, H, n_frames=1, seed=1)
    g = pkg.GradSdf(VS, T5, W, H, seq.K, win=5, capacity_log2=18)
    o = O.Oracle(VS, T5, W, H, seq.K, win=5)
    planes = g.normals_cache()
    for win in (0, 2, 17, -1):
        rc = g.L.gsdf_normals_init(g.h, W, H, g.K.ctypes.data_as(g.L.gsdf_normals_init.argtypes[3]), win)
        assert rc == pkg.binding.ERR_INVALID, win
        assert np.array_equal(g.normals_cache().view(np.uint32), planes.view(np.uint32))
        if win != 17:                                                   # (the oracle has no upper limit)
            with pytest.raises(ValueError):
                O.Oracle(VS, T5, W, H, seq.K, win=win)
    d, R, t = seq.frame(0)
    g.update(d, R, t)
    nu, nv = o.update(d, R, t)
    st = g.stats()
    assert st["n_upd"] == nu and st["n_valid"] == nv
    _cmp_maps(*g.export(sorted=True), *o.export())
    g.close()


# ---- B. the edge of the packable key range --------------------------------------------------------------------------------------

def _edge_ctx(pkg, W, H, K, flags, cap=18):
    """the production library (flags None) or the test build with its path-forcing flags"""
    if flags is None:
        return pkg.GradSdf(VS, T5, W, H, K, capacity_log2=cap)
    g = pkg.GradSdf(VS, T5, W, H, K, capacity_log2=cap, lib=pkg.binding.load_test_lib())
    g.debug_flags(flags)
    return g


LIBS = [None, 4, 512]
LIB_IDS = ["production", "flags4", "flags512"]


@pytest.mark.parametrize("flags", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("axis", [0, 1])
def test_edge_nearby_nothing_beyond(pkg, O, axis, flags):
    """t = edge - 5 m on x (y): every voxel of the frame is packable, but origin + 1023 of every tile's local key box is not, so
    k_fuse's tile-wide range_ok is false and EVERY sample takes the deferred route, with its per-sample range test."""
    W, H = 64, 48
    seq = pkg.synth.Sequence("tum", W, H, n_frames=1, seed=1)
    d, _, _ = seq.frame(0)
    R = np.eye(3, dtype=f32)
    t = np.zeros(3, f32)
    t[axis] = f32(EDGE - 5)
    o = O.Oracle(VS, T5, W, H, seq.K)
    nu, nv = o.update(d, R, t)
    ko, po = o.export()
    assert _in_range(ko).all() and ko[:, axis].max() > OFF - 1023 and len(ko) > 10000        # the premise
    g = _edge_ctx(pkg, W, H, seq.K, flags)
    g.update(d, R, t)                                                   # no error
    st = g.stats()
    assert st["n_upd"] == nu and st["n_valid"] == nv and st["frames"] == 1
    assert st["n_deferred"] == nu                                       # every sample went through the deferred list
    _cmp_maps(*g.export(sorted=True), ko, po)
    g.close()


# translation, and the voxels the CPU oracle leaves inside / outside the packable range (tum 64 x 48, seed 1, R = I).  On z the
# scene's depth (1.2 .. 2.3 m) decides: at -(edge - 2) everything is inside, at -(edge + 2) both sets hold more than 1000 voxels.
# At +-edge itself the float grid of the positions (2 mm at 20971 m) leaves no voxel on index 2^20 (-2^20 - 1) of x and y: an
# off-by-one of the range test would go unseen there.  The cases marked "on" are 3 cm off the edge, where the oracle has voxels on
# the last packable index AND on the first one beyond it (asserted below).
STRADDLE = [((EDGE, 0, 0), 10296, 8292, False), ((-EDGE, 0, 0), 8292, 10296, False), ((0, EDGE, 0), 11637, 6952, False),
            ((0, -EDGE, 0), 6952, 11637, False), ((0, 0, EDGE - 2), 3340, 15175, True), ((0, 0, -EDGE - 2), 15224, 3320, False),
            ((EDGE - 0.03, 0, 0), 10328, 8261, True), ((-EDGE - 0.03, 0, 0), 7967, 10621, True), ((0, EDGE - 0.03, 0), 11719, 6869, True),
            ((0, -EDGE + 0.03, 0), 7287, 11299, True)]
STRADDLE_IDS = ["+x", "-x", "+y", "-y", "+z", "-z", "+x-on", "-x-on", "+y-on", "-y-on"]


@pytest.mark.parametrize("flags", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("t,n_in,n_out,on_index", STRADDLE, ids=STRADDLE_IDS)
def test_frame_straddling_the_edge(pkg, O, t, n_in, n_out, on_index, flags):
    """A frame with voxels on both sides of the edge: gsdf_update returns GSDF_ERR_KEY_RANGE and leaves what include/gsdf.h states:
    every packable voxel fused as if the others did not exist, the others dropped, the frame counted, n_valid and n_upd counting
    every pixel and every sample (the dropped ones too); the status stays until gsdf_reset, after which the context is as new."""
    W, H = 64, 48
    seq = pkg.synth.Sequence("tum", W, H, n_frames=1, seed=1)
    d, R_seq, t_seq = seq.frame(0)
    R = np.eye(3, dtype=f32)
    axis, up = int(np.argmax(np.abs(t))), max(t, key=abs) > 0
    t = np.array(t, f32)
    o = O.Oracle(VS, T5, W, H, seq.K)
    nu, nv = o.update(d, R, t)
    ko, po = o.export()
    inr = _in_range(ko)
    assert int(inr.sum()) == n_in >= 1000 and int((~inr).sum()) == n_out >= 1000          # the premise (oracle alone)
    if on_index:
        last, first_out = (OFF - 1, OFF) if up else (-OFF, -OFF - 1)
        assert (ko[:, axis] == last).sum() >= 20 and (ko[:, axis] == first_out).sum() >= 20
    g = _edge_ctx(pkg, W, H, seq.K, flags)
    with pytest.raises(pkg.GsdfError) as e:
        g.update(d, R, t)
    assert e.value.code == pkg.binding.ERR_KEY_RANGE
    st = g.stats()
    assert st["n_upd"] == nu and st["n_valid"] == nv and st["frames"] == 1
    kg, pg = g.export(sorted=True)
    assert _cmp_maps(kg, pg, ko[inr], po[inr]) == n_in
    with pytest.raises(pkg.GsdfError) as e:                             # sticky
        g.sync()
    assert e.value.code == pkg.binding.ERR_KEY_RANGE
    with pytest.raises(pkg.GsdfError) as e:                             # ... and returned by the blocking tracker entry as well
        g.track(d, np.array([t[0], t[1], t[2], 0, 0, 0, 1], f32), iters=1)
    assert e.value.code == pkg.binding.ERR_KEY_RANGE
    g.reset()
    g.sync()
    assert g.count() == 0 and g.stats()["frames"] == 0
    g.update(d, R_seq, t_seq)                                           # an ordinary frame
    o2 = O.Oracle(VS, T5, W, H, seq.K)
    nu2, nv2 = o2.update(d, R_seq, t_seq)
    st = g.stats()
    assert st["n_upd"] == nu2 and st["n_valid"] == nv2 and st["frames"] == 1
    _cmp_maps(*g.export(sorted=True), *o2.export())
    g.close()


def _designed_map():
    """voxels on the edge and next to it: a wall across y = 50, 11 voxels thick, from x = 2^20 - 60 up to the last packable x,
    and a 6 x 6 x 6 cube in the lowest and in the highest corner of the range (voxels at -2^20 and 2^20 - 1 on every axis, with
    their neighbours), each with a plane through it.  dist, gradient sum, weight; weights are powers of two, so that the raw sum
    dist * w and the exported dist = sum / w are exact"""
    rng = np.random.default_rng(11)
    x, y, z = np.meshgrid(np.arange(OFF - 60, OFF), np.arange(45, 56), np.arange(-30, 30), indexing="ij")
    keys = [np.stack([x, y, z], -1).reshape(-1, 3)]
    dist = [((keys[0][:, 1] - 50).astype(f32) * VS + f32(0.003)).astype(f32)]
    grad = [np.tile(np.array([0, 1, 0], f32), (len(keys[0]), 1))]
    for lo in (-OFF, OFF - 6):
        c = np.stack(np.meshgrid(*[np.arange(lo, lo + 6)] * 3, indexing="ij"), -1).reshape(-1, 3)
        n = np.array([0.6, 0.48, 0.64], f32)
        keys.append(c)
        dist.append((((c - lo).astype(f32) - f32(2.4)) @ n * VS).astype(f32))
        grad.append(np.tile(n, (len(c), 1)))
    keys = np.concatenate(keys).astype(np.int32)
    dist = np.clip(np.concatenate(dist), -T5, T5).astype(f32)
    w = (2.0 ** rng.integers(0, 3, len(keys))).astype(f32)
    grad = (np.concatenate(grad) * w[:, None]).astype(f32)
    order = np.argsort(B._pack(keys[:, 0], keys[:, 1], keys[:, 2]))
    rows = np.concatenate([dist[:, None], grad, w[:, None]], 1).astype(f32)
    return keys[order], rows[order]


def test_designed_map_on_the_edge_through_every_reader(pkg, O):
    """gsdf_merge_raw accepts voxels at -2^20 and 2^20 - 1 on every axis and refuses the rows at 2^20 and -2^20 - 1 (GSDF_ERR_KEY_RANGE,
    the other rows of the call are merged); then every reader of the map on it: export, get_voxels, query (both map types), the
    mesh, the raycaster, grow."""
    W, H = 64, 48
    K = pkg.synth.intrinsics(W, H)
    keys, rows = _designed_map()                                        # (z, y, x) order
    assert keys.min() == -OFF and keys.max() == OFF - 1 and len(keys) == 60 * 11 * 60 + 2 * 216
    raw = rows.copy()
    raw[:, 0] = rows[:, 0] * rows[:, 4]
    assert np.array_equal((raw[:, 0] / raw[:, 4]).view(np.uint32), rows[:, 0].view(np.uint32))
    rng = np.random.default_rng(5)
    perm = rng.permutation(len(keys))
    g = pkg.GradSdf(VS, T5, W, H, K, capacity_log2=19)
    g.merge_raw(keys[perm], raw[perm])                                  # accepted
    o = O.Oracle(VS, T5, W, H, K)
    o.set_map(keys, rows)
    # export: (z, y, x) order, the input bit for bit
    for raw_flag, want in ((False, rows), (True, raw)):
        kg, pg = g.export(sorted=True, raw=raw_flag)
        assert np.array_equal(kg, keys) and np.array_equal(pg.view(np.uint32), want.view(np.uint32))
    ko, po = o.export()
    assert np.array_equal(ko, keys) and np.array_equal(po.view(np.uint32), rows.view(np.uint32))
    # get_voxels: the voxels on the edge, and one step beyond on every axis (not found, no error)
    on_edge = np.flatnonzero((keys == -OFF).any(axis=1) | (keys == OFF - 1).any(axis=1))
    assert len(on_edge) > 500
    beyond = []
    for i in on_edge[:: max(1, len(on_edge) // 200)]:
        for a in range(3):
            if keys[i, a] in (-OFF, OFF - 1):
                b = keys[i].copy()
                b[a] += -1 if keys[i, a] == -OFF else 1
                beyond.append(b)
    beyond = np.array(beyond, np.int32)
    assert not _in_range(beyond).any()
    got, found = g.get_voxels(np.concatenate([keys[on_edge], beyond]))
    assert found[:len(on_edge)].all() and not found[len(on_edge):].any()
    assert np.array_equal(got[:len(on_edge)].view(np.uint32), rows[on_edge].view(np.uint32)) and (got[len(on_edge):] == 0).all()
    # query: points that round to the voxels on the edge and to the ones just beyond (float spacing at 20971 m is 2 mm)
    probe = np.concatenate([keys[on_edge], beyond]).astype(np.float64)
    pts = ((probe + rng.uniform(-0.3, 0.3, probe.shape)) * float(VS)).astype(f32)
    dg, gg, wg = g.query(pts)
    do, go, wo = o.query(pts)
    assert (wo[:len(on_edge)] > 0).mean() > 0.9 and not (wo[len(on_edge):] > 0).all()
    for a, b in ((dg, do), (gg, go), (wg, wo)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # the mesh: the oracle's sweep on the same voxels, bit for bit (a cube with a corner beyond the edge has a missing corner).  The
    # oracle sweeps the bounding box of its map, so the wall and the two corner cubes are meshed one at a time
    gm = pkg.GradSdf(VS, T5, W, H, K, capacity_log2=19)
    wall = (keys[:, 1] >= 45) & (keys[:, 1] <= 55) & (keys[:, 0] >= OFF - 60) & (np.abs(keys[:, 2]) <= 30)
    low = (keys < -OFF + 6).all(axis=1)
    n_tris = []
    for part in (wall, low, ~wall & ~low):
        gm.reset()
        gm.merge_raw(keys[part], raw[part])
        om = O.Oracle(VS, T5, W, H, K)
        om.set_map(keys[part], rows[part])
        tg, to = gm.extract_mesh(), om.extract_mesh()
        assert tg.shape == to.shape and tg.shape[0] > 20
        assert np.array_equal(tg.view(np.uint32), to.view(np.uint32))
        n_tris.append(tg.shape[0])
    assert n_tris[0] > 5000
    assert gm.extract_mesh().shape[0] + n_tris[0] + n_tris[1] == g.extract_mesh().shape[0]      # and the whole map's mesh is their sum
    gm.close()
    # the raycaster, looking along the edge: the camera 0.5 m inside the last packable x, looking down +y at the wall 1 m away;
    # the right of the image leaves the packable range.  The criteria of test_raycast_matches_definition_and_input_depth
    R = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], f32)
    t = np.array([(OFF - 26) * float(VS), 0, 0], f32)
    zg, ng = g.raycast(R, t)
    zo, no = o.raycast(R, t)
    hit_g, hit_o = zg > 0, zo > 0
    assert (hit_g == hit_o).mean() > 0.999
    both = hit_g & hit_o
    assert both.mean() > 0.5 and not hit_o[:, -4:].any() and hit_o[:, :W // 2].all()
    dz = np.abs(zg - zo)[both]
    assert np.percentile(dz, 99.9) <= TOL and np.median(dz) <= 1e-6
    assert np.percentile(np.abs(ng - no)[:, both], 99.9) <= 1e-3
    # grow by one doubling: the export stays
    g.grow(20)
    kg, pg = g.export(sorted=True, raw=True)
    assert np.array_equal(kg, keys) and np.array_equal(pg.view(np.uint32), raw.view(np.uint32))
    # rows beyond the edge are refused, the other rows of the call are merged
    more_k = np.array([[OFF, 0, 0], [5, 5, 5], [0, -OFF - 1, 0], [0, 0, OFF], [5, 5, 6]], np.int32)
    more_p = np.tile(np.array([0.01, 0, 0, 1, 1], f32), (5, 1))
    with pytest.raises(pkg.GsdfError) as e:
        g.merge_raw(more_k, more_p)
    assert e.value.code == pkg.binding.ERR_KEY_RANGE
    assert g.count() == len(keys) + 2
    got, found = g.get_voxels(more_k)
    assert list(found) == [False, True, False, False, True]
    assert np.array_equal(got[[1, 4]].view(np.uint32), more_p[[1, 4]].view(np.uint32))
    g.close()
    # the base map type: k_query_base at points whose 8-corner cube straddles the edge
    gb = pkg.GradSdf(VS, T5, W, H, K, capacity_log2=19, map_type=pkg.MAP_BASE)
    gb.merge_raw(keys[perm], raw[perm])
    m = B.BaseMap.from_export(keys, rows, VS, T5)
    sel = on_edge[:: max(1, len(on_edge) // 400)]
    cube = keys[sel].astype(np.float64) + np.where(keys[sel] == -OFF, -1.0, 0.0)      # the cube's low corner: one below the low edge
    pts = ((cube + rng.uniform(0.05, 0.95, cube.shape)) * float(VS)).astype(f32)
    inside = ((keys[sel].astype(np.float64) - 1 + rng.uniform(0.05, 0.95, cube.shape)) * float(VS)).astype(f32)
    pts = np.concatenate([pts, inside])
    d, gr, w = gb.query(pts)
    wr, dr, grr = m.sample(pts)
    assert (wr > 0).any() and (wr == 0).any()
    assert np.array_equal(w.view(np.uint32), wr.view(np.uint32))
    assert np.array_equal(d.view(np.uint32), dr.view(np.uint32))
    assert np.array_equal(gr.view(np.uint32), grr.view(np.uint32))
    gb.close()


# ---- C. odd depth values ---------------------------------------------------------------------------------------------------------

# isolated pixels, 14 apart and at least 8 from the border (no window holds two of them, none is reached by the reflection)
ODD = [(8, 8, -1.5), (8, 22, np.inf), (8, 36, -np.inf), (8, 50, 1e30), (22, 8, 1e-40), (22, 22, -0.0)]
ODD_NAN = (22, 36, np.nan)


def _odd_frames(pkg, n, with_nan=False):
    W, H = 64, 48
    seq = pkg.synth.Sequence("tum", W, H, n_frames=n, seed=1)
    frames = []
    for i in range(n):
        d, R, t = seq.frame(i)
        d = d.copy()
        for y, x, v in ODD + ([ODD_NAN] if with_nan else []):
            d[y, x] = f32(v)
        frames.append((d, R, t))
    assert frames[0][0][22, 8] > 0 and frames[0][0][22, 8] < np.finfo(f32).tiny          # the denormal survives the cast
    return seq, frames


def test_odd_depth_normals(pkg, O):
    """-1.5, +-inf, 1e30, a denormal, -0 and NaN in the depth image: `z != 0 ? 1 / z : 0` (NormalEstimator.h:183-187) is 1 / z = inf
    for the denormal in the oracle -- on the GPU only if neither the comparison nor the division flushes denormals -- and -0 for
    -inf; a negative depth enters its neighbours' box sums, +inf is a hole.  The same non-finite mask, the same bits elsewhere."""
    seq, frames = _odd_frames(pkg, 1, with_nan=True)
    W, H = seq.W, seq.H
    o = O.Oracle(VS, T5, W, H, seq.K)
    d_clean = seq.frame(0)[0]
    n_clean = o.normals(d_clean)
    assert np.isfinite(n_clean).all()
    only_denormal = d_clean.copy()
    only_denormal[22, 8] = f32(1e-40)
    bad = ~np.isfinite(o.normals(only_denormal)).all(axis=0)
    assert int(bad.sum()) == 121 and bad[17:28, 3:14].all()             # the premise: one 11 x 11 window, by the denormal alone
    n_o = o.normals(frames[0][0])
    assert int((~np.isfinite(n_o).all(axis=0)).sum()) == 2 * 121       # the denormal's window and the NaN's
    changed = (n_o.view(np.uint32) != n_clean.view(np.uint32)).any(axis=0)
    assert int(changed.sum()) == 7 * 121                                # every odd pixel changes the 121 normals of its window
    g = pkg.GradSdf(VS, T5, W, H, seq.K, capacity_log2=14)
    _bits_equal_where_finite(g.normals(frames[0][0]), n_o)
    g.close()


@pytest.mark.parametrize("flags", [None, 4, 512], ids=LIB_IDS)
def test_odd_depth_fusion_and_tracking(pkg, O, flags):
    """Two such frames (without the NaN pixel) through the carriers of part A: the odd pixels fail the range gate themselves, their
    neighbours are fused with the normals the odd values left them -- around the denormal a non-finite one, which the reference
    fuses (module docstring).  Then one tracker pass of a third such frame against the map of two clean frames."""
    seq, frames = _odd_frames(pkg, 3)
    W, H = seq.W, seq.H
    lib = None if flags is None else pkg.binding.load_test_lib()
    nu, nv = _fuse_carriers_against_oracle(pkg, O, W, H, seq.K, 11, frames[:2], lib=lib, flags=flags or 0)
    o = O.Oracle(VS, T5, W, H, seq.K)
    a, b = o.update(*frames[0])
    assert (~np.isfinite(o.export()[1][:, 1:4]).all(axis=1)).sum() > 1000         # the premise: voxels with a NaN gradient exist
    if flags is None:
        conv = _frame_loop_equals_two_calls(pkg, O, W, H, seq.K, 11, frames)
        print("MEASURED converged flags of the two tracked odd frames:", conv)
    # one pass of the tracker: frame 2 (odd pixels) against the clean frames 0 and 1
    g = _edge_ctx(pkg, W, H, seq.K, flags)
    o = O.Oracle(VS, T5, W, H, seq.K)
    for i in range(2):
        g.update(*seq.frame(i))
        o.update(*seq.frame(i))
    p0 = pose7_from(O, seq.frame(1)[1], seq.frame(1)[2])
    n0 = g.stats()["n_hit"]
    cg, pg, passes = g.track(frames[2][0], p0, iters=1)
    co, po, used, trace, hits = o.track(frames[2][0], p0, iters=1)
    assert passes == used == 1 and int(hits[0]) > 1000
    assert g.stats()["n_hit"] - n0 == int(hits[0])
    assert np.abs(pg - po).max() <= TOL
    g.close()
