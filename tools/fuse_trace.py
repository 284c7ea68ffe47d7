#!/usr/bin/env python3
"""Per-workgroup timeline of one k_fuse launch (test build, debug bit 64: thread 0 of every workgroup stores a time stamp at
each phase boundary; 100 MHz clock).  Prints the phase durations by tile colour, when workgroups start, and how many
workgroups are in which phase over the launch, and what the launch does behind its last tile (the epilogue: the per-tile tail up
to the arrival ticket's answer, the steps of the launch's last workgroup, the normals workgroups of the next frame).
usage: fuse_trace.py [frame_index (default 20)] [extra debug flags] [scene (tum)] [mode (gt)]
mode gt:       frames fused at their ground-truth poses (gsdf_update_dev), the last one traced: no head, no riders, no log row
mode tracked:  the launch bench.py times -- the bench stream (frame 0 at its pose, then gsdf_track_and_fuse_dev with the next frame
               named ahead), frame `frame_index` traced: k_fuse<2048, true, true>.  Also prints the deferred list's length for
               every frame of the stream up to it (one sync per frame: a tool, not a timing)"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G
pkg = G.package()
last = int(sys.argv[1]) if len(sys.argv) > 1 else 20
extra = int(sys.argv[2]) if len(sys.argv) > 2 else 0
mode = sys.argv[4] if len(sys.argv) > 4 else "gt"
assert mode in ("gt", "tracked")
n = last + (2 if mode == "tracked" else 1)
scene = sys.argv[3] if len(sys.argv) > 3 else "tum"          # "spheres": the object-scan scene of C1 / C4 (most tiles background)
seq = pkg.synth.Sequence(scene, 640, 480, n_frames=n, seed=0) if scene == "tum" else pkg.synth.Sequence(scene, 640, 480, n_frames=n, seed=0, step_deg=360.0 * 4 / 2000)
vs = np.float32(0.01); T = np.float32(10) * vs
frames = [seq.frame(i) for i in range(n)]
L = pkg.binding.load_test_lib()
g = pkg.GradSdf(vs, T, 640, 480, seq.K, capacity_log2=22, lib=L)
dev = [g.upload(f[0]) for f in frames]
if mode == "gt":
    for i in range(n - 1):
        g.update_dev(dev[i], frames[i][1], frames[i][2])
    g.sync()
    g.debug_flags(64 | extra)
    g.update_dev(dev[n - 1], frames[n - 1][1], frames[n - 1][2])
    g.sync()
else:
    from bench import quat_to_R
    d0, R0, t0 = frames[0]
    p0 = np.concatenate([t0, pkg.synth.R_to_quat_np(R0).astype(np.float32)]).astype(np.float32)
    # an untimed window first, as bench.py's burn-in has run one before anything it times (table warm, host's hints settled)
    for window in range(2):
        g.reset()
        g.update_dev(dev[0], quat_to_R(p0[3:]), t0)
        g.set_pose(p0)
        lens, seen = [], 0
        for i in range(1, last):
            g.track_and_fuse_ahead_dev(dev[i], dev[i + 1])
            if window == 1:                                       # the list's length per launch: what n_deferred grew by
                g.sync()
                st = g.stats()
                lens.append(int(st["n_deferred"]) - seen); seen = int(st["n_deferred"])
    g.sync()
    print("deferred list per launch, frames 1..%d of the stream: %s" % (last - 1, lens))
    print("   driver window (frames 6..%d): median %d, max %d entries" % (last - 1, int(np.median(lens[5:])), max(lens[5:])))
    timeouts0 = g.stats()["fuse_timeouts"]
    g.debug_flags(64 | extra)
    g.track_and_fuse_ahead_dev(dev[last], dev[last + 1])
    g.sync()
    st = g.stats()
    print("tracked frame %d: converged %d, passes %d, fuse_timeouts in the launch %d" % (last, st["converged"], st["track_passes"], st["fuse_timeouts"] - timeouts0))
NW = 1200                                # fusion tiles; the normals workgroups' rows follow them, the last workgroup's row is 2047
NROWS = 2048
buf = (ctypes.c_ulonglong * (NROWS * 16))()
assert L.gsdf_debug_trace(g.h, buf, NROWS) == 0
rows = np.array(list(buf), dtype=np.int64).reshape(NROWS, 16)
t = rows[:NW]
t0 = t[:, 0].min()
ts = (t[:, :11] - t0) / 100.0          # us
word = t[:, 15]                          # tile (x | y << 16) | bands << 32 | list entries of the tile's flush << 36
tile = word & 0xFFFFFFFF; tx = tile & 0x7FFF; ty = (tile >> 16) & 0x7FFF
colour = (tx & 1) + 2 * (ty & 1)
xcc = t[:, 14] >> 32
hw = t[:, 14] & 0xFFFFFFFF
npass = (word >> 32) & 0xF
single = npass == 1
print("launch span %.1f us; workgroups %d, single band %d; per XCC: %s" % (ts[:, 10].max(), NW, single.sum(), np.bincount(xcc.astype(int), minlength=8).tolist()))
empty = npass == 0
if empty.any():
    life = ts[empty, 10] - ts[empty, 0]
    print("tiles without a band: %d; their lives %.2f us median / %.2f p90 / %.2f max; slot time %.0f us of %.0f us (all workgroups); the last of them starts at %.1f us" % (
        empty.sum(), np.median(life), np.percentile(life, 90), life.max(), life.sum(), (ts[:, 10] - ts[:, 0]).sum(), ts[empty, 0].max()))
    band = ~empty
    print("tiles with a band: %d; lives %.1f us median / %.1f p90 / %.1f max; first starts %.1f, last starts %.1f, last ends %.1f us" % (
        band.sum(), np.median(ts[band, 10] - ts[band, 0]), np.percentile(ts[band, 10] - ts[band, 0], 90), (ts[band, 10] - ts[band, 0]).max(),
        ts[band, 0].min(), ts[band, 0].max(), ts[band, 10].max()))
names = ["prologue", "walk", "keys", "wait", "lookup(w0)", "lookup(all)", "rec loads", "stores", "drain+flag", "tail"]
d = np.diff(ts[:, :11], axis=1)
print("phase durations, us (mean | median | p90) over single-band workgroups")
for c in list(range(4)) + [None]:
    sel = single & ((colour == c) if c is not None else True)
    print(" colour %s (%d tiles): total %.1f" % (c if c is not None else "all", sel.sum(), (ts[sel, 10] - ts[sel, 0]).mean()))
    for k, nm in enumerate(names):
        x = d[sel, k]
        print("    %-12s %6.2f | %6.2f | %6.2f" % (nm, x.mean(), np.median(x), np.percentile(x, 90)))
pl = (t[:, 11] - t[:, 0]) / 100.0; ps = (t[:, 12] - t[:, 0]) / 100.0
print("prologue detail (single band, mean us): pixel loads arrived %.2f, statistics reduced %.2f, decisions made %.2f" % (pl[single].mean(), ps[single].mean(), d[single, 0].mean()))
# start times: the dispatch rounds
st = np.sort(ts[:, 0])
print("start times us: wg 0 %.1f, 256 %.1f, 511 %.1f, 512 %.1f, 600 %.1f, 800 %.1f, 1000 %.1f, 1199 %.1f" % tuple(st[[0, 256, 511, 512, 600, 800, 1000, 1199]]))
# occupancy of phases over time
edges = np.arange(0, ts[:, 10].max() + 2, 2.0)
print("time   running  prologue walk  flush(wait) flush(other)")
for a in edges[:-1]:
    m = a + 1.0
    run = (ts[:, 0] <= m) & (ts[:, 10] > m)
    pro = (ts[:, 0] <= m) & (ts[:, 1] > m)
    wk = (ts[:, 1] <= m) & (ts[:, 2] > m)
    wt = (ts[:, 3] <= m) & (ts[:, 4] > m)
    fl = (ts[:, 2] <= m) & (ts[:, 10] > m) & ~wt
    print("%5.0f  %6d  %6d  %5d  %6d  %6d" % (a, run.sum(), pro.sum(), wk.sum(), wt.sum(), fl.sum()))
# per CU (XCC, SE, SH, CU of HW_ID): how many workgroups it ran, when its last one ended; slot time used
cu = (xcc << 16) | (hw & 0xFF00)
ids = np.unique(cu)
cnt = np.array([(cu == i).sum() for i in ids]); end = np.array([ts[cu == i, 10].max() for i in ids]); busy = np.array([(ts[cu == i, 10] - ts[cu == i, 0]).sum() for i in ids])
span = ts[:, 10].max()
print("CUs seen: %d; workgroups per CU: %s" % (len(ids), dict(zip(*np.unique(cnt, return_counts=True)))))
print("end of a CU's last workgroup, us: min %.1f p10 %.1f median %.1f p90 %.1f max %.1f" % (end.min(), np.percentile(end, 10), np.median(end), np.percentile(end, 90), end.max()))
print("slot time used: %.0f of %.0f wg-us (2 slots x %d CUs x %.1f us) = %.2f; mean workgroup life %.1f us" % (busy.sum(), 2 * len(ids) * span, len(ids), span, busy.sum() / (2 * len(ids) * span), (ts[:, 10] - ts[:, 0]).mean()))
for k in sorted(set(cnt)):
    print("   CUs with %d workgroups: %d, their last end %.1f us (mean)" % (k, (cnt == k).sum(), end[cnt == k].mean()))
life = ts[:, 10] - ts[:, 0]
order = np.argsort(ts[:, 0])
for a, b in ((0, 512), (512, 1024), (1024, NW)):
    sel = order[a:b]
    print("workgroups %4d..%4d by start: start %.1f..%.1f, mean life %.1f, walk %.1f, end %.1f..%.1f" % (a, b - 1, ts[sel, 0].min(), ts[sel, 0].max(), life[sel].mean(), d[sel, 1].mean(), ts[sel, 10].min(), ts[sel, 10].max()))
# ---- the epilogue: what happens behind a workgroup's last band, and behind the launch's last tile
ran = t[:, 13] > 0
tail = (t[ran, 13] - t[ran, 10]) / 100.0
work = ran & (npass > 0)
tail_w = (t[work, 13] - t[work, 10]) / 100.0
print("epilogue, per tile (stamp 10 -> ticket answered), us: all %d tiles median %.2f p90 %.2f max %.2f; the %d with a band median %.2f p90 %.2f" % (
    ran.sum(), np.median(tail), np.percentile(tail, 90), tail.max(), work.sum(), np.median(tail_w), np.percentile(tail_w, 90)))
lr = rows[2047]
last10 = t[:, 10].max()
if lr[0] > 0:
    e = (lr[:5] - last10) / 100.0
    print("last workgroup (%d, list of %d entries), us after the last tile's stamp 10: ticket answered %.2f, list length known %.2f, "
          "adds issued %.2f, bookkeeping stored %.2f, all drained (end of the fusion part) %.2f" % (lr[6], lr[5], e[0], e[1], e[2], e[3], e[4]))
    via_flush = int(((word >> 36) & 0xFFFFF).sum())
    print("   list entries by route: %d through a tile's flush (near tile, or expired wait: see fuse_timeouts), %d one by one from the walk (LDS table full)" % (
        via_flush, int(lr[5]) - via_flush))
    rid = rows[NW:2047]
    rid = rid[rid[:, 13] > 0]
    if len(rid):
        print("   normals workgroups of the next frame: %d, start %.2f .. %.2f us, last one ends %.2f us after the launch's start = %.2f us relative to the end of the fusion part" % (
            len(rid), (rid[:, 0].min() - t0) / 100.0, (rid[:, 0].max() - t0) / 100.0, (rid[:, 13].max() - t0) / 100.0, (rid[:, 13].max() - lr[4]) / 100.0))
    print("   end of the fusion part %.2f us after the launch's first stamp" % ((lr[4] - t0) / 100.0))
np.save(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpurun_out", "fuse_trace.npy"), t)
g.close()
