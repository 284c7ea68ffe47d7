"""PhotoBA's decoupled sweeps on the GPU (k_ba_energy, k_ba_pose, k_ba_pose_reduce, k_ba_dist; csrc/gsdf_ba.hip) at the keyframe
sets, keyframe counts, image borders and fallback paths of tests/photoba_edge_scenes.py, FROM IDENTICAL STATE: the map is fused on
the GPU with vis_ on and exported; the oracle takes the GPU's voxel values (set_payload, identical key sets asserted), the numpy
restatement (tests/ba_pose_full_ref.py) takes (keys, payload, vis_).  tests/test_photoba_edges.py holds the premises (not gpu).

The bars are the project's: energy 1e-4 relative against energy_f64; poses 1e-4 against the oracle; distances 1e-4 on every voxel
against the oracle given the GPU's poses; the system bar of tests/test_gpu_ba_pose_full.py (_system_errors) for the 6x6 blocks and
b; the counters equal the restatement's counts up to the edge-decision count of the case (0 for every case here).  Every test
prints its worst values (-s); the docstrings carry them beside the bar."""
import numpy as np
import pytest

import ba_pose_full_ref as REF
import photoba_edge_scenes as S
from test_gpu_ba_pose_full import _system_errors

pytestmark = pytest.mark.gpu

BAR = 1e-4
E_OPT = 3e-3                    # optimize(): the reference's single-float energy sum (tests/test_photoba.py)
COUPLED = ("subset", "unseen50", "unseen64", "twice")


class _Gpu:
    """a context with the scene's frames fused, and its export"""

    def __init__(self, pkg, sc, frames=None, n_fused=None):
        self.sc = sc
        self.n_fused = sc.n_fused if n_fused is None else n_fused
        self.g = sc.gpu(pkg, frames)
        self.export()

    def export(self):
        self.keys, self.pay = self.g.export(sorted=True)
        kv, self.vis = self.g.export_vis()
        assert np.array_equal(kv, self.keys)

    def oracle(self, pkg, O):
        """the oracle map of the same frames holding the GPU's voxel values (the key sets are identical, or this asserts)"""
        return S.oracle_on(O, S.scene(pkg, O, self.sc.name, self.n_fused), self.keys, self.pay)


def _diagonal_only(Hm, n):
    out = np.zeros_like(np.asarray(Hm, np.float64))
    for i in range(n):
        out[6 * i:6 * i + 6, 6 * i:6 * i + 6] = Hm[6 * i:6 * i + 6, 6 * i:6 * i + 6]
    return out


def _energy_and_counters(G, o, O, imgs, poses, idx, tag):
    """gsdf_ba_energy against energy_f64 at 1e-4 relative (exactly 0 where the oracle's is), its counters against the
    restatement's gated voxels / observations up to the edge-decision count"""
    g, sc = G.g, G.sc
    e_g = g.ba_energy()
    e_o = O.PhotoBA(o, imgs, poses, idx).energy_f64()
    pr = S.projections(G.keys, G.pay, G.vis, sc.seq.K, sc.vs, poses, idx)
    allow = S.edge_decisions(pr)
    vox, obs = g.ba_counters()
    rv, ro = int(pr["ok"].any(axis=1).sum()), int(pr["ok"].sum())
    rel = abs(e_g / e_o - 1) if e_o else abs(e_g)
    print("%s: E gpu %.8g oracle %.8g (%.2e); counters gpu (%d, %d) restatement (%d, %d), allowance %d" % (tag, e_g, e_o, rel, vox, obs, rv, ro, allow))
    assert np.isfinite(e_g)
    assert e_g == pytest.approx(e_o, rel=BAR, abs=0.0)
    assert allow <= 2 and abs(vox - rv) <= allow and abs(obs - ro) <= allow
    return rel


def _compare(pkg, O, G, imgs, Pp, idx, tag, coupled=False, reg_weight=10.0, damping=1.0, setup=True, dist=True):
    """energy + counters, the 27 sums per keyframe (and the coupled blocks), one pose step, one distance step + counters, each
    from the state the GPU is in, at the bars.  Returns the worst values and the poses of both sides."""
    g, sc = G.g, G.sc
    n = len(idx)
    if setup:
        g.ba_setup(imgs, Pp, idx, reg_weight)
    assert np.array_equal(g.ba_poses(), Pp)
    o = G.oracle(pkg, O)
    m = {"E": _energy_and_counters(G, o, O, imgs, Pp, idx, tag)}
    # the system: what k_ba_pose + k_ba_pose_reduce summed, free of the conditioning of the solve
    Hg, bg = g.ba_pose_system()
    obs = REF.observations(G.keys, G.pay, G.vis, sc.seq.K, sc.vs, imgs, Pp, idx)
    assert REF.energy(obs) == pytest.approx(O.PhotoBA(o, imgs, Pp, idx).energy_f64(), rel=1e-6, abs=0.0)
    Hr, br = REF.system(obs)
    if coupled:
        m["H"], m["b"] = _system_errors(Hg, bg, Hr, br, n)
    else:
        m["H"], m["b"] = _system_errors(_diagonal_only(Hg, n), bg, _diagonal_only(Hr, n), br, n)
    assert np.array_equal(g.ba_poses(), Pp)
    # the pose step against the oracle
    ba = O.PhotoBA(o, imgs, Pp, idx, reg_weight)
    ba.solve_pose()
    g.ba_solve_pose()
    Po, Pg = ba.poses(), g.ba_poses()
    assert np.all(np.isfinite(Pg))
    m["pose"] = float(np.abs(Pg - Po).max())
    step_o = np.abs(Po - Pp).reshape(n, -1).max(axis=1)
    step_g = np.abs(Pg - Pp).reshape(n, -1).max(axis=1)
    for i in range(n):
        if np.array_equal(Po[i], Pp[i]):
            assert np.array_equal(Pg[i].view(np.uint32), Pp[i].view(np.uint32)), "keyframe %d (id %d) moved" % (i, idx[i])
        elif step_o[i] > 1e-3:
            assert step_g[i] > 1e-3, "keyframe %d (id %d) did not move" % (i, idx[i])
    worst = int(np.argmax(np.abs(Pg - Po).reshape(n, -1).max(axis=1)))
    print("%s: pose step gpu vs oracle %.2e (worst keyframe %d, id %d), steps %.2e .. %.2e" % (tag, m["pose"], worst, idx[worst], step_o.min(), step_o.max()))
    assert m["pose"] < BAR
    m["Po"], m["Pg"] = Po, Pg
    if not dist:
        return m
    # the distance step from identical state again: the oracle takes the GPU's poses
    ba2 = O.PhotoBA(o, imgs, Pg, idx, reg_weight)
    before = G.pay[:, 0].copy()
    ba2.solve_dist(damping)
    g.ba_solve_dist(damping)
    vox, nobs = g.ba_counters()
    pr = S.projections(G.keys, G.pay, G.vis, sc.seq.K, sc.vs, Pg, idx, gate=False)      # solveDist has no gate
    allow = S.edge_decisions(pr)
    rv, ro = int(pr["ok"].any(axis=1).sum()), int(pr["ok"].sum())
    ko, po = o.export()
    G.export()
    assert np.array_equal(G.keys, ko)
    err = np.abs(G.pay[:, 0] - po[:, 0])
    m["dist"] = float(err.max())
    j = int(np.argmax(err))
    at_border = bool((pr["ok"][j] & ((np.floor(pr["m"][j]) + 1 >= S.W) | (np.floor(pr["n"][j]) + 1 >= S.H))).any())
    print("%s: distance step gpu vs oracle %.2e (worst voxel %s, a border observation: %s), moved by %.2e; counters gpu (%d, %d) "
          "restatement (%d, %d), allowance %d" % (tag, m["dist"], G.keys[j], at_border, np.abs(po[:, 0] - before).max(), vox, nobs, rv, ro, allow))
    assert m["dist"] < BAR
    assert np.array_equal(G.pay[:, 1:], po[:, 1:])                                      # gradient and weight untouched
    if np.abs(po[:, 0] - before).max() > 1e-3:
        assert np.abs(G.pay[:, 0] - before).max() > 1e-3
    assert allow <= 2 and abs(vox - rv) <= allow and abs(nobs - ro) <= allow
    m["E2"] = _energy_and_counters(G, G.oracle(pkg, O), O, imgs, Pg, idx, tag + " (after the distance step)")
    return m


@pytest.mark.parametrize("name", S.TABLE)
def test_keyframe_sets_and_counts(pkg, O, name):
    """Every case of the table: energy (bar 1e-4 relative; measured: <= 3e-8), counters (equal; measured: equal, the allowance
    was 0 except 2 and 1 on n64 behind the pose step), the 27 sums per keyframe and b at the system bar -- with the coupled blocks
    for subset / unseen / twice -- (measured: blocks <= 1.5e-3 of the bound, b <= 1.2e-3 of it), the pose step (bar 1e-4; measured:
    <= 1.4e-6, on unseen; <= 5.3e-7 elsewhere), the distance step per voxel (bar 1e-4; measured: <= 1.5e-8).  n1, twice and the
    unseen keyframe: the input pose bit for bit, no NaN, E = 0 exactly for n1 and twice (measured: so)."""
    sc = S.scene(pkg, O, name)
    G = _Gpu(pkg, sc)
    try:
        m = _compare(pkg, O, G, sc.imgs, sc.Pp, sc.idx, name, coupled=name in COUPLED)
        Pg = m["Pg"]
        if name in ("n1", "twice"):
            assert m["E"] == 0.0 and np.array_equal(Pg, sc.Pp)
        elif name.startswith("unseen"):
            assert np.array_equal(Pg[1], sc.Pp[1]) and np.abs(Pg[0] - sc.Pp[0]).max() > 1e-3 and np.abs(Pg[2] - sc.Pp[2]).max() > 1e-3
        else:
            assert np.abs(Pg - sc.Pp).max() > 1e-3
    finally:
        G.g.close()


def test_image_border(pkg, O):
    """n6 on 33x21 frames, 3.6 % of the gated observations in the last row or column, and the same with only those pixels
    changed (+0.05): tests/test_photoba_edges.py shows that they move energy, pose step and distance step by >= 3 bars, so a
    wrong border branch of ba_interp / ba_grad / ba_sample3 cannot hide.  Bars as above.
    measured, original / altered pixels: energy 2e-8 / 2e-8, pose 4.8e-7 / 3.2e-7, distance 7.5e-9 / 7.5e-9, blocks 6.1e-4 / 7.4e-4
    and b 9.3e-4 / 6.8e-4 of their bounds, counters equal"""
    sc = S.scene(pkg, O, "n6")
    alt = S.border_altered(sc.imgs)
    out = []
    for tag, imgs in (("n6", sc.imgs), ("n6, border pixels + 0.05", alt)):
        G = _Gpu(pkg, sc)
        try:
            out.append(_compare(pkg, O, G, imgs, sc.Pp, sc.idx, tag))
            out[-1]["d"] = G.pay[:, 0].copy()
        finally:
            G.g.close()
    # the two inputs really went different ways on the GPU too
    assert np.abs(out[0]["Pg"] - out[1]["Pg"]).max() >= 3 * BAR and np.abs(out[0]["d"] - out[1]["d"]).max() >= 3 * BAR


def test_distance_step_parameters(pkg, O):
    """gsdf_ba_setup(reg_weight = 1) then gsdf_ba_solve_dist(damping = 0.5), per voxel against the oracle with the same arguments
    (bar 1e-4; measured: 7.5e-9, the step was 1.1e-1); gsdf_ba_solve_pose(damping = 0.3) is gsdf_ba_solve_pose(1.0) bit for bit
    (the reference does not use it)."""
    sc = S.scene(pkg, O, "subset")
    G = _Gpu(pkg, sc)
    try:
        g = G.g
        P = []
        for damping in (0.3, 1.0):
            g.ba_setup(sc.imgs, sc.Pp, sc.idx, 1.0)
            g.ba_solve_pose(damping)
            P.append(g.ba_poses().copy())
        assert np.array_equal(P[0].view(np.uint32), P[1].view(np.uint32)) and np.abs(P[0] - sc.Pp).max() > 1e-3
        # (the premise: either argument ignored would show as 0.085 / half the step, tests/test_photoba_edges.py)
        _compare(pkg, O, G, sc.imgs, sc.Pp, sc.idx, "subset, reg_weight 1, damping 0.5", reg_weight=1.0, damping=0.5)
    finally:
        G.g.close()


def test_whole_table_fallback_after_grow(pkg, O):
    """gsdf_grow drops PhotoBA's gate list and mean cache: energy, pose step, distance step and counters then walk the whole
    table (gate_list == nullptr) -- same bars, against oracle / restatement on the post-grow export, whose key set and values
    are those from before the grow.  A new gsdf_ba_setup restores the list path and agrees at the same bars.
    measured, whole table / list again: energy 3e-8 / 3e-8, pose 4.6e-7 / 5.1e-7, distance 7.5e-9 / 7.5e-9, blocks 1.2e-3 / 7.9e-4 and
    b 5.3e-4 / 5.4e-4 of their bounds, counters equal; list and whole-table energy on one map: the same float"""
    sc = S.scene(pkg, O, "subset")
    G = _Gpu(pkg, sc)
    try:
        g = G.g
        g.ba_setup(sc.imgs, sc.Pp, sc.idx)
        e_list = g.ba_energy()
        c_list = g.ba_counters()
        keys0, pay0, vis0 = G.keys, G.pay, G.vis
        g.grow(S.CAPACITY_LOG2 + 1)
        assert g.capacity_log2() == S.CAPACITY_LOG2 + 1
        G.export()
        assert np.array_equal(G.keys, keys0) and np.array_equal(G.pay.view(np.uint32), pay0.view(np.uint32)) and np.array_equal(G.vis, vis0)
        _compare(pkg, O, G, sc.imgs, sc.Pp, sc.idx, "subset, whole table", coupled=True, setup=False)
        # (before any step the whole-table energy is the list's: the same terms, summed in double in another order)
        g.ba_setup(sc.imgs, sc.Pp, sc.idx)
        m = _compare(pkg, O, G, sc.imgs, sc.Pp, sc.idx, "subset, list again", coupled=True)
    finally:
        G.g.close()
    # the energy of the list path before the grow and of the whole-table path after it, on one unchanged map
    G = _Gpu(pkg, sc)
    try:
        g = G.g
        g.ba_setup(sc.imgs, sc.Pp, sc.idx)
        g.grow(S.CAPACITY_LOG2 + 1)
        e_table = g.ba_energy()
        print("energy: list %.9g, whole table %.9g; counters %s / %s" % (e_list, e_table, c_list, g.ba_counters()))
        assert e_table == pytest.approx(e_list, rel=1e-6) and g.ba_counters() == c_list     # (double sums rounded to one float)
    finally:
        G.g.close()


def test_map_changed_between_two_calls(pkg, O):
    """frames 0..38 fused, gsdf_ba_setup with subset's ids, gsdf_ba_energy; frame 39 fused; gsdf_ba_energy, counters and
    gsdf_ba_solve_pose are then those of the 40-frame map (the gate list is rebuilt, no mean cache is trusted), the first energy
    that of the 39-frame map.  Bars as above.  measured: energy 4e-9 (40 frames), pose 4.0e-7, blocks 5.7e-4 and b 7.9e-4 of their bounds, counters equal"""
    sc = S.scene(pkg, O, "subset")
    G = _Gpu(pkg, sc, frames=sc.frames[:39], n_fused=39)
    try:
        g = G.g
        g.ba_setup(sc.imgs, sc.Pp, sc.idx)
        n39 = len(G.keys)
        _energy_and_counters(G, G.oracle(pkg, O), O, sc.imgs, sc.Pp, sc.idx, "39 frames")
        g.update(*sc.frames[39])
        G.n_fused = 40
        G.export()
        assert len(G.keys) > n39
        _compare(pkg, O, G, sc.imgs, sc.Pp, sc.idx, "40 frames, the setup of 39", setup=False, dist=False)
    finally:
        G.g.close()


def test_setup_replaced_and_a_rejected_setup(pkg, O):
    """one context: gsdf_ba_setup with n64's keyframes and a pose step, then gsdf_ba_setup with 2 keyframes (ids 40 and 9): every
    result is the oracle's / a fresh context's at the bars; a rejected gsdf_ba_setup (negative id) then leaves the 2-keyframe
    setup answering as before, bit for bit.  measured: pose 2.4e-7 against the oracle, 3e-8 against the fresh context, whose energy is the same float"""
    sc = S.scene(pkg, O, "n64")
    seq, vs, T, frames, imgs, P, Pp = S.stream(pkg, O)
    idx2 = np.array([40, 9], np.int32)
    G = _Gpu(pkg, sc)
    F = _Gpu(pkg, sc)
    try:
        g, f = G.g, F.g
        g.ba_setup(sc.imgs, sc.Pp, sc.idx)
        g.ba_solve_pose()
        assert np.abs(g.ba_poses() - sc.Pp).max() > 1e-3
        m = _compare(pkg, O, G, imgs[idx2], Pp[idx2], idx2, "2 keyframes after 64", dist=False)
        f.ba_setup(imgs[idx2], Pp[idx2], idx2)
        e_f = f.ba_energy()
        f.ba_solve_pose()
        # the rejected call, and the setup it must not have touched (the poses are those behind the step)
        with pytest.raises(pkg.binding.GsdfError) as err:
            g.ba_setup(imgs[idx2], Pp[idx2], [40, -1])
        assert err.value.code == pkg.binding.ERR_INVALID
        assert np.array_equal(g.ba_poses(), m["Pg"])
        H1, b1 = g.ba_pose_system()
        e1 = g.ba_energy()
        with pytest.raises(pkg.binding.GsdfError):
            g.ba_setup(imgs[idx2], Pp[idx2], [-7, 9])
        H2, b2 = g.ba_pose_system()
        assert H1.tobytes() == H2.tobytes() and b1.tobytes() == b2.tobytes() and g.ba_energy() == e1
        assert np.array_equal(g.ba_poses(), m["Pg"])
        # a fresh context on the same frames: another table, so sums in another order -- at the bars
        g.ba_setup(imgs[idx2], Pp[idx2], idx2)
        e_g = g.ba_energy()
        print("2 keyframes: replaced setup E %.8g, fresh context E %.8g; poses differ by %.2e" % (e_g, e_f, np.abs(f.ba_poses() - m["Pg"]).max()))
        assert e_g == pytest.approx(e_f, rel=BAR) and np.abs(f.ba_poses() - m["Pg"]).max() < BAR
    finally:
        G.g.close()
        F.g.close()


def test_optimize_default_loss_and_trunc_l2(pkg, O):
    """gsdf_ba_optimize on `subset`, S.OPTIMIZE_MAX_IT iterations, the runs of S.OPTIMIZE_RUNS (the default loss: the mean-cache
    path k_ba_energy<true> -> k_ba_pose<true, 4>; TRUNC_L2(0.5): k_ba_pose<false, 2> inside the loop): the same `converged`, the
    same number of energies, energies within 3e-3 relative, final poses within 1e-4; the oracle's run on the GPU's map keeps
    the stop-rule margin of tests/test_photoba_edges.py; and the TRUNC_L2 series lies > 10 x 3e-3 from the default-loss series
    of the same start (the gate was active inside the loop).  measured: energies 3.5e-6 (default loss) and 3.3e-6 (TRUNC_L2) relative, poses 3.4e-7 and
    1.9e-7; the TRUNC_L2 series 24 % above the default-loss series of the same start"""
    sc = S.scene(pkg, O, "subset")
    series = {}
    for name, (loss, lam, scale) in list(S.OPTIMIZE_RUNS.items()) + [("contrast", (None, 0.5, 1.0))]:
        G = _Gpu(pkg, sc)
        try:
            g = G.g
            Pp = sc.perturbed(scale)
            g.ba_setup(sc.imgs, Pp, sc.idx)
            if loss is not None:
                g.ba_set_loss(loss, lam)
            conv_g, en_g = g.ba_optimize(S.OPTIMIZE_MAX_IT)
            series[name] = en_g
            if name == "contrast":
                continue
            ba = O.PhotoBA(G.oracle(pkg, O), sc.imgs, Pp, sc.idx)
            if loss is not None:
                ba.set_loss(loss, lam)
            conv_o, en_o = ba.optimize(S.OPTIMIZE_MAX_IT)
            dP = np.abs(g.ba_poses() - ba.poses()).max()
            print("optimize, %s: gpu %s %s\n            oracle %s %s; worst energy %.2e relative, poses %.2e, margins %s"
                  % (name, conv_g, [float(e) for e in en_g], conv_o, [float(e) for e in en_o],
                     np.abs(en_g[:len(en_o)] / en_o[:len(en_g)] - 1).max(), dP, ["%.2e" % v for v in S.stop_rule_margins(en_o)]))
            assert min(S.stop_rule_margins(en_o)) >= 3 * E_OPT
            assert conv_g == conv_o and len(en_g) == len(en_o) >= 3
            assert np.allclose(en_g, en_o, rtol=E_OPT, atol=0)
            assert dP < BAR
            assert np.abs(g.ba_poses() - Pp).max() > 1e-3
        finally:
            G.g.close()
    k = min(len(series["trunc_l2"]), len(series["contrast"]))
    assert series["trunc_l2"][0] == pytest.approx(series["contrast"][0], rel=1e-6)          # the same start (two tables: float rounding)
    assert np.abs(series["trunc_l2"][1:k] / series["contrast"][1:k] - 1).max() > 10 * E_OPT


def test_arguments(pkg, O):
    """gsdf_ba_setup rejects what the sweeps cannot index, before anything is allocated or launched: a negative keyframe id (first
    or last position) and frames with W < 2 or H < 2 are GSDF_ERR_INVALID; n = 65 still is.  After a rejected first setup the
    context has none (gsdf_ba_energy says so) and still fuses and exports."""
    ERR = pkg.binding.ERR_INVALID
    sc = S.scene(pkg, O, "n6")
    G = _Gpu(pkg, sc)
    try:
        g = G.g
        for bad in ([-1, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, -1], [0, 1, 2, 3, 4, -2147483648]):
            with pytest.raises(pkg.binding.GsdfError) as err:
                g.ba_setup(sc.imgs, sc.Pp, bad)
            assert err.value.code == ERR and "frame_idx" in str(err.value)
            with pytest.raises(pkg.binding.GsdfError) as err:
                g.ba_energy()
            assert err.value.code == ERR and "not called" in str(err.value)
        with pytest.raises(pkg.binding.GsdfError) as err:
            g.ba_setup(np.zeros((65, S.H, S.W, 3), np.float32), np.tile(np.eye(4, dtype=np.float32), (65, 1, 1)), np.arange(65))
        assert err.value.code == ERR
        g.ba_setup(sc.imgs, sc.Pp, sc.idx)                                       # ... and a good one still goes through
        assert g.ba_energy() > 0
    finally:
        G.g.close()
    for W, H in ((1, 21), (33, 1)):
        seq = pkg.synth.Sequence("tum", W, H, n_frames=2, seed=0, noise=False)
        g = pkg.GradSdf(np.float32(0.02), np.float32(0.1), W, H, seq.K, capacity_log2=14)
        try:
            g.enable_vis(64)
            g.update(*seq.frame(0))
            n0 = g.count()
            assert n0 > 0
            with pytest.raises(pkg.binding.GsdfError) as err:
                g.ba_setup(np.zeros((1, H, W, 3), np.float32), np.eye(4, dtype=np.float32)[None], [0])
            assert err.value.code == ERR and "2 x 2" in str(err.value)
            with pytest.raises(pkg.binding.GsdfError) as err:
                g.ba_energy()
            assert err.value.code == ERR and "not called" in str(err.value)
            g.update(*seq.frame(1))
            keys, pay = g.export(sorted=True)
            assert len(keys) == g.count() >= n0 and np.all(np.isfinite(pay[:, [0, 4]]))     # (a 1-pixel-wide frame has no normals: 0 / 0)
        finally:
            g.close()
