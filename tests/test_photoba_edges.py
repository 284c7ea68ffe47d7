"""The premises of tests/test_gpu_photoba_edges.py, not gpu: on the oracle's PhotoBA and the numpy restatement
(tests/ba_pose_full_ref.py) alone, on the 33x21 scenes of tests/photoba_edge_scenes.py.  Each test is a condition the GPU
comparisons rest on -- the reference's own uncertainty is a fifth of the bar or less, the keyframe ids / the border pixels / the
distance-step parameters move every compared quantity by a multiple of its bar, no inside/outside decision is a coin toss, and no
stop decision of optimize() is within reach of the energy's uncertainty.  Run with -s for the measured values."""
import numpy as np
import pytest

import ba_pose_full_ref as REF
import photoba_edge_scenes as S

BAR = 1e-4                      # the project's bar: energy relative, poses and distances absolute
E_OPT = 3e-3                    # the energy uncertainty of optimize() (the reference's single-float sum), tests/test_photoba.py

_cpu = {}


class _Cpu:
    """a case on the oracle's own map: the restatement's observations and system, the oracle's energy and pose step"""

    def __init__(self, pkg, O, name):
        sc = self.sc = S.scene(pkg, O, name)
        self.o = sc.oracle_map(O)
        self.keys, self.pay = self.o.export()
        self.vis = self.o.export_vis(2)
        self.obs = REF.observations(self.keys, self.pay, self.vis, sc.seq.K, sc.vs, sc.imgs, sc.Pp, sc.idx)
        self.H, self.b = REF.system(self.obs)
        ba = O.PhotoBA(self.o, sc.imgs, sc.Pp, sc.idx)
        self.E64 = ba.energy_f64()
        ba.solve_pose()
        self.P_oracle = ba.poses()


def _case(pkg, O, name):
    if name not in _cpu:
        _cpu[name] = _Cpu(pkg, O, name)
    return _cpu[name]


def _fresh(O, sc, imgs=None, poses=None, idx=None, reg_weight=10.0):
    """(oracle map, PhotoBA) on a map of its own: solve_dist and optimize change it"""
    o = sc.oracle_map(O)
    return o, O.PhotoBA(o, sc.imgs if imgs is None else imgs, sc.Pp if poses is None else poses, sc.idx if idx is None else idx,
                        reg_weight)


def _dist(o):
    return o.export()[1][:, 0].astype(np.float64)


@pytest.mark.parametrize("name", list(S.CASES))
def test_conditioning_and_edge_decisions(pkg, O, name):
    """u = max |decoupled step in float32 - in float64| of the restatement <= 2e-5, a fifth of the bar (measured: 5e-8 .. 5e-7);
    the oracle's solve_pose within 1e-4 of the float64 step (measured: <= 8e-7); the restatement's energy is the oracle's
    energy_f64 to 1e-6 relative for every id list; the helper's projection is the restatement's; and at most 2 observations per
    case whose inside / outside decision lies within 4 ulp of an image edge (measured: 0 everywhere)."""
    c = _case(pkg, O, name)
    sc = c.sc
    P32, _ = REF.decoupled_step(c.H, c.b, sc.Pp, np.float32)
    P64, _ = REF.decoupled_step(c.H, c.b, sc.Pp, np.float64)
    u = float(np.abs(P32.astype(np.float64) - P64).max())
    d_oracle = float(np.abs(c.P_oracle - P64).max())
    conds = [np.linalg.cond(c.H[6 * i:6 * i + 6, 6 * i:6 * i + 6]) for i in range(sc.n) if np.any(c.H[6 * i:6 * i + 6, 6 * i:6 * i + 6])]
    pr = S.projections(c.keys, c.pay, c.vis, sc.seq.K, sc.vs, sc.Pp, sc.idx)
    pr_all = S.projections(c.keys, c.pay, c.vis, sc.seq.K, sc.vs, sc.Pp, sc.idx, gate=False)
    at, of = S.border_share(pr)
    edge, edge_all = S.edge_decisions(pr), S.edge_decisions(pr_all)
    E_ref = REF.energy(c.obs)
    print("%-8s %6d voxels, %5d gated, %5d observations (%.1f %% at the border): u = %.2e, oracle vs float64 step %.2e, step %.2e, "
          "cond <= %.0f, E %.6g vs %.6g, edge decisions %d (gated) %d (all voxels)"
          % (name, len(c.keys), len(c.obs["rows"]), of, 100.0 * at / max(of, 1), u, d_oracle, np.abs(c.P_oracle - sc.Pp).max(),
             max(conds) if conds else 0.0, E_ref, c.E64, edge, edge_all))
    assert u <= 2e-5
    assert d_oracle < BAR
    assert E_ref == pytest.approx(c.E64, rel=1e-6, abs=0.0)
    assert np.array_equal(pr["rows"], c.obs["rows"]) and np.array_equal(pr["ok"], c.obs["seen"])
    assert pr_all["ok"].sum() > pr["ok"].sum()                       # (the distance step sees more than the gated voxels)
    assert edge <= 2 and edge_all <= 2
    # what the GPU tests assert bit for bit is exact here as well
    moved = np.abs(c.P_oracle - sc.Pp).reshape(sc.n, -1).max(axis=1)
    if name in ("n1", "twice"):
        assert c.E64 == 0.0 and np.array_equal(c.P_oracle, sc.Pp) and not np.any(c.b) and of > 0
    elif name.startswith("unseen"):
        assert np.array_equal(c.P_oracle[1], sc.Pp[1]) and not c.obs["seen"][:, 1].any() and moved[0] > 1e-3 and moved[2] > 1e-3
    else:
        assert c.E64 > 0 and moved.max() > 1e-3
    if name == "twice":
        assert np.any(c.H)                                           # N_j = 2: (1 - 1/N_j) J^T J stays, b = 0 makes the step zero


def test_the_ids_matter(pkg, O):
    """`subset` with its ids and with arange(6) in their place (same images, same poses): energy, pose step and distance step
    each differ by >= 100 x the bar they are compared at (measured: E 1.174 vs 5.498, pose 3.2e-2, distance 1.0e-1)"""
    c = _case(pkg, O, "subset")
    sc = c.sc
    out = []
    for idx in (sc.idx, np.arange(6)):
        o, ba = _fresh(O, sc, idx=idx)
        E = ba.energy_f64()
        ba.solve_pose()
        P = ba.poses()
        o2, ba2 = _fresh(O, sc, idx=idx)
        ba2.solve_dist()
        out.append((E, P, _dist(o2)))
    dE = abs(out[0][0] / out[1][0] - 1); dP = np.abs(out[0][1] - out[1][1]).max(); dD = np.abs(out[0][2] - out[1][2]).max()
    print("subset ids vs arange(6): E %.6g vs %.6g, pose step differs by %.2e, distance step by %.2e" % (out[0][0], out[1][0], dP, dD))
    assert out[0][0] == c.E64
    assert dE >= 100 * BAR and dP >= 100 * BAR and dD >= 100 * BAR


def test_the_border_matters(pkg, O):
    """n6 (33x21): +0.05 on the last row and the last column of every image and nothing else moves the oracle's energy, pose
    step and per-voxel distance step by >= 3 x the bar each is compared at on the GPU (measured: 3.6e-3 relative, 2.1e-3,
    2.5e-3), and >= 2 % of the gated observations are border observations (measured: 3.6 %; 3.3 - 4.4 % over the cases)."""
    c = _case(pkg, O, "n6")
    sc = c.sc
    alt = S.border_altered(sc.imgs)
    assert np.array_equal(alt[:, :-1, :-1], sc.imgs[:, :-1, :-1]) and np.all(alt[:, -1] != sc.imgs[:, -1]) and np.all(alt[:, :, -1] != sc.imgs[:, :, -1])
    out = []
    for imgs in (sc.imgs, alt):
        o, ba = _fresh(O, sc, imgs=imgs)
        E = ba.energy_f64()
        ba.solve_pose()
        P = ba.poses()
        o2, ba2 = _fresh(O, sc, imgs=imgs)
        ba2.solve_dist()
        out.append((E, P, _dist(o2)))
    dE = abs(out[1][0] / out[0][0] - 1); dP = np.abs(out[0][1] - out[1][1]).max(); dD = np.abs(out[0][2] - out[1][2]).max()
    at, of = S.border_share(S.projections(c.keys, c.pay, c.vis, sc.seq.K, sc.vs, sc.Pp, sc.idx))
    print("border pixels + 0.05: energy %.2e relative, pose step %.2e, distance step %.2e; %d of %d gated observations at the border"
          % (dE, dP, dD, at, of))
    assert dE >= 3 * BAR and dP >= 3 * BAR and dD >= 3 * BAR
    assert at >= 0.02 * of


def test_damping_and_regulariser(pkg, O):
    """solve_dist(0.5) moves every voxel by half of solve_dist(1.0): 0.5 b / H is exactly half of b / H, each new distance is
    rounded once, so (d_half - d0) - (d_one - d0) / 2 is below 1 ulp of the largest distance (measured: 4e-9, 1 ulp = 1.5e-8).
    reg_weight = 1 against 10 moves the step by >= 100 x the distance bar (measured: 0.085)."""
    sc = S.scene(pkg, O, "subset")
    d = {}
    for key, (reg, damping) in {"one": (10.0, 1.0), "half": (10.0, 0.5), "reg1": (1.0, 1.0)}.items():
        o, ba = _fresh(O, sc, reg_weight=reg)
        d0 = _dist(o)
        ba.solve_dist(damping)
        d[key] = _dist(o)
    assert np.abs(d["one"] - d0).max() > 100 * BAR
    ulp = float(np.spacing(np.float32(max(np.abs(v).max() for v in list(d.values()) + [d0]))))
    half = np.abs((d["half"] - d0) - 0.5 * (d["one"] - d0)).max()
    dreg = np.abs(d["reg1"] - d["one"]).max()
    print("damping 0.5 is half of damping 1 to %.2e (1 ulp = %.2e); reg_weight 1 vs 10: %.3f" % (half, ulp, dreg))
    assert half <= ulp
    assert dreg >= 100 * BAR


def test_stop_rule_margin_of_the_optimize_runs(pkg, O):
    """the two optimize() runs the GPU is compared on (S.OPTIMIZE_RUNS on `subset`, S.OPTIMIZE_MAX_IT iterations): every stop
    decision of the oracle's run is >= 3 x 3e-3 away from flipping.  Measured: TRUNC_L2(0.5) 1.174, 1.042, 1.019, 0.976, 0.989
    -- 2.1 % and 1.3 %; default loss from 1.5 x the perturbation 1.323, 1.085, 0.784, 0.647, 0.739 -- 28 % and 14 %.  The
    default loss from the default perturbation (1.174, 0.840, 0.833, ...) decides its first iteration at 8.4e-3: that is why
    its run starts elsewhere, and it is the contrast that shows the TRUNC_L2 gate acting inside the loop (> 10 x 3e-3 apart)."""
    sc = S.scene(pkg, O, "subset")
    runs = {}
    for name, (loss, lam, scale) in list(S.OPTIMIZE_RUNS.items()) + [("contrast", (None, 0.5, 1.0))]:
        o, ba = _fresh(O, sc, poses=sc.perturbed(scale))
        if loss is not None:
            ba.set_loss(loss, lam)
        conv, en = ba.optimize(S.OPTIMIZE_MAX_IT)
        margins = S.stop_rule_margins(en)
        print("optimize(%d), %s: converged %d, energies %s, margins %s" % (S.OPTIMIZE_MAX_IT, name, conv, [float(e) for e in en],
                                                                         ["%.2e" % m for m in margins]))
        if name != "contrast":
            assert len(margins) >= 1 and min(margins) >= 3 * E_OPT
        runs[name] = en
    assert min(S.stop_rule_margins(runs["contrast"])) < 3 * E_OPT      # (the reason of the other start)
    assert np.abs(runs["trunc_l2"][:3] / runs["contrast"][:3] - 1).max() > 10 * E_OPT
