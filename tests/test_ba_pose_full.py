"""PhotoBA's coupled pose step (solvePoseFull, PhotometricOptimizer.cpp:392-496), not gpu: the numpy restatement
tests/ba_pose_full_ref.py is tied to the oracle (its diagonal blocks solved one at a time are the oracle's solvePose, its energy
the oracle's), its known answers, its own float32-vs-float64 uncertainty on the scenes the GPU tests use, and the C-ABI."""
import os
import re

import numpy as np
import pytest

import ba_pose_full_ref as REF
from conftest import ROOT
from test_photoba import _oracle_map, _scene


class _Case:
    """a fused oracle map with perturbed keyframe poses, and the restatement's observations / system on it"""

    def __init__(self, pkg, O, n, extra_ids=(), scale=1.0):
        self.seq, self.vs, self.T, self.frames, self.imgs, self.P, Pp = _scene(pkg, O, n=n)
        self.Pp = (self.P + np.float32(scale) * (Pp - self.P)).astype(np.float32) if scale != 1.0 else Pp
        self.o = _oracle_map(O, self.seq, self.vs, self.T, self.frames)
        self.keys, self.pay = self.o.export()
        self.vis = self.o.export_vis(2)
        self.idx = np.concatenate([np.arange(n), np.asarray(extra_ids, int)]).astype(int)
        k = len(extra_ids)
        self.imgs_all = np.concatenate([self.imgs, self.imgs[:k]]) if k else self.imgs
        self.Pp_all = np.concatenate([self.Pp, self.Pp[:k]]) if k else self.Pp
        self.obs = REF.observations(self.keys, self.pay, self.vis, self.seq.K, self.vs, self.imgs_all, self.Pp_all, self.idx)
        self.H, self.b = REF.system(self.obs)


@pytest.fixture(scope="module")
def six(pkg, O):
    return _Case(pkg, O, 6)


def test_restatement_is_tied_to_the_oracle(pkg, O, six):
    """the restatement's diagonal blocks with its b, solved one 6 x 6 at a time, are the oracle's solvePose (1e-4, the project's
    bar), and its energy from A_ij is the oracle's energy_f64 (1e-6 relative)"""
    ba = O.PhotoBA(six.o, six.imgs, six.Pp, six.idx)
    assert REF.energy(six.obs) == pytest.approx(ba.energy_f64(), rel=1e-6)
    ba.solve_pose()
    for dtype in (np.float32, np.float64):
        Pn, _ = REF.decoupled_step(six.H, six.b, six.Pp, dtype)
        diff = np.abs(Pn - ba.poses()).max()
        print("decoupled step of the restatement (%s) vs oracle solve_pose: %.3e" % (dtype.__name__, diff))
        assert diff < 1e-4
    assert np.abs(ba.poses() - six.Pp).max() > 1e-3


def test_system_is_symmetric_and_positive_semidefinite(six):
    H = six.H
    assert np.array_equal(H, H.T) or np.abs(H - H.T).max() <= 1e-12 * np.abs(H).max()
    ev = np.linalg.eigvalsh(0.5 * (H + H.T))
    assert ev.min() >= -1e-6 * np.abs(ev).max()


def _block(H, i1, i2):
    return H[6 * i1:6 * i1 + 6, 6 * i2:6 * i2 + 6]


def test_off_diagonal_blocks_vanish_exactly_where_no_voxel_counts_both(pkg, O):
    """with an unseen keyframe (id 63 on a 6-frame map): a zero row and column, its pose unmoved, the others' steps those of the
    system without it"""
    c7 = _Case(pkg, O, 6, extra_ids=(63,))
    seen = c7.obs["seen"]
    n = len(c7.idx)
    some_zero = False
    for i1 in range(n):
        for i2 in range(n):
            if i1 == i2:
                continue
            shared = bool((seen[:, i1] & seen[:, i2]).any())
            zero = not np.any(_block(c7.H, i1, i2))
            assert zero == (not shared), (i1, i2)
            some_zero = some_zero or zero
    assert some_zero and not seen[:, 6].any()
    assert not np.any(c7.H[36:, :]) and not np.any(c7.H[:, 36:]) and not np.any(c7.b[36:])
    P7, d7 = REF.step(c7.H, c7.b, c7.Pp_all)
    P6, d6 = REF.step(c7.H[:36, :36], c7.b[:36], c7.Pp_all[:6])
    assert np.array_equal(P7[6], c7.Pp_all[6].astype(np.float64)) and not np.any(d7[36:])
    assert np.abs(P7[:6] - P6).max() < 1e-9 and np.abs(d6).max() > 1e-3


def test_one_keyframe_coupled_is_decoupled(pkg, O, six):
    obs = REF.observations(six.keys, six.pay, six.vis, six.seq.K, six.vs, six.imgs[1:2], six.Pp[1:2], [1])
    H, b = REF.system(obs)
    assert H.shape == (6, 6)
    Pc, dc = REF.step(H, b, six.Pp[1:2])
    Pd, dd = REF.decoupled_step(H, b, six.Pp[1:2])
    assert np.array_equal(Pc, Pd) and np.array_equal(dc, dd)
    # a voxel seen by one keyframe has N_j = 1: r = 0 and (1 - inv_Nj) = 0 -- nothing to solve, as in the reference
    assert not np.any(H) and not np.any(b) and np.array_equal(Pc, six.Pp[1:2].astype(np.float64))


def test_one_coupled_step_lowers_the_energy(pkg, O, six):
    E0 = O.PhotoBA(six.o, six.imgs, six.Pp, six.idx).energy_f64()
    Pn, delta = REF.step(six.H, six.b, six.Pp)
    E1 = O.PhotoBA(six.o, six.imgs, Pn.astype(np.float32), six.idx).energy_f64()
    Pd, _ = REF.decoupled_step(six.H, six.b, six.Pp)
    print("energy %.6g -> %.6g (coupled), step %.3e, coupled vs decoupled %.3e" % (E0, E1, np.abs(Pn - six.Pp).max(), np.abs(Pn - Pd).max()))
    assert E1 < E0 and np.abs(Pn - six.Pp).max() > 1e-3
    assert np.abs(Pn - Pd).max() > 1e-5                           # the coupling really acts


def test_trunc_l2_gate_changes_the_system(six):
    obs = REF.observations(six.keys, six.pay, six.vis, six.seq.K, six.vs, six.imgs, six.Pp, six.idx, trunc_lambda=0.5)
    H, b = REF.system(obs)
    assert obs["seen"].sum() < six.obs["seen"].sum()
    assert np.abs(H - six.H).max() > 1e-4 * np.abs(six.H).max()
    big = REF.observations(six.keys, six.pay, six.vis, six.seq.K, six.vs, six.imgs, six.Pp, six.idx, trunc_lambda=2.0)
    assert np.array_equal(REF.system(big)[0], six.H)              # lambda above every intensity: the ungated system


def uncertainty(H, b, poses):
    """u = max |poses(step in float32) - poses(step in float64)| of the restatement: what the reference's own float LDLT leaves
    open (the precedent of serial_vs_omp)"""
    P32, _ = REF.step(H, b, poses, np.float32)
    P64, _ = REF.step(H, b, poses, np.float64)
    return float(np.abs(P32.astype(np.float64) - P64).max())


# the perturbation of the scenes of tests/test_gpu_ba_pose_full.py's step test, as a fraction of _scene's default
GPU_STEP_SCENES = {6: 1.0, 50: 1.0}


# ... and of the 6-keyframe scene of the optimize() series tests (tests/test_gpu_ba_pose_full.py, test_gpu_ba_pose_full_facade.py).
# The energy behind a Gauss-Newton step is not at its minimum, so it answers the step's own rounding in first order: at _scene's
# default perturbation the restatement's energy behind ONE step differs by 4.2e-5 relative between its float32 and its float64
# LDLT -- two fifths of the 1e-4 bar before anything is compared --, at half the perturbation by 5.3e-6.  The series tests
# therefore start from half the perturbation (the rule of the step scenes: the reference's own uncertainty <= a fifth of the bar).
OPTIMIZE_SCENE = 0.5


def test_reference_energy_uncertainty_of_the_optimize_scene(pkg, O):
    c = _Case(pkg, O, 6, scale=OPTIMIZE_SCENE)
    E = []
    for dtype in (np.float32, np.float64):
        Pn, _ = REF.step(c.H, c.b, c.Pp, dtype)
        E.append(O.PhotoBA(c.o, c.imgs, Pn.astype(np.float32), c.idx).energy_f64())
    E0 = O.PhotoBA(c.o, c.imgs, c.Pp, c.idx).energy_f64()
    uE = abs(E[0] / E[1] - 1)
    print("optimize scene: E %.6g -> %.8g; float32 vs float64 step: %.3e relative" % (E0, E[1], uE))
    assert uE <= 2e-5 and E[1] < 0.1 * E0


@pytest.mark.parametrize("n", [6, 50])
def test_reference_uncertainty_of_the_gpu_step_scenes(pkg, O, n, six):
    c = six if n == 6 and GPU_STEP_SCENES[6] == 1.0 else _Case(pkg, O, n, scale=GPU_STEP_SCENES[n])
    u = uncertainty(c.H, c.b, c.Pp)
    print("n = %d: u = max |poses(float32 step) - poses(float64 step)| = %.3e, cond(H) = %.3e" % (n, u, np.linalg.cond(c.H)))
    assert u <= 2e-5                                              # a fifth of the 1e-4 bar


def test_abi_declares_and_exports_the_coupled_step(pkg):
    txt = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = ("gsdf_ba_pose_system", "gsdf_ba_solve_pose_full", "gsdf_ba_set_pose_step")
    for lib in (pkg.binding.load(), pkg.binding.load_test_lib()):
        for name in names:
            assert re.search(r"\bint\s+%s\s*\(" % name, txt), name + " is not declared in include/gsdf.h"
            assert hasattr(lib, name), name + " is not exported"
    assert hasattr(pkg.GradSdf, "ba_pose_system") and hasattr(pkg.GradSdf, "ba_solve_pose_full") and hasattr(pkg.GradSdf, "ba_set_pose_step")
