"""host/PhotometricOptimizer.h: solvePoseFull and optimize() with OptSettings::pose_step = POSE_STEP_FULL, EXECUTED from C++
(host/photoba_full_selftest) against the same steps driven through the C-ABI from here -- both sides are the GPU engine."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_ba_pose_full import OPTIMIZE_SCENE
from test_photoba import _scene


@pytest.mark.gpu
def test_photometric_optimizer_solve_pose_full_facade_executed(pkg, O, tmp_path):
    host = os.path.join(ROOT, "gradient-sdf_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    n, W, H, vsf, trunc = 6, 160, 120, 0.02, 5
    seq, vs, T, frames, imgs, P, Pp = _scene(pkg, O, W=W, H=H, n=n, vs=vsf, trunc=trunc)
    Pp = (P + np.float32(OPTIMIZE_SCENE) * (Pp - P)).astype(np.float32)          # (tests/test_ba_pose_full.py: OPTIMIZE_SCENE)
    d = tmp_path
    np.asarray(seq.K, np.float32).reshape(9).tofile(d / "K.bin")
    np.stack([f[0] for f in frames]).astype(np.float32).tofile(d / "depth.bin")
    imgs.astype(np.float32).tofile(d / "images.bin")
    P.astype(np.float32).tofile(d / "poses_true.bin")
    Pp.astype(np.float32).tofile(d / "poses_start.bin")
    out = subprocess.run([os.path.join(host, "photoba_full_selftest"), str(d), str(W), str(H), str(n), repr(vsf), str(trunc)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "photoba_full_selftest: OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    lines = {}
    for ln in out.stdout.splitlines():
        k, _, rest = ln.partition(" ")
        lines.setdefault(k, []).append(rest.split())
    g = pkg.GradSdf(vs, T, W, H, seq.K, capacity_log2=20)
    g.enable_vis(64)
    for (dep, R, t), Pi in zip(frames, P):
        Rq = O.quat_to_R(O.R_to_quat(Pi[:3, :3].astype(np.float32)))          # SE3(Matrix4f).rotationMatrix(), as the facade fuses
        g.update(dep, Rq, Pi[:3, 3].astype(np.float32))
    assert int(lines["voxels"][0][0]) == g.count() and int(lines["voxels"][0][2]) == n
    idx = np.arange(n)
    g.ba_setup(imgs, Pp, idx)
    e0 = g.ba_energy()
    g.ba_solve_pose_full()
    e1 = g.ba_energy()
    p1 = g.ba_poses()
    g.ba_solve_dist()
    e2 = g.ba_energy()
    got = [float(v) for v in lines["steps"][0]]
    assert got == pytest.approx([e0, e1, e2], rel=1e-4) and e1 < 0.5 * e0       # (two tables: sums in two slot orders)
    pf = np.array([[float(v) for v in row[1:]] for row in lines["pose_after_step"]]).reshape(n, 4, 4)
    # two float32 solves of systems that differ in summation order: within the step's uncertainty u (tests/test_ba_pose_full.py)
    assert np.abs(pf - p1).max() < 2e-5 and np.abs(pf - Pp).max() > 1e-3       # solvePoseFull() moved the poses, download() brought them back
    g.ba_set_pose_step(1)
    conv, en = g.ba_optimize(3)
    row = lines["optimize"][0]
    assert int(row[0]) == int(conv) and [float(v) for v in row[1:]] == pytest.approx(list(en), rel=1e-4)
    pe = np.array([[float(v) for v in r[1:]] for r in lines["pose_final"]]).reshape(n, 4, 4)
    assert np.abs(pe - g.ba_poses()).max() < 1e-4
    g.close()
