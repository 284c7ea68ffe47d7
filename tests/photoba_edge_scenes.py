"""The scenes of tests/test_photoba_edges.py (not gpu: the premises) and tests/test_gpu_photoba_edges.py (gpu): PhotoBA's decoupled
sweeps -- k_ba_energy, k_ba_pose, k_ba_pose_reduce, k_ba_dist -- at the keyframe sets, keyframe counts and image borders that the
160x120 / arange(n) scenes of tests/test_photoba.py never reach.  A plain helper module (no fixtures, no conftest).

Every scene is test_photoba._scene's: the noise-free "tum" stream, 2 cm voxels, trunc 5, seed 0, the default perturbation -- at
33x21 pixels: odd in both directions, narrower than a fusion tile row, and with 3-5 % of the gated observations in the last row
or column (tests/test_photoba_edges.py measures it), so that interpolateImage's and computeImageGradient's border branches carry
weight in every sum.  The stream does not depend on its length and _scene draws the perturbation frame by frame, so the n-frame
scene is the first n frames of the 64-frame one: it is rendered once.

A case = (frames fused, keyframe ids in this order).  Keyframe i takes image and start pose of frame ids[i]; an id that names no
rendered frame (`unseen`: 50 of 40 fused, 64 = the first bit beyond enable_vis(64)) takes those of frame ids[i] % frames -- its
pose must stay whatever they are."""
import numpy as np

import ba_pose_full_ref as REF
from test_photoba import _oracle_map, _scene

f32 = np.float32
W, H = 33, 21
N_MAX = 64
CAPACITY_LOG2 = 18                                                  # n64: 115 340 voxels, 0.44 of 2^18 slots

CASES = {
    "n1": (1, [0]), "n2": (2, [0, 1]), "n3": (3, [0, 1, 2]), "n5": (5, list(range(5))),      # empty and ragged slices of k_ba_pose
    "n6": (6, list(range(6))),                                      # the border case
    "n33": (33, list(range(33))), "n64": (64, list(range(64))),      # one past a word of `seen`; the limit
    "subset": (40, [37, 2, 33, 31, 32, 5]),                          # unsorted, both words of vis_, the word boundary
    "unseen50": (40, [1, 50, 7]),                                    # an id that was never fused
    "unseen64": (40, [1, 64, 7]),                                    # an id beyond the 64 enabled bits
    "twice": (40, [3, 3]),                                           # a duplicated id: r = 0 exactly, b = 0, nothing moves, E = 0
}
# The two optimize() comparisons on `subset`: name -> (loss, lambda, perturbation as a multiple of _scene's).  Every stop decision
# of the oracle's run has to keep 3 x 3e-3 of margin (tests/test_photoba_edges.py::test_stop_rule_margin_of_the_optimize_runs).
# With TRUNC_L2(0.5) the default perturbation does (2.1 % and 1.3 % in two iterations).  With the default loss it does not: the
# first iteration ends at |E_pose - E| / E_pose = 8.9e-3, 8.4e-3 from the 5e-4 threshold, and every max_it >= 1 makes that
# decision -- so that run starts from 1.5 x the perturbation (28 % and 14 %): another input, the same rule.
OPTIMIZE_MAX_IT = 2
OPTIMIZE_RUNS = {"default": (None, 0.5, 1.5), "trunc_l2": (4, 0.5, 1.0)}
TABLE = [c for c in CASES if c != "n6"]                            # the cases of the per-case GPU test; n6 is the border test's

_made = {}


def stream(pkg, O):
    """(seq, vs, T, frames, imgs, P, Pp) of the 64-frame 33x21 scene, made once per process; treat as read-only"""
    if "stream" not in _made:
        _made["stream"] = _scene(pkg, O, W=W, H=H, n=N_MAX, vs=0.02, perturb=True, trunc=5)
    return _made["stream"]


class Scene:
    """one case: what was fused, and the keyframe set handed to PhotoBA"""

    def __init__(self, pkg, O, name, n_fused=None):
        seq, self.vs, self.T, frames, imgs, P, Pp = stream(pkg, O)
        self.name, self.seq = name, seq
        self.n_frames, ids = CASES[name]
        self.n_fused = self.n_frames if n_fused is None else n_fused
        self.frames = frames[:self.n_fused]
        self.idx = np.asarray(ids, np.int32)
        self.n = len(ids)
        src = self.idx % self.n_frames
        self.imgs = np.ascontiguousarray(imgs[src])
        self.P = np.ascontiguousarray(P[src])
        self.Pp = np.ascontiguousarray(Pp[src])

    def perturbed(self, scale):
        """the start poses at `scale` x the perturbation (entries interpolated like tests/test_gpu_ba_pose_full.py's scenes)"""
        return self.Pp if scale == 1.0 else (self.P + f32(scale) * (self.Pp - self.P)).astype(f32)

    def oracle_map(self, O):
        """a freshly fused oracle map (vis_ included)"""
        return _oracle_map(O, self.seq, self.vs, self.T, self.frames)

    def gpu(self, pkg, frames=None, capacity_log2=CAPACITY_LOG2):
        g = pkg.GradSdf(self.vs, self.T, W, H, self.seq.K, capacity_log2=capacity_log2)
        g.enable_vis(64)
        for d, R, t in (self.frames if frames is None else frames):
            g.update(d, R, t)
        return g


def scene(pkg, O, name, n_fused=None):
    key = ("scene", name, n_fused)
    if key not in _made:
        _made[key] = Scene(pkg, O, name, n_fused)
    return _made[key]


def oracle_on(O, sc, keys, pay):
    """the case's oracle map -- fused once per (frames fused), shared -- holding the voxel values `pay`: every user sets the
    payload first, so what an earlier solve_dist left behind never shows"""
    key = ("oracle", sc.n_fused)
    if key not in _made:
        _made[key] = sc.oracle_map(O)
    o = _made[key]
    assert o.set_payload(keys, pay) == 0 and o.count() == len(keys)    # identical key sets
    return o


def border_altered(imgs, delta=0.05):
    """the same images with only the last row and the last column changed: what differs between the two sets passes through
    the border branches of interpolateImage / computeImageGradient and nowhere else"""
    out = np.array(imgs, f32, copy=True)
    out[:, -1, :, :] += f32(delta)
    out[:, :-1, -1, :] += f32(delta)
    return out


def projections(keys, pay, vis, K, vs, poses, frame_idx, gate=True):
    """REF.observations' projection alone (its float32 expression order, :165-177), also without the |dist| <= vs gate (solveDist
    has none): rows, and per (voxel, keyframe) the vis_ bit, column m, row n and `ok` = bit set and inside the image.
    tests/test_photoba_edges.py ties it to REF.observations: on the gated rows `ok` is its `seen`, bit for bit."""
    keys = np.asarray(keys); pay = np.asarray(pay, f32)
    K = np.asarray(K, f32).reshape(3, 3); vs = f32(vs)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    rows = np.nonzero(~(np.abs(pay[:, 0]) > vs))[0] if gate else np.arange(len(pay))
    dist = pay[rows, 0]; g = pay[rows, 1:4]
    z = REF._sum3(g[:, 0] * g[:, 0], g[:, 1] * g[:, 1], g[:, 2] * g[:, 2])
    with np.errstate(all="ignore"):
        gn = np.where((z > 0)[:, None], g / np.sqrt(z)[:, None], g)
    c = vs * keys[rows].astype(f32)
    n = len(frame_idx)
    bit = np.zeros((len(rows), n), bool); ok = np.zeros((len(rows), n), bool)
    m = np.zeros((len(rows), n), f32); nn = np.zeros((len(rows), n), f32)
    for i, f in enumerate(frame_idx):
        f = int(f)
        if f >= 32 * vis.shape[1]:
            continue
        bit[:, i] = ((vis[rows, f >> 5] >> np.uint32(f & 31)) & np.uint32(1)).astype(bool)
        R = np.asarray(poses[i], f32)[:3, :3]; t = np.asarray(poses[i], f32)[:3, 3]
        d = (c - dist[:, None] * gn) - t
        p = np.stack([REF._sum3(R[0, j] * d[:, 0], R[1, j] * d[:, 1], R[2, j] * d[:, 2]) for j in range(3)], axis=1)
        with np.errstate(all="ignore"):
            z_inv = (1.0 / p[:, 2].astype(np.float64)).astype(f32)
            m[:, i] = fx * p[:, 0] * z_inv + cx; nn[:, i] = fy * p[:, 1] * z_inv + cy
            ok[:, i] = bit[:, i] & ~((m[:, i] < 0) | (m[:, i] >= W) | (nn[:, i] < 0) | (nn[:, i] >= H))
    return dict(rows=rows, bit=bit, m=m, n=nn, ok=ok)


def border_share(pr):
    """the share of the observations that leave ba_sample3's fast path: floor(m) + 1 >= W or floor(n) + 1 >= H"""
    ok = pr["ok"]
    with np.errstate(all="ignore"):
        at = ok & ((np.floor(pr["m"]) + 1 >= W) | (np.floor(pr["n"]) + 1 >= H))
    return int(at.sum()), int(ok.sum())


def edge_decisions(pr):
    """the (voxel, keyframe) pairs with the vis_ bit set whose inside / outside decision two correct float32 evaluations could
    make differently: column m within 4 ulp of 0 or W, or row n within 4 ulp of 0 or H.  m = fx x / z + cx is a sum of two
    terms of the size of the image, so its rounding error is a few ulp AT THAT SIZE wherever m lies -- next to 0 as well: the
    ulp is that of W (the larger of the two spacings, for rows too).  This count is the only allowance of the counter
    comparisons."""
    tol = 4 * np.spacing(f32(W))
    m, n = pr["m"].astype(np.float64), pr["n"].astype(np.float64)
    with np.errstate(all="ignore"):
        near = (np.abs(m) <= tol) | (np.abs(m - W) <= tol) | (np.abs(n) <= tol) | (np.abs(n - H) <= tol)
    return int((pr["bit"] & near).sum())


def stop_rule_margins(energies):
    """optimize()'s decisions (:646-655) from its energy series E0, (E_pose, E) per iteration: the smaller of the relative
    changes of E that would flip `|E_pose - E| / E_pose < 5e-4` or `E_pose < E`, per iteration"""
    e = np.asarray(energies, np.float64)
    out = []
    for k in range((len(e) - 1) // 2):
        Ep, E = e[1 + 2 * k], e[2 + 2 * k]
        rel = abs(Ep - E) / Ep
        out.append(min(abs(rel - 5e-4), rel))
    return out
