"""numpy restatement of gsdf_align_points (include/gsdf.h): RigidPointOptimizer::optimize_sampled's loop
(RigidPointOptimizer.cpp:51-96) over a given point set instead of the back-projected pixels of :62-69.

The per-point map values come from a `query(points) -> (phi, g, w)` callable -- Oracle.query, or the engine's own gsdf_query --
so the restatement is the ARITHMETIC AROUND the query: transform, float32 terms, float64 sums, solve, stop rule.  float32
everywhere the reference computes in float; the sums with dtype=float64 (the engine widens every term to double)."""
import numpy as np

f32 = np.float32
NSUM = 29                       # E, g[6], H upper triangle[21] row-major, count


def _sum3(a, b, c):
    return a + (b + c)          # Eigen's unrolled 3-term redux


def transform(pose7, pts, O):
    """p = R x + t in float32: gsdf_matvec's x0 + (x1 + x2), then + t per component (:70)"""
    pose7 = np.asarray(pose7, f32)
    R = O.quat_to_R(pose7[3:])  # :53
    t = pose7[:3]
    x = np.asarray(pts, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        Rx = np.stack([_sum3(R[i, 0] * x[:, 0], R[i, 1] * x[:, 1], R[i, 2] * x[:, 2]) for i in range(3)], 1).astype(f32)
        return (Rx + t[None, :]).astype(f32)


def backproject(depth, K, zmin=0.5, zmax=3.5):
    """the camera-frame points of :62-69 for the in-range pixels, in the reference's pixel order"""
    d = np.asarray(depth, f32)
    H, W = d.shape
    K = np.asarray(K, f32).reshape(3, 3)
    ys, xs = np.mgrid[0:H, 0:W]
    m = ~((d <= f32(zmin)) | (d >= f32(zmax)))                               # :65
    fxi, fyi = f32(1) / K[0, 0], f32(1) / K[1, 1]                           # :47-48
    x0 = ((xs.astype(f32) - K[0, 2]) * fxi).astype(f32)                     # :67
    y0 = ((ys.astype(f32) - K[1, 2]) * fyi).astype(f32)                     # :68
    return np.stack([(x0 * d).astype(f32)[m], (y0 * d).astype(f32)[m], d[m]], 1)


def pass_sums(pts, pose7, query, O):
    """One pass.  Returns (S float64[29] unrounded, A float64[29] = sums of the terms' magnitudes, tot float32[29] = S rounded once)."""
    p = transform(pose7, pts, O)
    p = p[np.isfinite(p).all(axis=1)]                                       # skipped before any float -> int conversion
    S = np.zeros(NSUM, np.float64)
    A = np.zeros(NSUM, np.float64)
    if len(p):
        phi, g, w = query(p)
        m = w > 0                                                           # :73
        p, phi, g = p[m], np.asarray(phi, f32)[m], np.asarray(g, f32)[m]
        c = np.stack([p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1], p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2],
                      p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0]], 1).astype(f32)   # gsdf_cross3(p, g), :78
        J = np.concatenate([g, c], 1).astype(f32)
        terms = [(phi * phi).astype(f32)]                                   # :76
        terms += [(phi * J[:, i]).astype(f32) for i in range(6)]            # :79
        terms += [(J[:, i] * J[:, j]).astype(f32) for i in range(6) for j in range(i, 6)]   # :80
        for v, term in enumerate(terms):
            S[v] = term.sum(dtype=np.float64)
            A[v] = np.abs(term).sum(dtype=np.float64)
        S[28] = A[28] = float(len(p))                                       # :81
    return S, A, S.astype(f32)


def head(tot, damping, O):
    """xi = damping * H.llt().solve(g) (:86) and |xi|^2 = (x0 + (x1 + x2)) + (x3 + (x4 + x5))"""
    tot = np.asarray(tot, f32)
    Hm = np.zeros((6, 6), f32)
    q = 7
    for i in range(6):
        for j in range(i, 6):
            Hm[i, j] = Hm[j, i] = tot[q]
            q += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        xi = (f32(damping) * O.llt_solve6(Hm, tot[1:7])).astype(f32)
        sq = (xi * xi).astype(f32)
        x2 = f32(_sum3(sq[0], sq[1], sq[2]) + _sum3(sq[3], sq[4], sq[5]))
    return xi, x2


def step(pts, pose7, query, O, damping=1.0):
    """One pass and its head WITHOUT the stop test: (S, A, trace row float32[36], pose after applying -xi unless NaN)"""
    S, A, tot = pass_sums(pts, pose7, query, O)
    xi, x2 = head(tot, damping, O)
    row = np.concatenate([tot, xi, [x2]]).astype(f32)
    pose = np.asarray(pose7, f32).copy()
    if not np.isnan(xi).any():                                              # :94-95
        pose = O.se3_exp_mul(-xi, pose)
    return S, A, row, pose


def align(pts, pose7, query, O, iters=25, conv=1e-3, damping=1.0):
    """The loop with the stop rule: (converged, pose7, passes, trace float32[passes, 36])"""
    pose = np.asarray(pose7, f32).copy()
    conv_sq = f32(conv) * f32(conv)
    trace = []
    for _ in range(int(iters)):
        _, _, row, nxt = step(pts, pose, query, O, damping)
        trace.append(row)
        if row[35] < conv_sq:                                               # :88-91: xi is not applied
            return True, pose, len(trace), np.array(trace, f32).reshape(-1, 36)
        pose = nxt
    return False, pose, int(iters), np.array(trace, f32).reshape(-1, 36)


def displace(cloud_xyz, rot_deg=1.0, axis=(0.3, -0.5, 0.8), tr=(0.01, -0.008, 0.006)):
    """A cloud in the map's frame moved into a source frame: src = Rd^T (x - td), so the pose that brings it back is (Rd, td).
    Returns (src float32[n, 3], Rd float64[3, 3], td float64[3])."""
    ax = np.asarray(axis, np.float64)
    ax = ax / np.linalg.norm(ax)
    th = np.deg2rad(rot_deg)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    Rd = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    td = np.asarray(tr, np.float64)
    return ((np.asarray(cloud_xyz, np.float64) - td) @ Rd).astype(f32), Rd, td


def pose_error(pose7, Rd, td, O):
    """(rotation error in degrees, largest translation error) of a pose against (Rd, td)"""
    Rg = O.quat_to_R(np.asarray(pose7, f32)[3:]).astype(np.float64)
    ang = np.rad2deg(np.arccos(np.clip((np.trace(Rg.T @ Rd) - 1) / 2, -1, 1)))
    return float(ang), float(np.abs(np.asarray(pose7, np.float64)[:3] - td).max())


IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], f32)
