"""numpy restatement of gsdf_align_points_robust (include/gsdf.h): tests/align_points_ref.py's pass, step and loop with the
weight a robust loss gives each point's distance (csrc/gsdf_align_loss.h), in float32 with one rounding per operation.

The `query(points) -> (phi, g, w)` convention is align_points_ref's.  A pass has 31 sums: the 29 of the plain pass with the
weighted terms, then the weight sum and the number of points of weight > 0; a trace row has 38 floats: [0..35] as the plain
row, [36] = the weight sum, [37] = the inlier count."""
import numpy as np

import align_points_ref as ref

f32 = np.float32
NSUM = 31
L2, CAUCHY, HUBER, TUKEY, TRUNC_L2 = 0, 1, 2, 3, 4                          # ps_optimizer/loss.h:41-48
IDENTITY = ref.IDENTITY


def weight(loss, scale, phi):
    """the table of include/gsdf.h, every step a float32 operation"""
    phi = np.asarray(phi, f32)
    k = f32(scale)
    one, zero = np.ones_like(phi), np.zeros_like(phi)
    if loss == L2:
        return one
    with np.errstate(all="ignore"):
        a = np.abs(phi)
        r = (phi / k).astype(f32)
        rr = (r * r).astype(f32)
        if loss == CAUCHY:
            return (f32(1) / (f32(1) + rr).astype(f32)).astype(f32)
        if loss == HUBER:
            return np.where(a <= k, one, (k / a).astype(f32)).astype(f32)
        if loss == TUKEY:
            u = (f32(1) - rr).astype(f32)
            return np.where(a < k, (u * u).astype(f32), zero).astype(f32)
        if loss == TRUNC_L2:
            return np.where(a < k, one, zero).astype(f32)
    raise ValueError("loss outside 0..4")


def pass_sums(pts, pose7, query, O, loss=L2, scale=1.0):
    """One pass: (S float64[31] unrounded, A float64[31] = sums of the terms' magnitudes, tot float32[31] = S rounded once)"""
    p = ref.transform(pose7, pts, O)
    p = p[np.isfinite(p).all(axis=1)]
    S = np.zeros(NSUM, np.float64)
    A = np.zeros(NSUM, np.float64)
    if len(p):
        phi, g, w = query(p)
        m = w > 0
        p, phi, g = p[m], np.asarray(phi, f32)[m], np.asarray(g, f32)[m]
        c = np.stack([p[:, 1] * g[:, 2] - p[:, 2] * g[:, 1], p[:, 2] * g[:, 0] - p[:, 0] * g[:, 2],
                      p[:, 0] * g[:, 1] - p[:, 1] * g[:, 0]], 1).astype(f32)
        J = np.concatenate([g, c], 1).astype(f32)
        rw = weight(loss, scale, phi)
        wphi = (rw * phi).astype(f32)
        wJ = (rw[:, None] * J).astype(f32)
        terms = [(wphi * phi).astype(f32)]
        terms += [(wphi * J[:, i]).astype(f32) for i in range(6)]
        terms += [(wJ[:, i] * J[:, j]).astype(f32) for i in range(6) for j in range(i, 6)]
        for v, term in enumerate(terms):
            S[v] = term.sum(dtype=np.float64)
            A[v] = np.abs(term).sum(dtype=np.float64)
        S[28] = A[28] = float(len(p))
        S[29] = rw.sum(dtype=np.float64)
        A[29] = np.abs(rw).sum(dtype=np.float64)
        S[30] = A[30] = float((rw > 0).sum())
    return S, A, S.astype(f32)


def step(pts, pose7, query, O, loss=L2, scale=1.0, damping=1.0):
    """One pass and its head WITHOUT the stop test: (S, A, trace row float32[38], pose after applying -xi unless NaN)"""
    S, A, tot = pass_sums(pts, pose7, query, O, loss, scale)
    xi, x2 = ref.head(tot[:29], damping, O)
    row = np.concatenate([tot[:29], xi, [x2], tot[29:]]).astype(f32)
    pose = np.asarray(pose7, f32).copy()
    if not np.isnan(xi).any():
        pose = O.se3_exp_mul(-xi, pose)
    return S, A, row, pose


def align(pts, pose7, query, O, loss=L2, scale=1.0, iters=25, conv=1e-3, damping=1.0):
    """The loop with the stop rule: (converged, pose7, passes, trace float32[passes, 38])"""
    pose = np.asarray(pose7, f32).copy()
    conv_sq = f32(conv) * f32(conv)
    trace = []
    for _ in range(int(iters)):
        _, _, row, nxt = step(pts, pose, query, O, loss, scale, damping)
        trace.append(row)
        if row[35] < conv_sq:
            return True, pose, len(trace), np.array(trace, f32).reshape(-1, 38)
        pose = nxt
    return False, pose, int(iters), np.array(trace, f32).reshape(-1, 38)


def best(converged, passes, last, min_wsum, require_converged=True):
    """gsdf_align_best_robust: the eligible run with the smallest (double)E / (double)wsum, lowest index on ties; -1 if none"""
    pick, score = -1, 0.0
    for h in range(len(passes)):
        E, wsum = f32(last[h][0]), f32(last[h][36])
        if passes[h] <= 0 or (require_converged and not converged[h]):
            continue
        if not (wsum >= f32(min_wsum)) or not wsum > 0 or not np.isfinite(E):
            continue
        s = float(E) / float(wsum)
        if pick < 0 or s < score:
            pick, score = h, s
    return pick
