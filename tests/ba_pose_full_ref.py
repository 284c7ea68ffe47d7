"""The coupled pose step of PhotoBA -- PhotometricOptimizer::solvePoseFull, ps_optimizer/PhotometricOptimizer.cpp:392-496 -- stated
in vectorised numpy over an exported map (keys, payload, vis_), the keyframe images, poses and ids: the reference statement of
tests/test_ba_pose_full.py (not gpu) and the parity target of tests/test_gpu_ba_pose_full.py.  The oracle has no solvePoseFull.

Per observation (voxel j with |dist| <= vs, keyframe i that sees it) everything is float32 in the reference's expression order,
as getEnergy / solvePose have it (tests/test_oracle_second_statement.py::get_energy, csrc/gsdf_ba_shared.h): the projection with
the double 1./z (:165-177), interpolateImage (:57-77), both computeImageGradient directions with their border branches (:80-140),
computeJc (:206-233), the TRUNC_L2 rule (:435), N_j, inv_Nj = (float)(1. / (float)N_j), mean_j and r_ij = A_ij - mean_j.
H and b are then CONTRACTED IN FLOAT64 (the order-free sums of those float32 terms):

    b[6i..6i+5] = sum_j sum_c r_ij[c] J_ij[c, :]                    (:461-462)
    H[i, i]     = sum_j (1 - inv_Nj) J_ij^T J_ij                    (:464-466)
    H[i1, i2]   = sum_j (-inv_Nj) J_i1j^T J_i2j   (i1 != i2)        (:475-479)

step() is Eigen's LDLT (symmetric pivoting on the largest remaining |diagonal|, a zero pivot gives a zero component; :483) plus
the pose update t_i -= delta[6i..6i+2], R_i = R_i SO3::exp(-delta[6i+3..6i+5]) (:491-494; no pose moves if any component is NaN,
:488-490), in float32 or float64."""
import numpy as np

f32 = np.float32


def _sum3(a, b, c):
    return a + (b + c)                                              # float32 arrays: a + (b + c), every operation rounded


def _px(img, r, c):
    H, W = img.shape[:2]
    return img[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)]          # (clipped indices are only ever those of an unselected branch)


def _interp(row, col, img):
    """interpolateImage(m = row, n = col), :57-77: weights mix double and float, every term rounded to float; BGR -> RGB"""
    H, W = img.shape[:2]
    x = np.floor(row).astype(np.int64); y = np.floor(col).astype(np.int64)
    inner = ((x + 1) < H) & ((y + 1) < W)
    mx = (row - x.astype(f32)).astype(f32); ny = (col - y.astype(f32)).astype(f32)
    m64, n64 = row.astype(np.float64), col.astype(np.float64)
    w1 = (y + 1.0 - n64) * mx.astype(np.float64)
    w2 = (y + 1.0 - n64) * (x + 1.0 - m64)
    w3 = (ny * mx).astype(f32).astype(np.float64)                   # float * float: rounded to float, the others are double
    w4 = ny.astype(np.float64) * (x + 1.0 - m64)
    a, b, c, d = _px(img, x + 1, y), _px(img, x, y), _px(img, x + 1, y + 1), _px(img, x, y + 1)

    def term(w, p):
        return (w[:, None] * p.astype(np.float64)).astype(f32)
    t = ((term(w1, a) + term(w2, b)) + term(w3, c)) + term(w4, d)
    t = np.where(inner[:, None], t, b)                              # (behind getIntensity's test the other branches copy the pixel)
    return t[:, ::-1]


def _grad(row, col, img, direction):
    """computeImageGradient(m = row, n = col, direction), :80-140, with its border branches; BGR -> RGB"""
    H, W = img.shape[:2]
    x = np.floor(row).astype(np.int64); y = np.floor(col).astype(np.int64)
    xok = (x + 1) < H; yok = (y + 1) < W
    w01 = (row - x.astype(f32)).astype(f32); w11 = (col - y.astype(f32)).astype(f32)
    w00 = (1.0 - w01.astype(np.float64)).astype(f32); w10 = (1.0 - w11.astype(np.float64)).astype(f32)
    one, zero = np.ones_like(w01), np.zeros_like(w01)
    if direction == 0:
        v0 = np.where(yok[:, None], _px(img, x, y + 1) - _px(img, x, y), _px(img, x, y) - _px(img, x, y - 1))
        v1 = np.where(yok[:, None], _px(img, x + 1, y + 1) - _px(img, x + 1, y), _px(img, x + 1, y) - _px(img, x + 1, y - 1))
        v1 = np.where(xok[:, None], v1, f32(0))
        a = np.where(xok, w00, one); b = np.where(xok, w01, zero)
    else:
        v0 = np.where(xok[:, None], _px(img, x + 1, y) - _px(img, x, y), _px(img, x, y) - _px(img, x - 1, y))
        v1 = np.where(xok[:, None], _px(img, x + 1, y + 1) - _px(img, x, y + 1), _px(img, x, y + 1) - _px(img, x - 1, y + 1))
        v1 = np.where(yok[:, None], v1, f32(0))
        a = np.where(yok, w10, one); b = np.where(yok, w11, zero)
    g = a[:, None] * v0 + b[:, None] * v1
    return g[:, ::-1]


def observations(keys, pay, vis, K, vs, images, poses, frame_idx, trunc_lambda=None):
    """Every (gated voxel, keyframe) pair: seen (V, n) -- the keyframes voxel j counts --, A (V, n, 3), J (V, n, 3, 6), float32;
    `rows` = the indices of the gated voxels in keys.  Unseen pairs hold zeros."""
    keys = np.asarray(keys); pay = np.asarray(pay, f32); images = np.asarray(images, f32)
    K = np.asarray(K, f32).reshape(3, 3); vs = f32(vs)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    n = len(frame_idx)
    Himg, Wimg = images.shape[1:3]
    rows = np.nonzero(~(np.abs(pay[:, 0]) > vs))[0]                 # :406
    dist = pay[rows, 0]; g = pay[rows, 1:4]
    z = _sum3(g[:, 0] * g[:, 0], g[:, 1] * g[:, 1], g[:, 2] * g[:, 2])
    with np.errstate(all="ignore"):
        gn = np.where((z > 0)[:, None], g / np.sqrt(z)[:, None], g)  # Eigen normalized()
    c = vs * keys[rows].astype(f32)
    V = len(rows)
    seen = np.zeros((V, n), bool)
    A = np.zeros((V, n, 3), f32); J = np.zeros((V, n, 3, 6), f32)
    words = vis.shape[1]
    for i, f in enumerate(frame_idx):
        f = int(f)
        if f >= 32 * words:
            continue
        vbit = ((vis[rows, f >> 5] >> np.uint32(f & 31)) & np.uint32(1)).astype(bool)
        R = np.asarray(poses[i], f32)[:3, :3]; t = np.asarray(poses[i], f32)[:3, 3]
        d = (c - dist[:, None] * gn) - t                            # :247
        p = np.stack([_sum3(R[0, j] * d[:, 0], R[1, j] * d[:, 1], R[2, j] * d[:, 2]) for j in range(3)], axis=1)
        with np.errstate(all="ignore"):
            z_inv = (1.0 / p[:, 2].astype(np.float64)).astype(f32)
            m = fx * p[:, 0] * z_inv + cx; nn = fy * p[:, 1] * z_inv + cy
            ok = vbit & ~((m < 0) | (m >= Wimg) | (nn < 0) | (nn >= Himg))
        idx = np.nonzero(ok)[0]
        if not len(idx):
            continue
        pi, zi, mi, ni = p[idx], z_inv[idx], m[idx], nn[idx]
        Ai = _interp(ni, mi, images[i])                             # (n, m): m indexes columns
        if trunc_lambda is not None:                                # TRUNC_L2, :435
            keep = ~(np.max(Ai * Ai, axis=1) > f32(trunc_lambda) * f32(trunc_lambda))
            idx, pi, zi, mi, ni, Ai = idx[keep], pi[keep], zi[keep], mi[keep], ni[keep], Ai[keep]
        g0 = _grad(ni, mi, images[i], 0); g1 = _grad(ni, mi, images[i], 1)
        zz = zi * zi
        zero = np.zeros_like(zi)
        pg0 = np.stack([fx * zi, zero, -fx * pi[:, 0] * zz], axis=1)
        pg1 = np.stack([zero, fy * zi, -fy * pi[:, 1] * zz], axis=1)
        G = g0[:, :, None] * pg0[:, None, :] + g1[:, :, None] * pg1[:, None, :]       # (k, 3 colours, 3)
        S = np.zeros((len(idx), 3, 3), f32)
        S[:, 0, 1] = -pi[:, 2]; S[:, 0, 2] = pi[:, 1]; S[:, 1, 0] = pi[:, 2]
        S[:, 1, 2] = -pi[:, 0]; S[:, 2, 0] = -pi[:, 1]; S[:, 2, 1] = pi[:, 0]
        Ji = np.zeros((len(idx), 3, 6), f32)
        for col in range(3):                                        # computeJc :206-233
            Ji[:, :, col] = -_sum3(G[:, :, 0] * R[col, 0], G[:, :, 1] * R[col, 1], G[:, :, 2] * R[col, 2])
            Ji[:, :, 3 + col] = _sum3(G[:, :, 0] * S[:, None, 0, col], G[:, :, 1] * S[:, None, 1, col], G[:, :, 2] * S[:, None, 2, col])
        seen[idx, i] = True; A[idx, i] = Ai; J[idx, i] = Ji
    return dict(rows=rows, seen=seen, A=A, J=J)


def residuals(obs):
    """N_j, inv_Nj (float32) and r_ij = A_ij - mean_j (float32; zeros where unseen), the mean summed in keyframe order"""
    seen, A = obs["seen"], obs["A"]
    Nj = seen.sum(axis=1)
    with np.errstate(all="ignore"):
        inv = np.where(Nj > 0, (1.0 / Nj.astype(f32).astype(np.float64)).astype(f32), f32(0))
    mean = np.zeros((len(Nj), 3), f32)
    for i in range(seen.shape[1]):
        mean = mean + A[:, i]                                       # (an unseen keyframe adds its zeros: exact)
    mean = inv[:, None] * mean
    r = np.where(seen[:, :, None], A - mean[:, None, :], f32(0))
    return Nj, inv, r


def energy(obs):
    """getEnergy (:273-321) as the double sum of its float terms"""
    _, _, r = residuals(obs)
    return float(_sum3(r[..., 0] * r[..., 0], r[..., 1] * r[..., 1], r[..., 2] * r[..., 2]).astype(np.float64).sum())


def system(obs):
    """H (6n, 6n) and b (6n,) of solvePoseFull, contracted in float64"""
    J = obs["J"]
    V, n = J.shape[:2]
    Nj, inv, r = residuals(obs)
    X = J.transpose(0, 2, 1, 3).reshape(V * 3, 6 * n).astype(np.float64)            # one row per (voxel, colour channel)
    w_off = np.repeat(inv.astype(np.float64), 3)
    w_diag = np.repeat((f32(1) - inv).astype(np.float64), 3)
    H = -(X.T @ (w_off[:, None] * X))
    D = X.T @ (w_diag[:, None] * X)
    for i in range(n):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = D[6 * i:6 * i + 6, 6 * i:6 * i + 6]
    b = np.einsum("vic,vick->ik", r.astype(np.float64), J.astype(np.float64)).reshape(6 * n)
    return H, b


def ldlt_solve(H, b, dtype=np.float64):
    """Eigen LDLT's solve in `dtype`: pivot = the largest remaining |diagonal| (the first of equals); zero pivot -> zero component"""
    A = np.array(H, dtype=dtype)
    N = A.shape[0]
    perm = np.arange(N)
    for k in range(N):
        piv = k + int(np.argmax(np.abs(A.diagonal()[k:])))
        if piv != k:
            A[[k, piv], :] = A[[piv, k], :]
            A[:, [k, piv]] = A[:, [piv, k]]
            perm[[k, piv]] = perm[[piv, k]]
        d = A[k, k]
        if d == 0:
            continue
        l = (A[k + 1:, k] / d).astype(dtype)
        A[k + 1:, k + 1:] -= np.outer(l * d, l).astype(dtype)
        A[k + 1:, k] = l
    bb = np.array(b, dtype=dtype)[perm]
    for i in range(N):
        bb[i] -= A[i, :i] @ bb[:i]
    dg = A.diagonal()
    with np.errstate(all="ignore"):
        bb = np.where(dg != 0, bb / dg, dtype(0)).astype(dtype)
    for i in range(N - 1, -1, -1):
        bb[i] -= A[i + 1:, i] @ bb[i + 1:]
    x = np.empty(N, dtype)
    x[perm] = bb
    return x


def so3_exp(w, dtype):
    w = np.asarray(w, dtype)
    th = dtype(np.sqrt(w @ w))
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype)
    if th < 1e-10:
        return (np.eye(3, dtype=dtype) + Kx).astype(dtype)
    s = dtype(np.sin(th * dtype(0.5)))
    return (np.eye(3, dtype=dtype) + dtype(np.sin(th) / th) * Kx + dtype(2) * s * s / (th * th) * (Kx @ Kx)).astype(dtype)


def apply_delta(poses, delta, dtype=np.float64):
    """:488-494"""
    P = np.array(poses, dtype=dtype)
    delta = np.asarray(delta, dtype)
    if np.isnan(delta).any():
        return P
    for i in range(P.shape[0]):
        P[i, :3, 3] -= delta[6 * i:6 * i + 3]
        P[i, :3, :3] = P[i, :3, :3] @ so3_exp(-delta[6 * i + 3:6 * i + 6], dtype)
    return P


def step(H, b, poses, dtype=np.float64):
    """one solvePoseFull from (H, b): the new poses (n, 4, 4) and delta, in `dtype`"""
    delta = ldlt_solve(np.asarray(H).astype(dtype), np.asarray(b).astype(dtype), dtype)
    return apply_delta(poses, delta, dtype), delta


def decoupled_step(H, b, poses, dtype=np.float64):
    """solvePose (:499-590) from the same sums: every keyframe's own 6 x 6 block with its part of b; a keyframe whose step has a
    NaN stays (:581-583)"""
    P = np.array(poses, dtype=dtype)
    delta = np.zeros(len(b), dtype)
    for i in range(P.shape[0]):
        s = slice(6 * i, 6 * i + 6)
        d = ldlt_solve(np.asarray(H)[s, s].astype(dtype), np.asarray(b)[s].astype(dtype), dtype)
        if np.isnan(d).any():
            continue
        delta[s] = d
        P[i:i + 1] = apply_delta(P[i:i + 1], d, dtype)
    return P, delta
