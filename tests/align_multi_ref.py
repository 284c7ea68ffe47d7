"""numpy restatement of gsdf_align_starts and gsdf_align_best (include/gsdf.h): the grid of starting poses of a multi-start
registration, in double from the float inputs with one rounding per value, and the pick among the runs."""
import numpy as np

f32 = np.float32
MAX_STARTS = 1024               # GSDF_ALIGN_MAX_STARTS


def _quat_R(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def _quat_mul(a, b):
    """Hamilton product a (x) b of quaternions x y z w"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], np.float64)


def starts(center7, pivot, rot_step, rot_k, trans_step, trans_k):
    """[m, 7] float32, m = (2 rot_k + 1)^3 (2 trans_k + 1)^3, index ((((a Rn + b) Rn + c) Tn + d) Tn + e) Tn + f"""
    c = np.asarray(center7, f32).astype(np.float64)
    pv = np.asarray(pivot, f32).astype(np.float64)
    rs, ts = float(f32(rot_step)), float(f32(trans_step))
    qc = c[3:] / np.sqrt((c[3:] * c[3:]).sum())
    Rc = _quat_R(qc)
    Rn, Tn = 2 * rot_k + 1, 2 * trans_k + 1
    out = []
    for a in range(Rn):
        for b in range(Rn):
            for cc in range(Rn):
                r = rs * np.array([a - rot_k, b - rot_k, cc - rot_k], np.float64)
                th = np.sqrt((r * r).sum())
                qd = np.array([0, 0, 0, 1], np.float64)
                if th > 0:
                    qd = np.concatenate([np.sin(0.5 * th) / th * r, [np.cos(0.5 * th)]])
                q = _quat_mul(qc, qd)
                q = q / np.sqrt((q * q).sum())
                if q[3] < 0:
                    q = -q
                base = Rc @ (pv - _quat_R(qd) @ pv)
                for d in range(Tn):
                    for e in range(Tn):
                        for f in range(Tn):
                            o = ts * np.array([d - trans_k, e - trans_k, f - trans_k], np.float64)
                            out.append(np.concatenate([base + c[:3] + o, q]).astype(f32))
    return np.array(out, f32).reshape(-1, 7)


def best(converged, passes, last, min_count, require_converged=True):
    """the eligible run with the smallest (double)E / (double)count, lowest index on ties; -1 if none"""
    pick, score = -1, 0.0
    for h in range(len(passes)):
        E, count = f32(last[h][0]), f32(last[h][28])
        if passes[h] <= 0 or (require_converged and not converged[h]):
            continue
        if not (float(count) >= float(min_count)) or not count > 0 or not np.isfinite(E):
            continue
        s = float(E) / float(count)
        if pick < 0 or s < score:
            pick, score = h, s
    return pick
