"""numpy restatement of gsdf_merge_from_posed (include/gsdf.h), steps 1-7, by brute force over an integer box of dst keys.

The map values come from two callables of the SOURCE map -- `query(points) -> (phi, g, w)` (gsdf_query) and
`get_voxels(keys) -> (payload [n, 5] = dist, raw gx gy gz, weight; found)` (gsdf_get_voxels) -- so the restatement is the
arithmetic around the engine's own, already tested, readers: vox2float, c - t, R^T d, the finite test, float2vox, the clamp, the
product, the rotated gradient sum, the addition.  It knows nothing of blocks or of the kernel's enumeration: every key of the box
is evaluated.  float32 everywhere, x0 + (x1 + x2) for every 3-term sum."""
import numpy as np

f32 = np.float32
KEY_OFF = 1 << 20
CHUNK = 1 << 21


def _sum3(a, b, c):
    return a + (b + c)


def matvec(M, v):
    """gsdf_matvec: row i = M[i, 0] v0 + (M[i, 1] v1 + M[i, 2] v2), float32"""
    M = np.asarray(M, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([_sum3(M[i, 0] * v[:, 0], M[i, 1] * v[:, 1], M[i, 2] * v[:, 2]) for i in range(3)], 1).astype(f32)


def float2vox(q, vs):
    """gsdf_float2vox1 per component: (int) truncf(x + copysignf(0.49999997f, x)), x = inv_vs * q, inv_vs = (float)(1. / vs)"""
    inv_vs = f32(1.0 / np.float64(f32(vs)))
    x = (inv_vs * np.asarray(q, f32)).astype(f32)
    r = np.trunc((x + np.copysign(f32(0.49999997), x)).astype(f32))
    return np.clip(r, -2.0 ** 30, 2.0 ** 30).astype(np.int32)        # beyond the key range either way: such a voxel has w == 0


def truncate(phi, T):
    """Sdf::truncate = fmaxf(-T, fminf(T, phi))"""
    return np.fmax(-f32(T), np.fmin(f32(T), np.asarray(phi, f32))).astype(f32)


def in_range(keys):
    k = np.asarray(keys)
    return ((k >= -KEY_OFF) & (k < KEY_OFF)).all(axis=1)


def box_of(src_keys, pose7, vs, O, pad=2):
    """The bounding box (lo[3], hi[3], inclusive voxel indices) of T(c_V) = R c_V + t over src's voxels, widened by `pad` voxels
    per axis.  float64; R is the float32 matrix the kernel uses."""
    pose7 = np.asarray(pose7, f32)
    R = O.quat_to_R(pose7[3:]).astype(np.float64)
    p = np.asarray(src_keys, np.float64) @ R.T + pose7[:3].astype(np.float64) / np.float64(f32(vs))
    return np.floor(p.min(axis=0)).astype(np.int64) - pad, np.ceil(p.max(axis=0)).astype(np.int64) + pad


def box_size(box):
    lo, hi = box
    return int(np.prod(hi - lo + 1))


def contributions(query, get_voxels, pose7, vs, T, box, O):
    """Steps 1-6 for ALL keys of the box that lie inside the packable range.
    Returns (keys int32 [n, 3] in (z, y, x) order, contrib float32 [n, 5] = s', gx', gy', gz', w' -- gsdf_export's raw layout)."""
    pose7 = np.asarray(pose7, f32)
    vs = f32(vs)
    R = O.quat_to_R(pose7[3:])                                       # no renormalisation
    t = pose7[:3]
    lo, hi = box
    lo = np.maximum(lo, -KEY_OFF)
    hi = np.minimum(hi, KEY_OFF - 1)
    nx, ny, nz = (int(max(h - l + 1, 0)) for l, h in zip(lo, hi))
    total = nx * ny * nz
    out_k, out_c = [], []
    for a in range(0, total, CHUNK):
        idx = np.arange(a, min(a + CHUNK, total), dtype=np.int64)   # x fastest, then y, then z: the (z, y, x) key order
        K = np.stack([lo[0] + idx % nx, lo[1] + (idx // nx) % ny, lo[2] + idx // (nx * ny)], 1).astype(np.int32)
        with np.errstate(invalid="ignore", over="ignore"):
            c = (vs * K.astype(f32)).astype(f32)                     # 1
            d = (c - t[None, :]).astype(f32)                         # 2
            q = matvec(R.T, d)                                       # 3
        fin = np.isfinite(q).all(axis=1)                             # 4
        K, q = K[fin], q[fin]
        if not len(K):
            continue
        phi, _, w = query(q)                                         # 5
        m = np.asarray(w, f32) != 0
        K, q, phi = K[m], q[m], np.asarray(phi, f32)[m]
        if not len(K):
            continue
        pay, found = get_voxels(float2vox(q, vs))                    # 6
        assert np.asarray(found).all(), "a voxel gsdf_query saw is missing for gsdf_get_voxels"
        Sw = np.asarray(pay, f32)[:, 4]
        g = matvec(R, np.asarray(pay, f32)[:, 1:4])
        s = (Sw * truncate(phi, T)).astype(f32)
        out_k.append(K)
        out_c.append(np.concatenate([s[:, None], g, Sw[:, None]], 1).astype(f32))
    if not out_k:
        return np.zeros((0, 3), np.int32), np.zeros((0, 5), f32)
    return np.concatenate(out_k), np.concatenate(out_c)


def pack(keys):
    k = np.asarray(keys, np.int64) + KEY_OFF
    return k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def n_blocks(keys):
    """dst blocks (4^3 voxels, floor division) that hold the keys"""
    return len(np.unique(pack(np.asarray(keys, np.int64) >> 2 << 2))) if len(keys) else 0


def expected(dst_export, query, get_voxels, pose7, vs, T, box, O):
    """Step 7: dst's raw export (keys int32 [n, 3] sorted (z, y, x), payload float32 [n, 5] = s gx gy gz w) after the merge.
    Returns (keys, payload, contribution keys, contributions)."""
    dk, dp = dst_export
    ck, cc = contributions(query, get_voxels, pose7, vs, T, box, O)
    pk_d, pk_c = pack(np.asarray(dk).reshape(-1, 3)), pack(ck)
    allk = np.union1d(pk_d, pk_c)
    pay = np.zeros((len(allk), 5), f32)
    pay[np.searchsorted(allk, pk_d)] = np.asarray(dp, f32).reshape(-1, 5)
    at = np.searchsorted(allk, pk_c)
    pay[at] = (pay[at] + cc).astype(f32)                             # one float addition per field (a key receives once)
    keys = np.stack([(allk & 0x1FFFFF) - KEY_OFF, ((allk >> 21) & 0x1FFFFF) - KEY_OFF, ((allk >> 42) & 0x1FFFFF) - KEY_OFF], 1).astype(np.int32)
    return keys, pay, ck, cc
