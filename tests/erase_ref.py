"""numpy restatement of the selection predicates, the four ops, invert and erase of include/gsdf.h ("REMOVING VOXELS").

It works from a map's export(sorted=True, raw=True) -- keys [n, 3] int32 and raw sums [n, 5] = s, gx, gy, gz, w -- and evaluates
each predicate for EVERY voxel of the map by brute force (all voxels x all points in chunks): no blocks, no enumeration, no hash.
float32 wherever the kernels compute in float; a selection is a boolean mask over the rows of the export."""
import numpy as np

import align_points_ref as apr

f32 = np.float32
REPLACE, ADD, INTERSECT, SUBTRACT = 0, 1, 2, 3


def centres(keys, vs):
    """c = (vs * (float)i, vs * (float)j, vs * (float)k): one float product per component"""
    return (f32(vs) * np.asarray(keys).astype(f32)).astype(f32)


def box(keys, vs, lo, hi):
    """lo[a] <= c[a] && c[a] <= hi[a] on all three axes (closed; lo > hi is empty; infinities allowed)"""
    c = centres(keys, vs).reshape(-1, 3)
    lo, hi = np.asarray(lo, f32).reshape(3), np.asarray(hi, f32).reshape(3)
    return ((lo[None, :] <= c) & (c <= hi[None, :])).all(axis=1)


def weight(pay, w_min, w_max):
    """w_min <= w && w < w_max on the stored weight sum (half-open)"""
    w = np.asarray(pay, f32).reshape(-1, 5)[:, 4]
    return (f32(w_min) <= w) & (w < f32(w_max))


def moved(pts, pose7, O):
    """the points as the kernel sees them: p = x, or R x + t as the registration forms it; non-finite ones dropped"""
    p = np.asarray(pts, f32).reshape(-1, 3)
    if pose7 is not None:
        p = apr.transform(pose7, p, O)
    return p[np.isfinite(p).all(axis=1)]


def points(keys, vs, pts, radius, pose7=None, O=None, chunk=1 << 22):
    """member iff for some point dx*dx + (dy*dy + dz*dz) <= radius*radius, d = c - p per component, all float32"""
    c = centres(keys, vs).reshape(-1, 3)
    p = moved(pts, pose7, O)
    r2 = f32(f32(radius) * f32(radius))
    out = np.zeros(len(c), bool)
    if len(c) == 0 or len(p) == 0:
        return out
    step = max(1, chunk // len(c))
    for a in range(0, len(p), step):
        q = p[a:a + step]
        with np.errstate(over="ignore"):                       # a point far away: inf, which is not <= r2
            d = (c[:, None, :] - q[None, :, :]).astype(f32)
            sq = (d * d).astype(f32)
            s = (sq[:, :, 0] + (sq[:, :, 1] + sq[:, :, 2]).astype(f32)).astype(f32)
        out |= (s <= r2).any(axis=1)
    return out


def combine(op, S, P):
    """S := P, S | P, S & P, S & ~P; S None (no selection) counts as the empty set"""
    P = np.asarray(P, bool)
    S = np.zeros_like(P) if S is None else np.asarray(S, bool)
    return {REPLACE: P, ADD: S | P, INTERSECT: S & P, SUBTRACT: S & ~P}[op]


def invert(S, n):
    """the complement over the map (S None: everything)"""
    return np.ones(n, bool) if S is None else ~np.asarray(S, bool)


def pack(keys):
    """one int64 per key, ordered like (z, y, x)"""
    k = np.asarray(keys, np.int64).reshape(-1, 3) + (1 << 20)
    return k[:, 0] | (k[:, 1] << 21) | (k[:, 2] << 42)


def blocks(keys):
    """the distinct 4x4x4 blocks of the keys, packed"""
    return np.unique(pack(np.asarray(keys, np.int64).reshape(-1, 3) >> 2))


def erase(keys, pay, S):
    """(keys, payload) of the map without the members, voxels erased, blocks that lost a voxel and hold none afterwards"""
    keys, pay, S = np.asarray(keys), np.asarray(pay), np.asarray(S, bool)
    emptied = np.setdiff1d(blocks(keys[S]), blocks(keys[~S]))
    return keys[~S], pay[~S], int(S.sum()), len(emptied)
