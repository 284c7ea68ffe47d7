"""numpy float32 restatement of ColorUpsampler (ps_optimizer/ColorUpsampler.h/.cpp) with SdfVoxelHr (sdf_voxel/SdfVoxel.h:61-112)
over an exported map: the known answers of the CPU tests and the parity target of the GPU colour pass (gsdf_color_compute /
_export / _cloud).  Every float operation is a float32 operation in the reference's order (the tie-break rules are written at each
step); interpolateImage keeps its double weights, as PhotoBA's restatement (csrc/gsdf_interp.h) does.

Inputs: keys (n, 3) int32 and payload (n, 5) float32 [dist, gx, gy, gz, w] as gsdf_export(sorted=1) gives them, vis words
(n, vw) uint32 as gsdf_export_vis gives them, images (k, H, W, 3) float32 BGR, poses (k, 4, 4) float32, frame_idx (k,) int, the
intrinsics K (3, 3) and the voxel size."""
import math

import numpy as np

f32 = np.float32
ROW = 37                     # dist, weight, grad[3], d[8], r[8], g[8], b[8]

_SUB = np.arange(8)
_SX = np.where(_SUB & 1, 1, -1).astype(np.float32)      # sub-voxel i: x from bit 0, y from bit 1, z from bit 2
_SY = np.where(_SUB & 2, 1, -1).astype(np.float32)
_SZ = np.where(_SUB & 4, 1, -1).astype(np.float32)


def gate(vs):
    """init :143: (float)(sqrt(3.) * voxel_size), computed in double"""
    return f32(math.sqrt(3.0) * float(vs))


def normalized(g):
    """Eigen normalized() as gsdf_normalized3: z = x^2 + (y^2 + z^2); v / sqrt(z) if z > 0"""
    g = np.asarray(g, np.float32)
    z = g[..., 0] * g[..., 0] + (g[..., 1] * g[..., 1] + g[..., 2] * g[..., 2])
    s = np.sqrt(np.where(z > 0, z, f32(1))).astype(np.float32)
    return np.where((z > 0)[..., None], g / s[..., None], g).astype(np.float32)


def select(keys, payload, vs):
    """indices of the kept voxels: exists (w > 0) and fabsf(dist) < gate, strict, in float"""
    d = payload[:, 0].astype(np.float32)
    return np.nonzero((payload[:, 4] > 0) & (np.abs(d) < gate(vs)))[0]


def subvoxel_centres(keys, vs):
    """getSubvoxelFloat (:208-212): vs * (0.25f * corner_i + idx), (n, 8, 3)"""
    corner = np.stack([_SX, _SY, _SZ], axis=1) * f32(0.25)
    return (f32(vs) * (corner[None, :, :] + keys.astype(np.float32)[:, None, :])).astype(np.float32)


def hr_voxels(payload, vs):
    """SdfVoxelHr(voxel, vs) of the given voxels (SdfVoxel.h:83-101): (grad (n, 3), d (n, 8))"""
    g = normalized(payload[:, 1:4])
    dist = payload[:, 0].astype(np.float32)
    vs4 = f32(0.25) * f32(vs)
    s0 = g[:, 0:1] * _SX[None, :]
    s1 = g[:, 1:2] * _SY[None, :]
    s2 = g[:, 2:3] * _SZ[None, :]
    d = (dist[:, None] + vs4 * ((s0 + s1) + s2)).astype(np.float32)          # :92-99, left to right
    return g, d


def interp(m, n, img):
    """interpolateImage(m = row, n = col) -- :57-82 as PhotoBA's ba_interp: weights in double (but for the float product w3), each term
    rounded to float, the four terms added in float; BGR -> RGB.  m, n: float32 arrays inside the image."""
    H, W = img.shape[:2]
    m = np.asarray(m, np.float32)
    n = np.asarray(n, np.float32)
    x = np.floor(m).astype(np.int64)
    y = np.floor(n).astype(np.int64)
    md, nd = m.astype(np.float64), n.astype(np.float64)
    out = np.empty(m.shape + (3,), np.float32)
    inner = ((x + 1) < H) & ((y + 1) < W)
    if inner.any():
        xi, yi, mi, ni = x[inner], y[inner], md[inner], nd[inner]
        w1 = (yi + 1.0 - ni) * (mi - xi)
        w2 = (yi + 1.0 - ni) * (xi + 1.0 - mi)
        # (n - y) * (m - x) multiplies two floats: a float product (the other three weights have a double factor)
        w3 = ((ni - yi).astype(np.float32) * (mi - xi).astype(np.float32)).astype(np.float64)
        w4 = (ni - yi) * (xi + 1.0 - mi)
        a = img[xi + 1, yi].astype(np.float64)
        b = img[xi, yi].astype(np.float64)
        c = img[xi + 1, yi + 1].astype(np.float64)
        d = img[xi, yi + 1].astype(np.float64)
        t = (((w1[:, None] * a).astype(np.float32) + (w2[:, None] * b).astype(np.float32))
             + (w3[:, None] * c).astype(np.float32)) + (w4[:, None] * d).astype(np.float32)
        out[inner] = t
    edge = ~inner & (y >= W) & ((x + 1) < H)
    if edge.any():
        xi, mi = x[edge], md[edge]
        yc = np.minimum(y[edge], W - 1)
        t = ((mi - xi)[:, None] * img[xi + 1, yc].astype(np.float64)).astype(np.float32) + \
            ((xi + 1.0 - mi)[:, None] * img[xi, yc].astype(np.float64)).astype(np.float32)
        out[edge] = t
    rest = ~inner & ~edge
    if rest.any():
        out[rest] = img[np.minimum(x[rest], H - 1), np.minimum(y[rest], W - 1)]
    return out[..., ::-1].copy()


def visible(vis_words, frame_id):
    """PhotoBA's rule (ba_visible): the bit frame_id of the voxel's vectors; ids past the vectors are unset"""
    vw = vis_words.shape[1]
    if frame_id < 0 or frame_id >= 32 * vw:
        return np.zeros(vis_words.shape[0], bool)
    return ((vis_words[:, frame_id >> 5] >> np.uint32(frame_id & 31)) & np.uint32(1)).astype(bool)


def compute(keys, payload, vis_words, images, poses, frame_idx, K, vs):
    """computeColor (:334-377) of the selected voxels.  Returns (sel, rows (n, 37), counts (n,)): sel indexes keys / payload in
    their (sorted) order, rows are gsdf_color_export's."""
    vs = f32(vs)
    sel = select(keys, payload, vs)
    k, p, vw = keys[sel], payload[sel], vis_words[sel]
    g, d = hr_voxels(p, vs)
    centres = subvoxel_centres(k, vs)
    n = len(sel)
    fx, fy, cx, cy = f32(K[0, 0]), f32(K[1, 1]), f32(K[0, 2]), f32(K[1, 2])
    H, W = images.shape[1:3]
    q = (centres - g[:, None, :] * d[:, :, None]).astype(np.float32)          # centre_i - grad d[i]
    sums = np.zeros((n, 8, 3), np.float32)
    counts = np.zeros(n, np.int64)
    for i, f in enumerate(frame_idx):
        seen = visible(vw, int(f))
        if not seen.any():
            continue
        P = np.asarray(poses[i], np.float32)
        R, t = P[:3, :3], P[:3, 3]
        e = (q[seen] - t[None, None, :]).astype(np.float32)
        # R^T e summed as ba_project: a + (b + c)
        px = R[0, 0] * e[..., 0] + (R[1, 0] * e[..., 1] + R[2, 0] * e[..., 2])
        py = R[0, 1] * e[..., 0] + (R[1, 1] * e[..., 1] + R[2, 1] * e[..., 2])
        pz = R[0, 2] * e[..., 0] + (R[1, 2] * e[..., 1] + R[2, 2] * e[..., 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            m = ((fx * px) / pz + cx).astype(np.float32)
            nn = ((fy * py) / pz + cy).astype(np.float32)
            bad = np.isnan(m).any(axis=1) | np.isnan(nn).any(axis=1)
            oob = ((m < 0) | (m >= f32(W)) | (nn < 0) | (nn >= f32(H))).any(axis=1)
        ok = ~bad & ~oob
        if not ok.any():
            continue
        idx = np.nonzero(seen)[0][ok]
        A = interp(nn[ok], m[ok], images[i])                                  # interpolateImage(n(i), m(i), img)
        sums[idx] = (sums[idx] + A).astype(np.float32)
        counts[idx] += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f32(1) / counts.astype(np.float32)).astype(np.float32)
        c = (inv[:, None, None] * sums).astype(np.float32)
        c = np.where(c < 0, f32(0), c)                                        # std::max(c, 0): NaN stays
        c = np.where(f32(1) < c, f32(1), c)                                   # std::min(c, 1): NaN stays
    rows = np.empty((n, ROW), np.float32)
    rows[:, 0] = p[:, 0]
    rows[:, 1] = p[:, 4]
    rows[:, 2:5] = g
    rows[:, 5:13] = d
    rows[:, 13:21] = c[:, :, 0]
    rows[:, 21:29] = c[:, :, 1]
    rows[:, 29:37] = c[:, :, 2]
    return sel, rows, counts


def cloud(keys_sel, rows, vis_sel, frame_idx, vs):
    """extractCloud (:251-330) literally, in the given voxel order, then by sub-voxel index: rows (m, 9) float32 of point, normal,
    colour"""
    vs4 = f32(0.25 * float(f32(vs)))
    seen = np.zeros(len(rows), bool)
    for f in frame_idx:
        seen |= visible(vis_sel, int(f))
    keep = seen & ~(rows[:, 1] < 5)
    nrm = -normalized(rows[:, 2:5])                                           # normalised a second time
    d = rows[:, 5:13]
    dvec = (nrm[:, None, :] * d[:, :, None]).astype(np.float32)               # (n, 8, 3)
    col = np.stack([rows[:, 13:21], rows[:, 21:29], rows[:, 29:37]], axis=2)
    ok = (np.abs(dvec) < vs4).all(axis=2) & ~np.isnan(col).any(axis=2) & keep[:, None]
    pts = (subvoxel_centres(keys_sel, vs) + dvec).astype(np.float32)
    out = np.concatenate([pts, np.broadcast_to(nrm[:, None, :], pts.shape), col], axis=2)
    return out[ok].reshape(-1, 9).astype(np.float32)


def ply_text(rows9):
    """the PLY of extractCloud (:302-327): the reference's header, floats as std::ostream writes them (%g, 6 digits),
    int(255.f * c)"""
    lines = ["ply", "format ascii 1.0", "element vertex %d" % len(rows9), "property float x", "property float y",
             "property float z", "property float nx", "property float ny", "property float nz", "property uchar red",
             "property uchar green", "property uchar blue", "end_header"]
    for r in rows9:
        cols = [int(f32(255) * f32(c)) for c in r[6:9]]
        lines.append(" ".join("%g" % float(v) for v in r[:6]) + " " + " ".join(str(c) for c in cols))
    return "\n".join(lines) + "\n"
