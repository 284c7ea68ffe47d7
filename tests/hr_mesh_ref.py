"""numpy restatement of HrLayeredMarchingCubes::computeIsoSurface (mesh/HrLayeredMarchingCubes.cpp:359-822), the reference
statement for gsdf_color_mesh.  Written as the reference is written, not as the kernel is: a bounding box over all keys, a
window of 4 fine z-layers that copyLayer refills every second z (copyCube where the map holds the coarse voxel, zeroWeights
where it does not), and the sweep over x < dim - 2 per axis that reads cube corners out of the window.  One fine z-layer is
processed at a time, vectorised over y and x.

Number formats as the reference's: tsdf, weights and positions float32; colours bytes; interpolate's comparisons and blend in
float64 with a float32 quotient.  Two definitions the reference leaves open:
  * (unsigned char)(NaN) -- the colour of a voxel no keyframe counted -- is 0;
  * getColor reads red, green and blue at the cell's own index (the reference reads green at idx + 1 and blue at idx + 2,
    :764-766: other cells of the window, stale or out of bounds -- not a function of the map).
Input: keys (n, 3) int32 and rows (n, 37) float32 as GradSdf.color_export() returns them."""
import os
import re

import numpy as np

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tri_table():
    txt = open(os.path.join(ROOT, "include", "gsdf_mc_tables.h")).read()
    t = re.search(r"GSDF_MC_TRI_TABLE\[256 \* 16\] = \{(.*?)\};", txt, re.S).group(1)
    return np.array([int(v) for v in re.findall(r"-?\d+", t)], np.int64).reshape(256, 16)


TRI = _tri_table()
# computeLutIndex :680-687: the cell offsets (dx, dy, dz) behind the bits 1, 2, 4, ..., 128
CORNER = ((1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 1, 1))
# the getVertex calls of :422-576, edge 0 .. 11: first and second cell
VERTEX_ENDS = (((1, 1, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, 0)), ((0, 0, 0), (0, 1, 0)), ((0, 1, 0), (1, 1, 0)),
               ((1, 1, 1), (1, 0, 1)), ((1, 0, 1), (0, 0, 1)), ((0, 0, 1), (0, 1, 1)), ((0, 1, 1), (1, 1, 1)),
               ((1, 1, 0), (1, 1, 1)), ((1, 0, 0), (1, 0, 1)), ((0, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 1, 1)))
# the getColor calls of the same lines: edges 2, 3, 6 and 7 name their cells the other way round (:458, :471, :510, :523)
COLOR_ENDS = (((1, 1, 0), (1, 0, 0)), ((1, 0, 0), (0, 0, 0)), ((0, 1, 0), (0, 0, 0)), ((1, 1, 0), (0, 1, 0)),
              ((1, 1, 1), (1, 0, 1)), ((1, 0, 1), (0, 0, 1)), ((0, 1, 1), (0, 0, 1)), ((1, 1, 1), (0, 1, 1)),
              ((1, 1, 0), (1, 1, 1)), ((1, 0, 0), (1, 0, 1)), ((0, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 1, 1)))


def to_byte(v):
    """static_cast<unsigned char>(float) for values in [0, 256): truncation; NaN is defined as 0"""
    v = np.asarray(v, f32)
    nan = np.isnan(v)
    return np.where(nan, 0, np.where(nan, f32(0), v).astype(np.int32) & 0xFF).astype(np.uint8)


def interpolate(t0, t1, v0, v1, iso):
    """:723-743 for m pairs: t0, t1 (m,) float32, v0, v1 (m, 3) float32"""
    iso = f32(iso)
    t0, t1 = np.asarray(t0, f32), np.asarray(t1, f32)
    c0 = np.abs((iso - t0).astype(f64)) < 1e-7
    c1 = np.abs((iso - t1).astype(f64)) < 1e-7
    c2 = np.abs((t0 - t1).astype(f64)) < 1e-7
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = ((iso - t0) / (t1 - t0)).astype(f64)                              # a float quotient held in a double
    mu = np.where(mu > 1.0, 1.0, np.where(mu < 0, 0.0, mu))
    with np.errstate(invalid="ignore"):
        val = (v0.astype(f64) + mu[:, None] * (v1 - v0).astype(f64)).astype(f32)
    return np.where(c0[:, None], v0, np.where(c1[:, None], v1, np.where(c2[:, None], v0, val))).astype(f32)


def compute(keys, rows, vs, iso=0.0):
    """(tris (n, 3, 3) float32, rgb (n, 3, 3) uint8) in the reference's sweep order"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    rows = np.asarray(rows, f32).reshape(-1, 37)
    vs, iso = f32(vs), f32(iso)
    empty = np.zeros((0, 3, 3), f32), np.zeros((0, 3, 3), np.uint8)
    if len(keys) == 0:
        return empty
    mn, mx = keys.min(0), keys.max(0)                                          # :374-381: over ALL keys
    origin = -(mn.astype(f32)) * vs                                            # :384
    dim = 2 * (mx - mn + 1)                                                    # :385
    tsdf = np.zeros((4, dim[1], dim[0]), f32)                                  # :388-399
    weights = np.zeros((4, dim[1], dim[0]), f32)
    red = np.zeros((4, dim[1], dim[0]), np.uint8)
    green = np.zeros((4, dim[1], dim[0]), np.uint8)
    blue = np.zeros((4, dim[1], dim[0]), np.uint8)
    layer_of = {}
    for cz in np.unique(keys[:, 2]):
        layer_of[int(cz)] = np.nonzero(keys[:, 2] == cz)[0]

    def copy_layer(z):
        """:589-607 for an even fine z: every coarse cell of the layer gets copyCube (:632-654) or zeroWeights (:611-628)"""
        k = z % 4
        idx = layer_of.get(z // 2 + int(mn[2]), np.zeros(0, np.int64))
        weights[k:k + 2] = 0                                                   # zeroWeights everywhere ...
        X, Y = 2 * (keys[idx, 0] - mn[0]), 2 * (keys[idx, 1] - mn[1])
        for i in range(8):                                                     # ... copyCube where the map holds the voxel
            bx, by, bz = i & 1, (i >> 1) & 1, i >> 2
            weights[k + bz, Y + by, X + bx] = rows[idx, 1]
            tsdf[k + bz, Y + by, X + bx] = rows[idx, 5 + i]
            red[k + bz, Y + by, X + bx] = to_byte(rows[idx, 13 + i] * f32(255))          # setVoxel :666-668
            green[k + bz, Y + by, X + bx] = to_byte(rows[idx, 21 + i] * f32(255))
            blue[k + bz, Y + by, X + bx] = to_byte(rows[idx, 29 + i] * f32(255))

    ny, nx = int(dim[1]) - 2, int(dim[0]) - 2
    out_t, out_c = [], []
    copy_layer(0)
    for z in range(int(dim[2]) - 2):                                           # :410
        if z % 2:
            copy_layer(z + 1)
        if ny <= 0 or nx <= 0:
            continue

        def cells(a, off):                                                     # the window read at (x + dx, y + dy, (z + dz) % 4)
            return a[(z + off[2]) % 4, off[1]:off[1] + ny, off[0]:off[0] + nx]

        ok = np.ones((ny, nx), bool)                                           # computeLutIndex :692-699
        cube = np.zeros((ny, nx), np.int64)
        for c, off in enumerate(CORNER):
            ok &= ~(cells(weights, off) == f32(0))
            cube |= (cells(tsdf, off) > iso).astype(np.int64) << c
        cube = np.where(ok, cube, 0)
        ys, xs = np.nonzero((cube != 0) & (cube != 255))                       # y outer, x inner: the sweep's order
        if len(ys) == 0:
            continue
        cube = cube[ys, xs]

        def at(a, off):
            return a[(z + off[2]) % 4, ys + off[1], xs + off[0]]

        def world(off):                                                        # voxelToWorld :817-821
            ijk = np.stack([xs + off[0], ys + off[1], np.full(len(xs), z + off[2])], 1).astype(f32)
            return f32(0.5) * (ijk * vs) - origin

        def colour(off):                                                       # getColor :765-768, channels at the cell's own index
            return np.stack([at(red, off), at(green, off), at(blue, off)], 1).astype(f32) / f32(255)

        pts = np.zeros((len(ys), 12, 3), f32)
        col = np.zeros((len(ys), 12, 3), np.uint8)
        for e in range(12):
            a, b = VERTEX_ENDS[e]
            pts[:, e] = interpolate(at(tsdf, a), at(tsdf, b), world(a), world(b), iso)   # getVertex :746-753
            a, b = COLOR_ENDS[e]
            col[:, e] = to_byte(interpolate(at(tsdf, a), at(tsdf, b), colour(a), colour(b), iso) * f32(255))
        tri = TRI[cube][:, :15].reshape(-1, 5, 3)                              # computeTriangles :776-804
        live = tri[:, :, 0] >= 0
        e = np.where(tri >= 0, tri, 0)
        rows_i = np.arange(len(ys))[:, None, None]
        p, cc = pts[rows_i, e], col[rows_i, e]                                 # (cubes, 5, 3 vertices, 3)
        same = lambda u, v: np.all(u == v, axis=-1)                            # noqa: E731
        live &= ~(same(p[:, :, 0], p[:, :, 1]) | same(p[:, :, 0], p[:, :, 2]) | same(p[:, :, 1], p[:, :, 2]))     # :789
        out_t.append(p[live])
        out_c.append(cc[live])
    if not out_t:
        return empty
    return np.concatenate(out_t).astype(f32), np.concatenate(out_c).astype(np.uint8)


def ply_text(tris, rgb):
    """savePly :824-864: floats as std::ostream writes them (%g, 6 digits), one vertex per triangle corner, faces of
    consecutive indices"""
    v = np.asarray(tris, f32).reshape(-1, 3)
    c = np.asarray(rgb, np.uint8).reshape(-1, 3)
    lines = ["ply", "format ascii 1.0", "element vertex %d" % len(v), "property float x", "property float y", "property float z",
             "property uchar red", "property uchar green", "property uchar blue", "element face %d" % (len(v) // 3),
             "property list uchar int vertex_indices", "end_header"]
    lines += ["%g %g %g %d %d %d" % (float(p[0]), float(p[1]), float(p[2]), int(q[0]), int(q[1]), int(q[2])) for p, q in zip(v, c)]
    lines += ["3 %d %d %d" % (3 * i, 3 * i + 1, 3 * i + 2) for i in range(len(v) // 3)]
    return "\n".join(lines) + "\n"
