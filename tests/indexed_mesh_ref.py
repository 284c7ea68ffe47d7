"""numpy restatement of the indexed iso-surface mesh (gsdf_extract_mesh_indexed, include/gsdf.h), the reference statement for
the kernels of csrc/gsdf_mesh_index.hip.  Written from the definition, not as the kernels are: a dense grid over the bounding
box of the export, marching cubes over it in the z-y-x sweep with the project's CORNER / EDGE numbering and the committed case
table, and numpy's unique over the edge keys where the device sorts, flags and scans.

Number formats as mesh_interpolate's (csrc/gsdf_math.h): distances and positions float32, the three 1e-7 guards compared in
float64, mu a float32 quotient held in float64 and clamped, the blend in float64 rounded once.  The normal's blend is float32.
Input: keys (n, 3) int32 and payload (n, 5) float32 = dist, gx, gy, gz, weight, as GradSdf.export() / Oracle.export() give them."""
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
# corner c -> (dx, dy, dz) and edge e -> its two corners: the numbering of k_mesh (csrc/gsdf_kernels.hip)
CORNER = np.array([(1, 1, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 0, 1), (0, 1, 1)], np.int64)
EDGE = np.array([(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)], np.int64)
EDGE_AXIS = np.array([int(np.nonzero(CORNER[a] != CORNER[b])[0][0]) for a, b in EDGE], np.int64)
EDGE_LOW = np.array([np.minimum(CORNER[a], CORNER[b]) for a, b in EDGE], np.int64)
EDGE_DOWN = np.array([CORNER[a][ax] for (a, b), ax in zip(EDGE, EDGE_AXIS)], np.int64)       # 1: a is the upper endpoint


def interpolate(t0, t1, v0, v1, iso):
    """mesh_interpolate for m pairs: (positions (m, 3) float32, mu (m,) float32 -- 0 / 1 / 0 on the three guard returns)"""
    iso = f32(iso)
    t0, t1 = np.asarray(t0, f32), np.asarray(t1, f32)
    c0 = np.abs((iso - t0).astype(f64)) < 1e-7
    c1 = np.abs((iso - t1).astype(f64)) < 1e-7
    c2 = np.abs((t0 - t1).astype(f64)) < 1e-7
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = ((iso - t0) / (t1 - t0)).astype(f64)
    mu = np.where(mu > 1.0, 1.0, np.where(mu < 0, 0.0, mu))
    with np.errstate(invalid="ignore"):
        val = (v0.astype(f64) + mu[:, None] * (v1 - v0).astype(f64)).astype(f32)
    pos = np.where(c0[:, None], v0, np.where(c1[:, None], v1, np.where(c2[:, None], v0, val))).astype(f32)
    return pos, np.where(c0, 0.0, np.where(c1, 1.0, np.where(c2, 0.0, mu))).astype(f32)


def unit_gradient(g):
    """gsdf_normalized3: g / sqrt(|g|^2) in float32 where |g|^2 > 0 (summed x^2 + (y^2 + z^2)), else g"""
    g = np.asarray(g, f32)
    z = (g[:, 0] * g[:, 0] + (g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (g / np.sqrt(z)[:, None]).astype(f32)
    return np.where((z > 0)[:, None], u, g)


def compute(keys, payload, vs, iso=0.0, tri_table=None):
    """dict: soup (n, 3, 3) float32 in sweep order, edge_keys (n, 3) int64, V (nv, 3) float32, N (nv, 3) float32, F (n, 3) int32,
    table_triangles = what the case table lists for the map's cubes (n plus the degenerate triangles that were dropped)"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    pay = np.asarray(payload, f32).reshape(-1, 5)
    tri_table = TRI if tri_table is None else np.asarray(tri_table, np.int64).reshape(256, 16)
    vs, iso = f32(vs), f32(iso)
    empty = dict(soup=np.zeros((0, 3, 3), f32), edge_keys=np.zeros((0, 3), np.int64), V=np.zeros((0, 3), f32), N=np.zeros((0, 3), f32),
                 F=np.zeros((0, 3), np.int32), table_triangles=0)
    live = pay[:, 4] > 0
    keys, pay = keys[live], pay[live]
    if len(keys) == 0:
        return empty
    mn = keys.min(0)
    dim = keys.max(0) - mn + 2                                                # one empty layer behind the maximum: no cube there
    rel = keys - mn
    W = np.zeros((dim[2], dim[1], dim[0]), f32)
    D = np.zeros_like(W)
    G = np.zeros(W.shape + (3,), f32)
    W[rel[:, 2], rel[:, 1], rel[:, 0]] = pay[:, 4]
    D[rel[:, 2], rel[:, 1], rel[:, 0]] = pay[:, 0]
    G[rel[:, 2], rel[:, 1], rel[:, 0]] = pay[:, 1:4]
    nz, ny, nx = dim[2] - 1, dim[1] - 1, dim[0] - 1

    def at(a, off):
        return a[off[2]:off[2] + nz, off[1]:off[1] + ny, off[0]:off[0] + nx]

    ok = np.ones((nz, ny, nx), bool)
    cube = np.zeros((nz, ny, nx), np.int64)
    for c, off in enumerate(CORNER):
        ok &= at(W, off) > 0
        cube |= (at(D, off) > iso).astype(np.int64) << c
    zs, ys, xs = np.nonzero(ok & (cube != 0) & (cube != 255))                 # z outer, then y, then x: the sweep's order
    if len(zs) == 0:
        return empty
    cube = cube[zs, ys, xs]
    anchor = np.stack([xs, ys, zs], 1)
    origin = -(mn.astype(f32)) * vs

    def world(c):
        return (anchor + CORNER[c]).astype(f32) * vs - origin

    def dist(c):
        p = anchor + CORNER[c]
        return D[p[:, 2], p[:, 1], p[:, 0]]

    m = len(anchor)
    pts = np.zeros((m, 12, 3), f32)
    mus = np.zeros((m, 12), f32)
    eks = np.zeros((m, 12), np.int64)
    for e, (a, b) in enumerate(EDGE):
        pts[:, e], mus[:, e] = interpolate(dist(a), dist(b), world(a), world(b), iso)
        lo = anchor + EDGE_LOW[e]
        eks[:, e] = (((lo[:, 2] << 40) | (lo[:, 1] << 20) | lo[:, 0]) << 2) | EDGE_AXIS[e]
    tri = tri_table[cube][:, :15].reshape(-1, 5, 3)
    keep = tri[:, :, 0] >= 0
    listed = int(keep.sum())                                                   # before any degenerate triangle is dropped
    e = np.where(tri >= 0, tri, 0)
    rows = np.arange(m)[:, None, None]
    p = pts[rows, e]                                                           # (cubes, 5, 3 corners, 3)
    same = lambda u, v: np.all(u == v, axis=-1)                                # noqa: E731
    keep &= ~(same(p[:, :, 0], p[:, :, 1]) | same(p[:, :, 0], p[:, :, 2]) | same(p[:, :, 1], p[:, :, 2]))
    soup = p[keep].astype(f32)
    if len(soup) == 0:
        return dict(empty, table_triangles=listed)
    ek = eks[rows, e][keep]                                                    # (n, 3)
    # the weld: ids = ranks of the distinct keys; the first corner on an edge, in (face, corner) order, is the canonical one
    uniq, first, inverse = np.unique(ek.reshape(-1), return_index=True, return_inverse=True)
    F = inverse.reshape(-1, 3).astype(np.int32)
    V = soup.reshape(-1, 3)[first]
    edge_of = e[keep].reshape(-1)[first]
    cube_of = np.broadcast_to(rows, e.shape)[keep].reshape(-1)[first]
    mu = mus[cube_of, edge_of]
    lo = anchor[cube_of] + EDGE_LOW[edge_of]
    up = lo.copy()
    up[np.arange(len(up)), EDGE_AXIS[edge_of]] += 1
    down = EDGE_DOWN[edge_of].astype(bool)
    glo, gup = unit_gradient(G[lo[:, 2], lo[:, 1], lo[:, 0]]), unit_gradient(G[up[:, 2], up[:, 1], up[:, 0]])
    ga, gb = np.where(down[:, None], gup, glo), np.where(down[:, None], glo, gup)
    with np.errstate(invalid="ignore", over="ignore"):
        blend = ((f32(1) - mu)[:, None] * ga + mu[:, None] * gb).astype(f32)
        z = (blend[:, 0] * blend[:, 0] + (blend[:, 1] * blend[:, 1] + blend[:, 2] * blend[:, 2])).astype(f32)
    good = np.isfinite(z) & (z > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        N = np.where(good[:, None], -(blend / np.sqrt(z)[:, None]), f32(0)).astype(f32)
    return dict(soup=soup, edge_keys=ek, V=V.astype(f32), N=N, F=F, table_triangles=listed)


def sphere_map(radius=6.3, centre=(0.37, -0.21, 0.13), vs=0.02, band=3.0):
    """an analytic closed sphere as (keys, payload): every voxel with |dist| <= band vs, dist = (|p - c| - r) vs exactly rounded
    to float32, weight 1, gradient the outward radial direction.  radius and centre in voxels."""
    r = int(np.ceil(radius + band)) + 2
    g = np.arange(-r, r + 1)
    zz, yy, xx = np.meshgrid(g, g, g, indexing="ij")
    keys = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)                   # (z, y, x) order
    d = keys.astype(f64) - np.asarray(centre, f64)
    rho = np.sqrt((d * d).sum(1))
    sel = np.abs(rho - radius) <= band
    keys, d, rho = keys[sel], d[sel], rho[sel]
    pay = np.zeros((len(keys), 5), f32)
    pay[:, 0] = ((rho - radius) * float(f32(vs))).astype(f32)
    pay[:, 1:4] = (d / rho[:, None]).astype(f32)
    pay[:, 4] = 1
    return keys.astype(np.int32), pay


def manifold_counts(F):
    """(vertices used, undirected edges, faces, edges that do not lie in exactly two faces)"""
    F = np.asarray(F, np.int64)
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    e.sort(axis=1)
    _, cnt = np.unique(e, axis=0, return_counts=True)
    return len(np.unique(F)), len(cnt), len(F), int((cnt != 2).sum())

# WELD_MEASURED -- the cost of welding: the largest |V[F] - soup's own corner| per coordinate, in float32 spacings at
# max(|p|, |p'|, vs), as tests/test_indexed_mesh.py::test_weld_cost_in_float_spacings measures and prints it on the oracle's maps
# (spheres_64x48: 0, spheres_160x120: 1.000, tum_128x96: 1.000).  The GPU tests hold V[F] against gsdf_extract_mesh to it.
# It is the figure of THESE maps at the iso values the tests use, not a property of the weld: the restatement gives 2.000 on
# spheres_160x120 at iso = vs / 4, which no test uses.  A test on another map or iso value measures its own figure first.
# Why a move at all: two cubes walk a grid edge from opposite ends, p = fl(v0 + mu d) and p' = fl(v1 - mu' d) with d = fl(v1 - v0)
# on both sides; mu and mu' are float quotients of float differences (|mu + mu' - 1| <= 3 * 2^-24) and each position is rounded to
# float32 once.  What arithmetic alone allows is 1 + 3 * 1.001 < 4.01 of these units; the maps show one rounding.
# Why the unit has a floor of vs: the part of a move that comes from mu is absolute (up to 3 * 2^-24 vs), so against the spacing
# of a coordinate near 0 -- the maps straddle the origin -- it reads as dozens of spacings without being any larger.
# Not covered: an edge with both ends within 1e-7 of the iso value, where interpolate's guards return opposite ENDS from either
# side; the tests assert that their maps have none (no_guarded_edges).
WELD_MEASURED = 1.0


def weld_cost(V, F, soup, vs):
    """largest |V[F] - soup| per coordinate, in float32 spacings at max(|a|, |b|, vs)"""
    a, b = np.asarray(V, f32)[F], np.asarray(soup, f32)
    unit = np.spacing(np.maximum(np.maximum(np.abs(a), np.abs(b)), f32(vs))).astype(f64)
    return float((np.abs(a.astype(f64) - b.astype(f64)) / unit).max()) if a.size else 0.0


def no_guarded_edges(payload, iso=0.0):
    """the premise of the arithmetic beside WELD_MEASURED, checked wholesale: no voxel within 1e-7 of the iso value (a crossed edge whose ends lie within 1e-7
    of each other has both within 1e-7 of iso, up to a rounding)"""
    return not (np.abs(np.asarray(payload, f32)[:, 0].astype(f64) - float(f32(iso))) < 2e-7).any()


def parse_indexed_ply(path):
    """the binary PLY of MarchingCubes::saveIndexedPly: (V, N float32 [nv, 3], F int32 [nf, 3], header lines)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")[:-1]
    nv = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in head if l.startswith("element face")][0].split()[-1])
    vn = np.frombuffer(raw, "<f4", nv * 6, end).reshape(nv, 6)
    rec = np.frombuffer(raw, np.dtype([("n", "u1"), ("i", "<i4", (3,))]), nf, end + nv * 24)
    assert len(raw) == end + nv * 24 + nf * 13 and (rec["n"] == 3).all()
    return vn[:, :3].copy(), vn[:, 3:].copy(), rec["i"].astype(np.int32), head
