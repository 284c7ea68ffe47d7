"""numpy restatement of the connected components of the indexed mesh and of the filtered mesh (gsdf_mesh_components,
gsdf_extract_mesh_indexed_filtered, include/gsdf.h), the reference statement for the kernels of csrc/gsdf_mesh_components.hip.
Written from the definition: a union-find over the faces by repeated np.minimum.at (hook the larger root under the smaller) and
pointer jumping to a fixed point, ids by the smallest vertex, counts, boxes, and the filter with its remap.  Pure numpy: scipy is
used only by the CPU test that checks this file against scipy.sparse.csgraph."""
import numpy as np

f32 = np.float32
KEEP_LARGEST = -1


def components(F, n_vertices):
    """(vertex_comp int32 [nv], face_comp int32 [nf], rounds): two vertices are adjacent iff a face names both; ids 0 .. C-1 in
    ascending order of a component's smallest vertex id.  rounds = hook-then-compress rounds until no edge joins two roots."""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    parent = np.arange(n_vertices, dtype=np.int64)
    a = np.concatenate([F[:, 0], F[:, 1]])
    b = np.concatenate([F[:, 1], F[:, 2]])
    rounds = 0
    while True:
        ra, rb = parent[a], parent[b]                                          # roots: parent is fully compressed here
        diff = ra != rb
        if not diff.any():
            break
        rounds += 1
        np.minimum.at(parent, np.maximum(ra, rb)[diff], np.minimum(ra, rb)[diff])
        while True:                                                            # pointer jumping: parent[v] <= v, to the root
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
    roots = np.flatnonzero(parent == np.arange(n_vertices))                   # ascending root = ascending smallest vertex
    vcomp = np.searchsorted(roots, parent).astype(np.int32)
    fcomp = vcomp[F[:, 0]].astype(np.int32) if len(F) else np.zeros(0, np.int32)
    return vcomp, fcomp, rounds


def tables(V, vcomp, fcomp):
    """(counts int32 [C, 2] = faces, vertices; bbox float32 [C, 6] = min x y z, max x y z)"""
    C = int(vcomp.max()) + 1 if len(vcomp) else 0
    counts = np.stack([np.bincount(fcomp, minlength=C), np.bincount(vcomp, minlength=C)], 1).astype(np.int32).reshape(C, 2)
    bbox = np.empty((C, 6), f32)
    bbox[:, :3], bbox[:, 3:] = np.inf, -np.inf
    V = np.asarray(V, f32)
    for k in range(3):
        np.minimum.at(bbox[:, k], vcomp, V[:, k])
        np.maximum.at(bbox[:, 3 + k], vcomp, V[:, k])
    return counts, bbox


def compute(V, F):
    """dict: vertex_comp, face_comp, counts, bbox, rounds, C"""
    vcomp, fcomp, rounds = components(F, len(V))
    counts, bbox = tables(V, vcomp, fcomp)
    return dict(vertex_comp=vcomp, face_comp=fcomp, counts=counts, bbox=bbox, rounds=rounds, C=len(counts))


def keep_mask(counts, min_faces):
    """bool [C]: min_faces >= 1 keeps the components with at least that many faces; KEEP_LARGEST the one with the most faces, the
    lowest id among equals"""
    faces = np.asarray(counts)[:, 0]
    if min_faces == KEEP_LARGEST:
        keep = np.zeros(len(faces), bool)
        if len(faces):
            keep[int(np.argmax(faces))] = True                                 # argmax: the first among equals
        return keep
    if min_faces < 1:
        raise ValueError("min_faces must be >= 1 or KEEP_LARGEST")
    return faces >= min_faces


def filter_mesh(V, N, F, min_faces, comp=None):
    """(V', N', F' int32, C, kept): the kept vertices in ascending original id with their bytes, the kept faces in their order with
    the ids remapped to the rank among the kept"""
    comp = compute(V, F) if comp is None else comp
    keep = keep_mask(comp["counts"], min_faces)
    vk = keep[comp["vertex_comp"]] if len(V) else np.zeros(0, bool)
    fk = keep[comp["face_comp"]] if len(F) else np.zeros(0, bool)
    new_id = np.cumsum(vk) - 1
    Fk = new_id[np.asarray(F, np.int64)[fk]].astype(np.int32).reshape(-1, 3)
    return np.asarray(V)[vk], np.asarray(N)[vk], Fk, comp["C"], int(keep.sum())


def strip_map(length, y0=0, vs=0.02, cubes=None):
    """a flat strip, the shape a round-limited label spread gets wrong: (keys int32 [n, 3], payload float32 [n, 5] = dist, g, w)
    of the voxels x in -length .. length (or 0 .. cubes), y in {y0, y0 + 1}, z in {0, 1} with dist = (z - 0.4f) vs, weight 1,
    gradient +z.  One row of 2 length (or `cubes`) cubes, each cut by the plane z = 0.4 into two faces: 4 length faces, 2 (2 length
    + 1) vertices, one component whose diameter is the strip's length."""
    xs = np.arange(-length, length + 1) if cubes is None else np.arange(0, cubes + 1)
    x, y, z = np.meshgrid(xs, np.array([y0, y0 + 1]), np.array([0, 1]), indexing="ij")
    keys = np.stack([x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)
    pay = np.zeros((len(keys), 5), f32)
    pay[:, 0] = (keys[:, 2].astype(f32) - f32(0.4)) * f32(vs)
    pay[:, 3] = 1
    pay[:, 4] = 1
    return keys, pay


def strip_counts(length=None, cubes=None):
    """(faces, vertices) of strip_map's surface"""
    n = 2 * length if cubes is None else cubes
    return 2 * n, 2 * (n + 1)
