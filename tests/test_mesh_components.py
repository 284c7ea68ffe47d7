"""Connected components of the indexed mesh and the filtered mesh (gsdf_mesh_components, gsdf_extract_mesh_indexed_filtered)
without a GPU: the C-ABI exports both entries; the numpy restatement (tests/mesh_components_ref.py) agrees with scipy's connected
components on the oracle's maps, its tables add up, the filter's identities hold, and the long strip is one component."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import indexed_mesh_ref as IM  # noqa: E402
import mesh_components_ref as MC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_abi_exports_the_mesh_component_entries(pkg):
    so = os.path.join(ROOT, "gradient-sdf_amd", "csrc", "libgsdf.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "gsdf.h")).read()
    for name in ("gsdf_mesh_components", "gsdf_extract_mesh_indexed_filtered"):
        assert re.search(r"\bT %s\b" % name, out), name
        assert re.search(r"\bint %s\(gsdf_ctx\* c, float iso, const int8_t tri_table\[256 \* 16\]," % name, hdr), name
        assert name in pkg.binding.ABI_SYMBOLS
    assert re.search(r"#define GSDF_MESH_KEEP_LARGEST \(-1\)", hdr)
    assert pkg.binding.MESH_KEEP_LARGEST == -1 == MC.KEEP_LARGEST and pkg.MESH_KEEP_LARGEST == -1
    assert callable(pkg.GradSdf.mesh_components) and callable(pkg.GradSdf.extract_mesh_indexed_filtered)


def _oracle_mesh(O, name):
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    depth = z["depth_u16"].astype(np.float32) * np.float32(z["unit"])
    o = O.Oracle(z["voxel_size"], z["trunc_dist"], int(z["W"]), int(z["H"]), z["K"])
    for i in range(depth.shape[0] - 1):                                        # the fixture's map: all frames but the last
        o.update(depth[i], z["R"][i], z["t"][i])
    keys, pay = o.export()
    return IM.compute(keys, pay, f32(z["voxel_size"]))


@pytest.fixture(scope="module", params=["spheres_64x48", "spheres_160x120", "tum_128x96"])
def oracle_case(O, request):
    r = _oracle_mesh(O, request.param)
    return request.param, r["V"], r["N"], r["F"], MC.compute(r["V"], r["F"])


def test_restatement_agrees_with_scipy(oracle_case):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    name, V, N, F, c = oracle_case
    nv = len(V)
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    n, lab = connected_components(sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(nv, nv)).tocsr(), directed=False)
    first = np.full(n, nv, np.int64)
    np.minimum.at(first, lab, np.arange(nv))                                   # scipy's labels renumbered by smallest vertex
    renum = np.argsort(np.argsort(first))[lab]
    assert n == c["C"] and np.array_equal(renum, c["vertex_comp"])


def test_component_tables_add_up(oracle_case):
    name, V, N, F, c = oracle_case
    vc, fc, counts, bbox = c["vertex_comp"], c["face_comp"], c["counts"], c["bbox"]
    order = np.argsort(-counts[:, 0], kind="stable")
    print("%s: faces %d vertices %d components %d (rounds %d), face counts %s, under 10 faces: %d"
          % (name, len(F), len(V), c["C"], c["rounds"], " / ".join(str(int(counts[i, 0])) for i in order), int((counts[:, 0] < 10).sum())))
    assert vc.dtype == np.int32 and fc.dtype == np.int32 and counts.dtype == np.int32 and bbox.dtype == np.float32
    assert (vc[F] == fc[:, None]).all()                                        # a face lies in the component of each of its vertices
    assert counts[:, 0].sum() == len(F) and counts[:, 1].sum() == len(V) and (counts > 0).all()
    assert vc[0] == 0 and np.array_equal(np.unique(vc), np.arange(c["C"]))
    firsts = np.array([np.flatnonzero(vc == i)[0] for i in range(c["C"])])
    assert (np.diff(firsts) > 0).all()                                         # ids ascend with the smallest vertex id
    for i in range(c["C"]):
        P = V[vc == i]
        assert np.array_equal(bbox[i, :3], P.min(0)) and np.array_equal(bbox[i, 3:], P.max(0))


def test_filter_identities(oracle_case):
    name, V, N, F, c = oracle_case
    V1, N1, F1, C, kept = MC.filter_mesh(V, N, F, 1, c)
    assert kept == C and V1.tobytes() == V.tobytes() and N1.tobytes() == N.tobytes() and F1.tobytes() == F.tobytes()
    faces = c["counts"][:, 0]
    top = int(faces.max())
    assert (faces == top).sum() == 1                                           # unique on all three maps
    a, b = MC.filter_mesh(V, N, F, MC.KEEP_LARGEST, c), MC.filter_mesh(V, N, F, top, c)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    assert a[3:] == b[3:] == (C, 1) and len(a[2]) == top
    for m in (2, 10, 100, top, top + 1, 10**9, MC.KEEP_LARGEST):
        Vm, Nm, Fm, _, k = MC.filter_mesh(V, N, F, m, c)
        want = int((faces >= m).sum()) if m > 0 else 1
        assert k == want and len(Fm) == (int(faces[faces >= m].sum()) if m > 0 else top)
        assert len(np.unique(Fm)) == len(Vm) == len(Nm)                        # every kept vertex is used, none is missing
        if len(Fm):
            assert Fm.min() == 0 and Fm.max() == len(Vm) - 1
            assert np.array_equal(Vm[Fm], V[F[np.isin(c["face_comp"], np.flatnonzero(MC.keep_mask(c["counts"], m)))]])
    with pytest.raises(ValueError):
        MC.keep_mask(c["counts"], 0)


def _strip_mesh(pieces):
    keys = np.concatenate([p[0] for p in pieces])
    pay = np.concatenate([p[1] for p in pieces])
    r = IM.compute(keys, pay, 0.02)
    return r["V"], r["N"], r["F"]


def test_long_strip_is_one_component():
    L = 1000
    keys, pay = MC.strip_map(L)
    assert len(keys) == 4 * (2 * L + 1) and keys[:, 0].min() == -L and keys[:, 0].max() == L
    assert len(np.unique(keys >> 2, axis=0)) > 400                             # hundreds of 4 x 4 x 4 blocks
    V, N, F = _strip_mesh([(keys, pay)])
    c = MC.compute(V, F)
    print("strip: faces %d vertices %d components %d, restatement rounds %d" % (len(F), len(V), c["C"], c["rounds"]))
    assert (len(F), len(V)) == MC.strip_counts(L) == (4 * L, 4 * L + 2)
    assert c["C"] == 1 and c["counts"].tolist() == [[4 * L, 4 * L + 2]]
    assert not c["vertex_comp"].any() and not c["face_comp"].any()


def test_two_equal_strips_keep_largest_keeps_component_zero():
    L = 40
    V, N, F = _strip_mesh([MC.strip_map(L), MC.strip_map(L, y0=4), MC.strip_map(0, y0=8, cubes=3)])
    c = MC.compute(V, F)
    big, small = MC.strip_counts(L), MC.strip_counts(cubes=3)
    assert c["C"] == 3 and c["counts"].tolist() == [list(big), list(big), list(small)]
    Vk, Nk, Fk, C, kept = MC.filter_mesh(V, N, F, MC.KEEP_LARGEST, c)
    assert (C, kept) == (3, 1) and len(Fk) == big[0]
    assert c["vertex_comp"][0] == 0 and np.array_equal(Vk, V[c["vertex_comp"] == 0])       # the one that holds vertex 0
    Vk, Nk, Fk, C, kept = MC.filter_mesh(V, N, F, small[0] + 1, c)                          # between the two counts: only the piece goes
    assert kept == 2 and len(Fk) == 2 * big[0] and np.array_equal(Vk, V[c["vertex_comp"] < 2])
