"""Allocation failures inside the library: every device allocation the owning types (csrc/gsdf_dev.h) make for an entry point
fails in turn (gsdf_debug_fail_alloc, test library), and the context must be left whole -- no frame after a failed
gsdf_normals_init, no BA setup after a failed gsdf_ba_setup, the old table after a failed gsdf_grow, nothing at all after a failed
temporary -- and give, once the hook is disarmed, bit for bit what a context that never saw a failure gives.

The number of allocations of an entry point is never written down here: a clean call tells it through the hook's return value.
A context whose entry point returned an error is only ever asked what must be refused on the host, gsdf_normals_cache (a plain
copy of `planes`) before gsdf_update_dev; every step asserts, so the first failure ends the test."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 160, 120                      # the sequence and the map of __graft_entry__.smoke()
VS = np.float32(0.02)
T = np.float32(5) * VS
CAP = 18
OK, ERR_INVALID, ERR_HIP = 0, 3, 4


@pytest.fixture(scope="module")
def L(pkg):
    lib = pkg.binding.load_test_lib()
    yield lib
    lib.gsdf_debug_fail_alloc(0)


@pytest.fixture(scope="module")
def seq(pkg):
    return pkg.synth.Sequence("spheres", W, H, n_frames=3, seed=1, step_deg=0.5)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _bits(a, b):
    """the same arrays bit for bit (tuples: element by element)"""
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_bits(x, y) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _counted(L, call):
    """a clean call: (its result, the owned allocations it made)"""
    L.gsdf_debug_fail_alloc(0)
    out = call()
    return out, L.gsdf_debug_fail_alloc(0)


def _code_with_failure(pkg, L, k, call):
    """the error code of `call` when its k-th owned allocation fails"""
    L.gsdf_debug_fail_alloc(k)
    try:
        call()
        return OK
    except pkg.binding.GsdfError as e:
        return e.code
    finally:
        L.gsdf_debug_fail_alloc(0)


def _create(L):
    h = C.c_void_p()
    assert L.gsdf_create(C.byref(h), VS, T, CAP, 0) == OK
    return h


def _init(L, h, seq):
    K = np.ascontiguousarray(seq.K, np.float32).reshape(9)
    return L.gsdf_normals_init(h, W, H, _fp(K), 11)


def _wrap(pkg, L, h, seq):
    """the facade over an existing context: its constructor calls gsdf_normals_init"""
    return pkg.GradSdf(VS, T, W, H, seq.K, capacity_log2=CAP, lib=L, _handle=h)


def _fuse2(g, seq):
    for i in range(2):
        g.update(*seq.frame(i))
    return g.export(sorted=True)


def _must_refuse(L, h, seq):
    """the context has no frame: gsdf_normals_cache refuses, and only then gsdf_update_dev is asked"""
    planes = np.zeros(11 * W * H, np.float32)
    assert L.gsdf_normals_cache(h, _fp(planes)) == ERR_INVALID, "the frame gate is open after a failed gsdf_normals_init"
    d, R, t = seq.frame(0)
    nbytes = W * H * 4
    dev = C.c_void_p()
    assert L.gsdf_dev_alloc(h, C.byref(dev), nbytes) == OK            # the caller's memory: not an owned allocation
    d = np.ascontiguousarray(d, np.float32)
    assert L.gsdf_dev_upload(h, dev, d.ctypes.data_as(C.c_void_p), nbytes) == OK
    R = np.ascontiguousarray(R, np.float32).reshape(9)
    t = np.ascontiguousarray(t, np.float32).reshape(3)
    assert L.gsdf_update_dev(h, dev, _fp(R), _fp(t)) == ERR_INVALID
    assert L.gsdf_dev_free(h, dev) == OK


def _init_allocs(L, seq):
    h = _create(L)
    rc, n = _counted(L, lambda: _init(L, h, seq))
    L.gsdf_destroy(h)
    assert rc == OK and n >= 10, (rc, n)
    return n


def test_normals_init_failure_leaves_no_frame(pkg, L, seq):
    n = _init_allocs(L, seq)
    g = _wrap(pkg, L, _create(L), seq)
    want = _fuse2(g, seq)                                             # a context that never saw a failure
    g.close()
    assert want[0].shape[0] > 1000
    print("MEASURED gsdf_normals_init makes %d owned allocations" % n)
    for k in range(1, n + 1):
        h = _create(L)
        L.gsdf_debug_fail_alloc(k)
        rc = _init(L, h, seq)
        assert L.gsdf_debug_fail_alloc(0) == k, k                     # the k-th allocation was the last one made
        assert rc == ERR_HIP, (k, rc)
        _must_refuse(L, h, seq)
        g = _wrap(pkg, L, h, seq)                                     # disarmed: init again
        got = _fuse2(g, seq)
        g.close()
        assert _bits(got, want), k


def test_normals_reinit_failure_leaves_no_frame_and_the_map(pkg, L, seq):
    n = _init_allocs(L, seq)

    def run(k):
        g = _wrap(pkg, L, _create(L), seq)
        first = _fuse2(g, seq)
        if k:
            L.gsdf_debug_fail_alloc(k)
            rc = _init(L, g.h, seq)
            L.gsdf_debug_fail_alloc(0)
            assert rc == ERR_HIP, (k, rc)
            _must_refuse(L, g.h, seq)
            assert _bits(g.export(sorted=True), first), k             # the map fused before the failed call
        assert _init(L, g.h, seq) == OK
        second = _fuse2(g, seq)                                       # the same two frames once more, into the same map
        g.close()
        return first, second

    want = run(0)
    for k in range(1, n + 1):
        assert _bits(run(k), want), k


def _ba_scene(pkg, L):
    """tests/test_gpu_color_upsampler.py::_scene without the BA iterations, on the test library"""
    n_frames = 6
    s = pkg.synth.Sequence("tum", W, H, n_frames=n_frames, seed=0, noise=False)
    kf = np.arange(n_frames, dtype=np.int32)
    imgs = np.stack([pkg.synth.render_color_bgr(s, int(i)) for i in kf]).astype(np.float32)
    P = np.stack([pkg.synth.pose16(*s.pose(int(i))) for i in kf]).astype(np.float32)
    g = pkg.GradSdf(VS, T, W, H, s.K, capacity_log2=20, lib=L)
    g.enable_vis(64)
    for i in range(n_frames):
        g.update(*s.frame(i))
    return g, imgs, P, kf


def test_ba_setup_failure_leaves_no_setup(pkg, L):
    g, imgs, P, kf = _ba_scene(pkg, L)
    _, n = _counted(L, lambda: g.ba_setup(imgs, P, kf))
    E0 = g.ba_energy()
    assert np.isfinite(E0) and n >= 7, (E0, n)
    ok = []
    for k in range(1, n + 1):
        code = _code_with_failure(pkg, L, k, lambda: g.ba_setup(imgs, P, kf))
        assert code in (OK, ERR_HIP), (k, code)
        e = C.c_float(np.nan)
        rc = L.gsdf_ba_energy(g.h, C.byref(e))
        if code == ERR_HIP:
            assert rc == ERR_INVALID, (k, rc)                         # no BA setup: refused on the host
        else:
            assert rc == OK and np.isfinite(e.value), (k, rc, e.value)
            ok.append(k)
    print("MEASURED gsdf_ba_setup makes %d owned allocations; it survives the failure of %s" % (n, ok))
    # the optional buffers are the last four it allocates: the gate list, its rocPRIM scratch, counter2, the mean cache
    assert ok == list(range(n - 3, n + 1)), (ok, n)
    assert 0 < len(ok) < n
    g.ba_setup(imgs, P, kf)
    assert abs(g.ba_energy() - E0) <= 1e-6 * abs(E0)
    g.close()


def test_grow_failure_leaves_the_map(pkg, L, seq):
    def fused():
        g = _wrap(pkg, L, _create(L), seq)
        g.enable_vis(32)
        return g, _fuse2(g, seq)

    a, before = fused()
    _, n = _counted(L, lambda: a.grow(CAP + 1))
    assert n >= 3 and a.capacity_log2() == CAP + 1, n
    assert _bits(a.export(sorted=True), before)
    a.close()
    g, before = fused()
    vis_before = g.export_vis()
    print("MEASURED gsdf_grow makes %d owned allocations" % n)
    for k in range(1, n + 1):
        assert _code_with_failure(pkg, L, k, lambda: g.grow(CAP + 1)) == ERR_HIP, k
        assert g.capacity_log2() == CAP
        assert _bits(g.export(sorted=True), before), k
        assert _bits(g.export_vis(), vis_before), k
    g.grow(CAP + 1)
    assert g.capacity_log2() == CAP + 1 and _bits(g.export(sorted=True), before)
    g.close()


@pytest.mark.parametrize("what", ["export", "query", "raycast", "extract_mesh", "extract_mesh_indexed", "mesh_components",
                                  "extract_mesh_indexed_filtered", "surface_cloud", "gradient_angles", "gradient_stats"])
def test_temporary_failure_leaves_nothing_behind(pkg, L, seq, what):
    g = _wrap(pkg, L, _create(L), seq)
    _fuse2(g, seq)
    _, R, t = seq.frame(1)
    rng = np.random.default_rng(0)
    pts = (rng.uniform(-1, 1, (10000, 3)) * 0.5 + np.array([0, 0, 1.5])).astype(np.float32)
    assert pts.shape[0] * 8 * 4 > 256 * 1024                         # above GSDF_SCRATCH_BYTES: the call allocates
    sph = np.asarray(seq.spheres, np.float32).reshape(-1, 4)          # the scene's own spheres (test_gpu_gradient_analysis.py)
    thr = [0.011, 0.1]
    call = {"export": lambda: g.export(sorted=True), "query": lambda: g.query(pts),
            "raycast": lambda: g.raycast(R, t), "extract_mesh": lambda: (g.extract_mesh(),),
            "extract_mesh_indexed": lambda: g.extract_mesh_indexed(), "mesh_components": lambda: g.mesh_components(),
            "extract_mesh_indexed_filtered": lambda: g.extract_mesh_indexed_filtered(2),
            "surface_cloud": lambda: (g.surface_cloud(),), "gradient_angles": lambda: g.gradient_angles(sph),
            "gradient_stats": lambda: (g.gradient_stats(sph, thr),)}[what]
    call()                                                            # (what the context keeps is allocated now)
    want, n = _counted(L, call)
    assert n >= 1 and want[0].shape[0] > 0, n
    if what == "extract_mesh_indexed_filtered":
        assert want[2].shape[0] > 0 and want[4] >= 1, want[3:]        # faces were kept, of at least one component
    if what == "gradient_stats":
        assert (want[0][:, -1, 0] > 0).all(), want[0][:, :, 0]        # every estimator counted voxels: the map is not empty
    print("MEASURED %s makes %d owned allocations" % (what, n))
    for k in range(1, n + 1):
        assert _code_with_failure(pkg, L, k, call) == ERR_HIP, k
        assert _bits(call(), want), k
    g.close()
