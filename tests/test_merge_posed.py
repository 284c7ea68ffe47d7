"""gsdf_merge_from_posed without a GPU: the enumeration's host helper (gsdf_posed_blocks in csrc/gsdf_posed.h, exported by the
test build as plain integers) against a float64 brute force, and the numpy restatement tests/merge_posed_ref.py on the CPU
oracle's map at the poses whose answer is known."""
import ctypes as C

import numpy as np
import pytest

import merge_posed_ref as ref

f32 = np.float32
VS = f32(0.02)


@pytest.fixture(scope="module")
def posed_blocks(pkg):
    L = pkg.binding.load_test_lib()
    out = np.zeros((4096, 3), np.int32)

    def call(pose7, block):
        p = np.ascontiguousarray(pose7, f32)
        b = np.ascontiguousarray(block, np.int32)
        n = L.gsdf_debug_posed_blocks(p.ctypes.data_as(C.POINTER(C.c_float)), C.c_float(VS), b.ctypes.data_as(C.POINTER(C.c_int32)),
                                      out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
        assert n <= len(out)
        return n, out[:max(n, 0)].copy()
    return call


def _random_pose(rng, far):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    q *= np.sqrt(1 + rng.uniform(-1e-4, 1e-4))                       # the quaternion is used as it comes: | |q|^2 - 1 | <= 1e-4
    t = rng.uniform(-1, 1, 3) * (rng.choice([0.05, 2.0, 40.0]) if far else 0.05)
    return np.concatenate([t, q]).astype(f32)


def test_enumeration_lists_every_block_within_the_bound(O, posed_blocks):
    """10^4 seeded (pose, block) pairs.  Brute force in float64: the image of the src block's centre is c = A b + t with
    A = (R^T)^-1 of the float32 R the kernel uses -- the exact preimage relation of q = R^T (c_K - t) -- and every dst block that
    holds a voxel centre within (1.5 sqrt(3) + sqrt(3) / 2) vs of it must be in the helper's list.  The list is also finite and
    small: at most 64 blocks at these magnitudes (27 for a ball of 3.75 voxels that is axis-aligned at its worst)."""
    rng = np.random.default_rng(11)
    bound = 1.5 * np.sqrt(3) + np.sqrt(3) / 2
    off = np.stack(np.meshgrid(*[np.arange(-12, 16)] * 3, indexing="ij"), -1).reshape(-1, 3)       # voxels around the image
    worst, most = 0.0, 0
    for it in range(10000):
        pose = _random_pose(rng, far=it % 2 == 1)
        block = rng.integers(-600, 600, 3).astype(np.int32)
        n, got = posed_blocks(pose, block)
        assert 0 < n <= 64, (pose, block, n)
        R = O.quat_to_R(pose[3:]).astype(np.float64)
        A = np.linalg.inv(R.T)
        c = A @ (4.0 * block + 1.5) + pose[:3].astype(np.float64) / np.float64(VS)
        vox = np.floor(c).astype(np.int64)[None, :] + off
        need = np.unique(vox[np.linalg.norm(vox - c[None, :], axis=1) <= bound] >> 2, axis=0)
        have = {tuple(r) for r in got.tolist()}
        assert len(have) == n, "a block is listed twice"
        missing = [tuple(r) for r in need.tolist() if tuple(r) not in have]
        assert not missing, (pose, block, missing)
        most = max(most, n)
        # how far the farthest listed block's nearest voxel centre lies from the image: the radius in use, from outside
        lo = got.astype(np.float64) * 4
        d = np.maximum(np.maximum(lo - c, c - (lo + 3)), 0)
        worst = max(worst, float(np.linalg.norm(d, axis=1).max()))
    print("enumeration: at most %d blocks per src block, farthest listed block %.3f voxels from the image (bound %.3f)" % (most, worst, bound))
    # the radius gsdf_posed.h states, at the largest magnitude here (|image| <= sqrt(3) * 2400 + 2000 voxels): no block beyond it
    assert worst <= 1.001 * 2 * np.sqrt(3) + 0.25 + (np.sqrt(3) * 2400 + 2000 + 17) * 2.0 ** -17


def test_enumeration_refuses_what_it_cannot_list(posed_blocks):
    """an image beyond +-2^22 voxels, or one that is not finite, is reported (-1), never listed"""
    far = np.array([f32(2.0 ** 22) * VS, 0, 0, 0, 0, 0, 1], f32)
    assert posed_blocks(far, (0, 0, 0))[0] == -1
    assert posed_blocks(np.array([np.inf, 0, 0, 0, 0, 0, 1], f32), (0, 0, 0))[0] == -1
    ok = np.array([f32(2.0 ** 21) * VS, 0, 0, 0, 0, 0, 1], f32)
    n, got = posed_blocks(ok, (0, 0, 0))
    assert n > 0 and (got[:, 0] >= 2 ** 19 - 8).all()                 # listed although beyond the packable range (|block| >= 2^18)


@pytest.fixture(scope="module")
def oracle_map(pkg, O):
    Wd, Hd = 80, 60
    seq = pkg.synth.Sequence("spheres", Wd, Hd, n_frames=2, seed=1, step_deg=0.5)
    T = f32(5) * VS
    o = O.Oracle(VS, T, Wd, Hd, seq.K)
    for i in range(2):
        o.update(*seq.frame(i))
    keys, pay = o.export()                                           # dist, gx, gy, gz, weight
    packed = ref.pack(keys)
    order = np.argsort(packed)
    keys, pay, packed = keys[order], pay[order], packed[order]

    def get_voxels(k):
        pk = ref.pack(k)
        at = np.clip(np.searchsorted(packed, pk), 0, len(packed) - 1)
        found = packed[at] == pk
        return np.where(found[:, None], pay[at], 0).astype(f32), found
    return dict(o=o, keys=keys, pay=pay, T=T, get_voxels=get_voxels)


def test_restatement_identity_returns_the_source(O, oracle_map):
    """pose identity: every voxel of src receives from itself -- keys equal, w and the gradient sums in bits (up to the sign of a
    zero), s' = w * dist (tsdf() at a voxel centre is the stored dist)"""
    m = oracle_map
    pose = np.array([0, 0, 0, 0, 0, 0, 1], f32)
    box = ref.box_of(m["keys"], pose, VS, O)
    k, c = ref.contributions(m["o"].query, m["get_voxels"], pose, VS, m["T"], box, O)
    assert np.array_equal(k, m["keys"]) and len(k) > 1000
    assert np.array_equal(c[:, 4], m["pay"][:, 4]) and np.array_equal(c[:, 1:4], m["pay"][:, 1:4])
    assert np.array_equal(c[:, 0], (m["pay"][:, 4] * ref.truncate(m["pay"][:, 0], m["T"])).astype(f32))
    assert ref.n_blocks(k) == len(np.unique(k >> 2, axis=0))


def test_restatement_integer_shift_and_expected(O, oracle_map):
    """R = I, t = vs * (3, -5, 2): the keys shift by exactly that; expected() adds into an existing export once per key"""
    m = oracle_map
    shift = np.array([3, -5, 2], np.int32)
    pose = np.concatenate([(VS * shift.astype(f32)).astype(f32), [0, 0, 0, 1]]).astype(f32)
    box = ref.box_of(m["keys"], pose, VS, O)
    k, c = ref.contributions(m["o"].query, m["get_voxels"], pose, VS, m["T"], box, O)
    sk = m["keys"] + shift[None, :]
    assert np.array_equal(k, sk[np.argsort(ref.pack(sk))])
    raw = np.concatenate([(m["pay"][:, 4] * m["pay"][:, 0])[:, None], m["pay"][:, 1:4], m["pay"][:, 4:5]], 1).astype(f32)
    ek, ep, ck, cc = ref.expected((m["keys"], raw), m["o"].query, m["get_voxels"], pose, VS, m["T"], box, O)
    assert np.array_equal(ck, k) and len(ek) == len(np.union1d(ref.pack(m["keys"]), ref.pack(k)))
    both = np.isin(ref.pack(ek), ref.pack(m["keys"])) & np.isin(ref.pack(ek), ref.pack(k))
    assert both.any()
    at_old = np.searchsorted(ref.pack(m["keys"]), ref.pack(ek[both]))
    at_new = np.searchsorted(ref.pack(k), ref.pack(ek[both]))
    assert np.array_equal(ep[both], (raw[at_old] + c[at_new]).astype(f32))
