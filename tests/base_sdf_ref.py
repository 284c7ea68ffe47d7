"""MapPixelSdf (the plain-SDF baseline, --scan-type base-sdf) restated in numpy float32, operation for operation, for the tests
of the base map type (tests/test_base_sdf.py, tests/test_gpu_base_sdf.py).

The map is given as arrays (keys int32 [n,3], dist float32 [n], weight float32 [n]) -- what gsdf_export or the oracle's export()
return: MapPixelSdf::update fuses the same voxels with the same weight / truncation / running mean as MapGradPixelSdf::update
(MapPixelSdfOmp.cpp:163-186 = MapGradPixelSdf.cpp:86-118), so the oracle's update() builds a base map too.  Corner lookups are a
searchsorted over the sorted packed keys.  The 6x6 solve and the pose update are the oracle's (oracle/oracle.py: llt_solve6,
se3_exp_mul).

Line numbers refer to cpp/include/sdf_tracker/MapPixelSdf.h / MapPixelSdf.cpp and RigidPointOptimizer.cpp of the reference."""
import numpy as np

f32 = np.float32
_OFF = 1 << 20


def _pack(x, y, z):
    """the engine's packed voxel key (21 bits per axis, x low): orders like (z, y, x)"""
    return ((x.astype(np.int64) + _OFF) | ((y.astype(np.int64) + _OFF) << 21) | ((z.astype(np.int64) + _OFF) << 42))


def _in_range(v):
    return (v >= -_OFF) & (v < _OFF)


class BaseMap:
    """tsdf_ of a MapPixelSdf as sorted arrays."""

    def __init__(self, keys, dist, weight, voxel_size, T):
        keys = np.asarray(keys, np.int32).reshape(-1, 3)
        pk = _pack(keys[:, 0], keys[:, 1], keys[:, 2])
        order = np.argsort(pk, kind="stable")
        self.pk = pk[order]
        self.dist = np.asarray(dist, f32).reshape(-1)[order]
        self.weight = np.asarray(weight, f32).reshape(-1)[order]
        self.vs = f32(voxel_size)
        self.inv_vs = f32(1.0 / float(self.vs))            # voxel_size_inv_(1./voxel_size_), MapPixelSdf.h:90
        self.T = f32(T)

    @classmethod
    def from_export(cls, keys, payload, voxel_size, T):
        """keys [n,3] and payload [n,5] = (dist, gx, gy, gz, weight) of gsdf_export / Oracle.export"""
        payload = np.asarray(payload, f32).reshape(-1, 5)
        return cls(keys, payload[:, 0], payload[:, 4], voxel_size, T)

    def _find(self, x, y, z):
        """tsdf_.find(Vec3i(x, y, z)): (found, index)"""
        ok = _in_range(x) & _in_range(y) & _in_range(z)
        k = _pack(np.where(ok, x, 0), np.where(ok, y, 0), np.where(ok, z, 0))
        if len(self.pk) == 0:
            return np.zeros(x.shape, bool), np.zeros(x.shape, np.int64)
        ic = np.minimum(np.searchsorted(self.pk, k), len(self.pk) - 1)
        return ok & (self.pk[ic] == k), ic

    def sample(self, pts):
        """weights() and tsdf() at the points [n,3]: (w [n], phi [n], grad [n,3])"""
        p = np.asarray(pts, f32).reshape(-1, 3)
        pv = self.inv_vs * p                                  # MapPixelSdf.cpp:44  (float * Vec3f)
        i, j, k = pv[:, 0], pv[:, 1], pv[:, 2]                # :45
        im = np.floor(i).astype(np.int64)                     # :48-50  (int)std::floor
        jm = np.floor(j).astype(np.int64)
        km = np.floor(k).astype(np.int64)
        dx = (i - im.astype(f32)).astype(f32)                 # :53-55
        dy = (j - jm.astype(f32)).astype(f32)
        dz = (k - km.astype(f32)).astype(f32)
        n = p.shape[0]
        d = np.full((8, n), -self.T, f32)                     # :58  extrap * Ones, extrap = -T_ (MapPixelSdf.h:111)
        wv = np.zeros((8, n), f32)
        present = np.zeros((8, n), bool)
        for k0 in range(2):                                   # :60-69  corner i0 + 2 j0 + 4 k0
            for j0 in range(2):
                for i0 in range(2):
                    c = i0 + 2 * j0 + 4 * k0
                    found, idx = self._find(im + i0, jm + j0, km + k0)
                    present[c] = found
                    if len(self.pk):
                        d[c] = np.where(found, self.dist[idx], d[c])
                        wv[c] = np.where(found, self.weight[idx], f32(0))
        none = ~present.any(0)
        full = present.all(0)
        one = f32(1)
        # :74-103, in its operation order (numpy float32: every operation rounds once, no fma)
        d01 = (one - dx) * d[0] + dx * d[1]
        d23 = (one - dx) * d[2] + dx * d[3]
        d45 = (one - dx) * d[4] + dx * d[5]
        d67 = (one - dx) * d[6] + dx * d[7]
        d02 = (one - dy) * d[0] + dy * d[2]
        d13 = (one - dy) * d[1] + dy * d[3]
        d46 = (one - dy) * d[4] + dy * d[6]
        d57 = (one - dy) * d[5] + dy * d[7]
        gx = self.inv_vs * ((one - dz) * d13 + dz * d57 - (one - dz) * d02 - dz * d46)
        gy = self.inv_vs * ((one - dz) * d23 + dz * d67 - (one - dz) * d01 - dz * d45)
        gz = self.inv_vs * ((one - dy) * d45 + dy * d67 - (one - dy) * d01 - dy * d23)
        dy0 = (one - dy) * d01 + dy * d23
        dy1 = (one - dy) * d45 + dy * d67
        phi = (one - dz) * dy0 + dz * dy1
        phi = np.where(full, phi, np.where(none, -self.T, f32(0))).astype(f32)   # :71-72 extrap, :106 0.0
        grad = np.where(full[:, None], np.stack([gx, gy, gz], 1), f32(0)).astype(f32)
        # weights(): MapPixelSdf.h:118-143 -- all 8 floor corners, then the weight of float2vox(point) = std::round(pv) (:69-72)
        rc = ((_round(i) != im).astype(np.int64) + 2 * (_round(j) != jm).astype(np.int64)
              + 4 * (_round(k) != km).astype(np.int64))
        w = np.where(full, wv[rc, np.arange(n)], f32(0)).astype(f32)
        return w, phi, grad


def _round(x):
    """std::round (half away from zero) of float32 values, as int64"""
    x = np.asarray(x, f32)
    return (np.sign(x) * np.floor(np.abs(x).astype(np.float64) + 0.5)).astype(np.int64)


def _sum3(a, b, c):
    return a + (b + c)


def optimize_sampled(O, m, depth, K, pose7, iters=25, conv=1e-3, damping=1.0, sampling=1, zmin=0.5, zmax=3.5):
    """RigidPointOptimizer::optimize_sampled on a MapPixelSdf (RigidPointOptimizer.cpp:40-99), O = oracle/oracle.py.
    Returns (converged, pose7, passes, trace [passes, 36] like Oracle.track's: E, g[6], H upper[21], hits, xi[6], |xi|^2)."""
    depth = np.asarray(depth, f32)
    K = np.asarray(K, f32).reshape(9)
    h, w = depth.shape
    ys, xs = np.meshgrid(np.arange(0, h, sampling), np.arange(0, w, sampling), indexing="ij")   # :62
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    z = depth[ys, xs]
    ok = ~((z <= f32(zmin)) | (z >= f32(zmax)))                                                # :64-65
    xs, ys, z = xs[ok], ys[ok], z[ok]
    fx_inv, fy_inv = f32(1) / K[0], f32(1) / K[4]                                               # :46-47
    x0 = (xs.astype(f32) - K[2]) * fx_inv                                                       # :67-68
    y0 = (ys.astype(f32) - K[5]) * fy_inv
    pc = np.stack([x0 * z, y0 * z, z], 1)
    pose = np.asarray(pose7, f32).reshape(7).copy()
    conv_sq = f32(conv) * f32(conv)
    trace = []
    for k in range(iters):                                                                      # :51
        R = O.quat_to_R(pose[3:]).reshape(9)                                                    # :53
        p = np.stack([_sum3(R[3 * r] * pc[:, 0], R[3 * r + 1] * pc[:, 1], R[3 * r + 2] * pc[:, 2]) + pose[r]
                      for r in range(3)], 1).astype(f32)                                        # :70
        w0, phi, gr = m.sample(p)                                                               # :72, :75
        hit = w0 > 0
        phi, gr, p = phi[hit], gr[hit], p[hit]
        pxg = np.stack([p[:, 1] * gr[:, 2] - p[:, 2] * gr[:, 1], p[:, 2] * gr[:, 0] - p[:, 0] * gr[:, 2],
                        p[:, 0] * gr[:, 1] - p[:, 1] * gr[:, 0]], 1)                            # :78
        J = np.concatenate([gr, pxg], 1).astype(np.float64)
        ph = phi.astype(np.float64)
        E = f32((ph * ph).sum())                                                                # :76
        g = (ph[:, None] * J).sum(0).astype(f32)                                                # :79
        H = (J.T @ J).astype(f32)                                                               # :80
        xi = (f32(damping) * O.llt_solve6(H, g)).astype(f32)                                    # :86
        sq = xi * xi
        nrm = _sum3(sq[0], sq[1], sq[2]) + _sum3(sq[3], sq[4], sq[5])
        row = np.zeros(36, f32)
        row[0] = E
        row[1:7] = g
        row[7:28] = H[np.triu_indices(6)]
        row[28] = hit.sum()
        row[29:35] = xi
        row[35] = nrm
        trace.append(row)
        if nrm < conv_sq:                                                                       # :88-91
            return True, pose, k + 1, np.array(trace)
        if not np.isnan(xi).any():
            pose = O.se3_exp_mul(-xi, pose)                                                     # :94-95
    return False, pose, iters, np.array(trace)
