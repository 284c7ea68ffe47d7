"""The gradient-accuracy analysis (gsdf_gradient_angles / gsdf_gradient_stats, include/gsdf.h) restated in numpy: the MATLAB
scripts matlab/GradientAnalysisSpheres.m and matlab/phi_statistics.m on a sorted export instead of save_sdf's text files.

The map goes into a dense box (the bounding box of the existing voxels, :48-50) filled with trunc_dist (:55); central differences
are np.gradient -- MATLAB's gradient(D, vs): one-sided on the box's faces -- with 0 written explicitly where the box is one voxel
thick (np.gradient refuses that extent); percentiles are np.percentile(method="hazen"), MATLAB's prctile.  All arithmetic in
float64 on the float32 values of the export, the angles rounded to float32 at the end, as the header states it.
"""
import numpy as np

f32 = np.float32
STAT_NAMES = ("count", "mean", "median", "rmse", "p95")
ESTIMATORS = ("stored", "central", "forward", "backward")


def _normalized(v):
    """rows of v over their norm; NaN rows where the norm is 0 or not finite"""
    with np.errstate(all="ignore"):
        n2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        bad = ~(n2 > 0) | ~np.isfinite(n2)
        out = v / np.sqrt(n2)[:, None]
    out[bad] = np.nan
    return out


def ground_truth(keys, spheres, vs):
    """unit vector from the centre of the sphere maximising R - |c - centre| (the first among equals) to the voxel centre
    c = vs * (float)idx, a float32 product widened to float64 (:96-111)"""
    sp = np.asarray(spheres, f32).reshape(-1, 4).astype(np.float64)
    c = (f32(vs) * np.asarray(keys).astype(f32)).astype(np.float64)
    d = c[:, None, :] - sp[None, :, :3]
    m = sp[None, :, 3] - np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    which = np.argmax(m, axis=1)
    return _normalized(d[np.arange(len(c)), which])


def estimators(keys, payload, vs, trunc_dist):
    """the four direction fields of the existing voxels, float64 [4, n, 3], not normalised: stored sum, central, forward and
    backward differences of D over the dense bounding box"""
    keys = np.asarray(keys, np.int64)
    pay = np.asarray(payload, f32)
    n = len(keys)
    mn, mx = keys.min(0), keys.max(0)
    sz = mx - mn + 1
    D = np.full(sz, np.float64(f32(trunc_dist)))
    ix = tuple((keys - mn).T)
    D[ix] = pay[:, 0].astype(np.float64)
    h = np.float64(f32(vs))
    vs_inv = 1.0 / h
    out = np.zeros((4, n, 3))
    out[0] = pay[:, 1:4].astype(np.float64)
    for ax in range(3):
        if sz[ax] >= 2:
            out[1, :, ax] = np.gradient(D, h, axis=ax)[ix]
            diff = vs_inv * np.diff(D, axis=ax)
            zero = np.zeros([1 if a == ax else sz[a] for a in range(3)])
            out[2, :, ax] = np.concatenate([diff, zero], axis=ax)[ix]       # :117-124
            out[3, :, ax] = np.concatenate([zero, diff], axis=ax)[ix]       # :136-143
    return out


def angles(keys, payload, spheres, vs, trunc_dist):
    """rows float32 [n, 5]: dist, phi of the four estimators in degrees (NaN = undefined), in the order of `keys`"""
    keys = np.asarray(keys)
    pay = np.asarray(payload, f32)
    rows = np.empty((len(keys), 5), f32)
    rows[:, 0] = pay[:, 0]
    if len(keys) == 0:
        return rows
    g = ground_truth(keys, spheres, vs)
    est = estimators(keys, pay, vs, trunc_dist)
    with np.errstate(all="ignore"):
        for e in range(4):
            u = _normalized(est[e])
            cos = np.abs((u[:, 0] * g[:, 0] + u[:, 1] * g[:, 1]) + u[:, 2] * g[:, 2])
            phi = np.arccos(np.where(cos < 1.0, cos, 1.0)) * (180.0 / np.pi)
            phi[np.isnan(cos)] = np.nan
            rows[:, 1 + e] = phi.astype(f32)
    return rows


def stats(rows, thresholds):
    """float64 [4, n_thr, 5] = count, mean, median, rmse, p95 over fabsf(dist) < d[k] (a float32 compare) and phi not NaN
    (phi_statistics.m:69-73); an empty subset: count 0, NaN for the rest"""
    thr = np.asarray(thresholds, f32).reshape(-1)
    out = np.full((4, len(thr), 5), np.nan)
    out[:, :, 0] = 0
    ad = np.abs(np.asarray(rows, f32)[:, 0])
    for e in range(4):
        phi32 = np.asarray(rows, f32)[:, 1 + e]
        for k, d in enumerate(thr):
            sel = (ad < d) & ~np.isnan(phi32)
            x = phi32[sel].astype(np.float64)
            if len(x) == 0:
                continue
            med, p95 = np.percentile(x, [50, 95], method="hazen")
            out[e, k] = (len(x), x.mean(), med, np.sqrt((x * x).mean()), p95)
    return out


def ladder(trunc_dist):
    """the script's thresholds d = 0.001 : 0.001 : vs*T (:155) as float32; the count forgives the float32 rounding of trunc_dist
    (a thousandth of a step), as Scan3D --gradient-analysis counts them"""
    n = int(np.floor(np.float64(f32(trunc_dist)) / 0.001 + 1e-3))
    return (np.arange(1, n + 1) * 0.001).astype(f32)


def sphere_map(radius_vox, centre_vox, vs, trunc_dist, band_vox):
    """an analytic sphere as a map: the voxels within band_vox voxels of the surface, dist = clamp(R - |c|, +-trunc_dist)
    (positive inside, as ground_truth's maximised quantity), gradient sum radial (outwards; the angle takes |cos|), w = 1.
    The sphere row for the ground truth is returned beside it.  Keys come out in gsdf_export's sorted order (z, y, x)."""
    vs = f32(vs)
    ctr = (np.asarray(centre_vox, np.float64) * float(vs)).astype(f32).astype(np.float64)      # the float32 row, widened
    R = float(f32(float(radius_vox) * float(vs)))
    r = int(np.ceil(radius_vox + band_vox)) + 1
    lo = np.floor(np.asarray(centre_vox)).astype(int) - r
    ax = [np.arange(lo[a], lo[a] + 2 * r + 2) for a in range(3)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    keys = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.int32)
    c = (vs * keys.astype(f32)).astype(np.float64)
    d = c - ctr
    rho = np.linalg.norm(d, axis=1)
    keep = np.abs(R - rho) < band_vox * float(vs)
    keys, d, rho = keys[keep], d[keep], rho[keep]
    pay = np.zeros((len(keys), 5), f32)
    pay[:, 0] = np.clip(R - rho, -float(f32(trunc_dist)), float(f32(trunc_dist))).astype(f32)
    pay[:, 1:4] = (d / rho[:, None]).astype(f32)
    pay[:, 4] = 1
    sphere = np.array([[ctr[0], ctr[1], ctr[2], R]], f32)
    return keys, pay, sphere
