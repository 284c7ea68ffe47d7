/*
 * gsdf_posed.h -- the enumeration behind gsdf_merge_from_posed (gsdf_merge_posed.hip): which blocks of dst's grid can hold a
 * voxel that receives something from a given block of src under a pose.  Host and device; plain integers and doubles, so the
 * tests can call it without a device (gsdf_debug_posed_blocks of the test build).
 *
 * Voxel K of dst receives from voxel V of src when float2vox(q) == V for q = R^T (c_K - t), i.e. |q - c_V|inf <= vs / 2 up to
 * the float rounding of q and of float2vox.  In exact arithmetic c_K = A c_V' + t with A = (R^T)^-1 and |c_V' - c_V|2 <=
 * (sqrt(3) / 2) vs; every voxel of a block lies within 1.5 sqrt(3) vs of the block's centre b; so every receiver of the block
 * lies within rho * 2 sqrt(3) vs of A b + t, rho = the largest singular value of A.  A is the true inverse (inverted in double
 * on the host), not R: the quaternion is used as it comes, |q|^2 within 1e-4 of 1, and R = (1 - |q|^2) I + |q|^2 R^ then has
 * singular values within 2e-4 of 1 -- R c + t would drift from the kernel's preimage by 2e-4 of the coordinate, 0.2 voxels at
 * 1000 voxels from the origin.  rho <= 1.001 covers it.
 *
 * Float rounding, with u = 2^-24 and M the largest coordinate the kernel's arithmetic sees, in voxels (|c_K|, |t| / vs, |q|):
 * c = vs * (float)i is off by M u, d = c - t by another 2 M u, each component of q = R^T d by about 25 M u (three rounded
 * products of |d| <= 2 M, two sums, the propagated error of d), float2vox's inv_vs * q by about 10 M u: 35 M u per axis,
 * 61 M u in length.  The radius carries 128 M u = M * 2^-17 for it and a constant quarter of a voxel on top:
 *
 *     radius = 1.001 * 2 sqrt(3) + 0.25 + (M + 1) * 2^-17    voxels      (3.72 near the origin, 3.73 at 1000 voxels)
 *
 * A dst block is listed when the box of its 4^3 voxel centres comes within the radius of the image of the src block's centre:
 * 13 blocks on average near the origin.  Block indices are floor(voxel index / 4), signed; they are listed up to +-2^20
 * (voxels up to +-2^22), four times beyond the packable range, so that the sampling kernel can tell whether a key beyond the
 * range WOULD have received something (GSDF_ERR_KEY_RANGE); an image farther out than that is reported as `far`.
 */
#ifndef GSDF_POSED_H_
#define GSDF_POSED_H_

#include "gsdf_math.h"
#include "gsdf_table.h"

#define GSDF_POSED_WIDE_OFF   (1 << 20)      /* bias of a signed block index in a candidate key, 21 bits per axis */
#define GSDF_POSED_WIDE_MASK  0x1FFFFFull
#define GSDF_POSED_FAR        4194240.0      /* 2^22 - 64: an image beyond it (in voxels, any axis) is not enumerated */

/* src block centre (voxel units) -> its image in dst's voxel units: p = A b + tv */
struct gsdf_posed_map {
    double A[9];                 /* (R^T)^-1, row-major */
    double tv[3];                /* t / vs */
    double tmag;                 /* max |tv| */
};

GSDF_HD unsigned long long gsdf_posed_wide_pack(int X, int Y, int Z) {
    return (unsigned long long)(uint32_t)(X + GSDF_POSED_WIDE_OFF) | ((unsigned long long)(uint32_t)(Y + GSDF_POSED_WIDE_OFF) << 21) |
           ((unsigned long long)(uint32_t)(Z + GSDF_POSED_WIDE_OFF) << 42);
}
GSDF_HD void gsdf_posed_wide_unpack(unsigned long long k, int* X, int* Y, int* Z) {
    *X = (int)(k & GSDF_POSED_WIDE_MASK) - GSDF_POSED_WIDE_OFF;
    *Y = (int)((k >> 21) & GSDF_POSED_WIDE_MASK) - GSDF_POSED_WIDE_OFF;
    *Z = (int)((k >> 42) & GSDF_POSED_WIDE_MASK) - GSDF_POSED_WIDE_OFF;
}
/* a signed block index whose 4 voxels are packable */
GSDF_HD bool gsdf_posed_block_in_range(int X, int Y, int Z) {
    const int lim = GSDF_KEY_OFF >> 2;
    return X >= -lim && X < lim && Y >= -lim && Y < lim && Z >= -lim && Z < lim;
}
/* signed block index of a table's block key, and back (in range only) */
GSDF_HD void gsdf_posed_block_of_key(unsigned long long bk, int* X, int* Y, int* Z) {
    *X = (int)(bk & 0x7FFFFull) - (GSDF_KEY_OFF >> 2);
    *Y = (int)((bk >> 19) & 0x7FFFFull) - (GSDF_KEY_OFF >> 2);
    *Z = (int)((bk >> 38) & 0x7FFFFull) - (GSDF_KEY_OFF >> 2);
}
GSDF_HD unsigned long long gsdf_posed_key_of_block(int X, int Y, int Z) {
    return (unsigned long long)(uint32_t)(X + (GSDF_KEY_OFF >> 2)) | ((unsigned long long)(uint32_t)(Y + (GSDF_KEY_OFF >> 2)) << 19) |
           ((unsigned long long)(uint32_t)(Z + (GSDF_KEY_OFF >> 2)) << 38);
}

GSDF_HD double gsdf_posed_floor(double x) { const double t = (double)(long long)x; return t > x ? t - 1.0 : t; }

/* The dst blocks for src block (X, Y, Z): emit(Xd, Yd, Zd) once per block, in z-y-x order.  Returns their number, or -1 when the
 * image is not finite or beyond GSDF_POSED_FAR (`far`: nothing is emitted). */
template <class Emit>
GSDF_HD int gsdf_posed_blocks(const gsdf_posed_map& m, int X, int Y, int Z, Emit&& emit) {
    const double b[3] = { 4.0 * X + 1.5, 4.0 * Y + 1.5, 4.0 * Z + 1.5 };
    double p[3], mag = m.tmag;
    for (int a = 0; a < 3; ++a) {
        p[a] = m.A[3 * a] * b[0] + m.A[3 * a + 1] * b[1] + m.A[3 * a + 2] * b[2] + m.tv[a];
        if (!(p[a] > -GSDF_POSED_FAR && p[a] < GSDF_POSED_FAR)) return -1;          /* NaN fails both */
        const double ap = p[a] < 0 ? -p[a] : p[a], ab = b[a] < 0 ? -b[a] : b[a];
        mag = mag > ap ? mag : ap;
        mag = mag > ab ? mag : ab;
    }
    /* M: the image's, the source's and the translation's magnitude, and the reach of the ball itself */
    const double r = 1.001 * 3.4641016151377544 + 0.25 + (mag + 16.0 + 1.0) * (1.0 / 131072.0);
    int lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int)gsdf_posed_floor(gsdf_posed_floor(p[a] - r) * 0.25);
        hi[a] = (int)gsdf_posed_floor(gsdf_posed_floor(p[a] + r) * 0.25);
    }
    int n = 0;
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y)
            for (int x = lo[0]; x <= hi[0]; ++x) {
                const int c[3] = { x, y, z };
                double d2 = 0.0;
                for (int a = 0; a < 3; ++a) {                  /* distance to the box of the block's voxel centres, [4c, 4c + 3] */
                    const double l = 4.0 * c[a], h = l + 3.0;
                    const double d = p[a] < l ? l - p[a] : (p[a] > h ? p[a] - h : 0.0);
                    d2 += d * d;
                }
                if (d2 <= r * r) { emit(x, y, z); ++n; }
            }
    return n;
}

/* the map of a pose: R row-major as gsdf_quat_to_R gives it, t, voxel size.  false: R^T is singular (cannot happen for
 * | |q|^2 - 1 | <= 1e-4) */
inline bool gsdf_posed_map_make(const float R[9], const float t[3], float vs, gsdf_posed_map* m) {
    double B[9];                                               /* R^T */
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) B[3 * i + j] = (double)R[3 * j + i];
    const double c00 = B[4] * B[8] - B[5] * B[7], c01 = B[5] * B[6] - B[3] * B[8], c02 = B[3] * B[7] - B[4] * B[6];
    const double det = B[0] * c00 + B[1] * c01 + B[2] * c02;
    if (!(det > 0.5 && det < 2.0)) return false;
    const double id = 1.0 / det;
    m->A[0] = c00 * id; m->A[1] = (B[2] * B[7] - B[1] * B[8]) * id; m->A[2] = (B[1] * B[5] - B[2] * B[4]) * id;
    m->A[3] = c01 * id; m->A[4] = (B[0] * B[8] - B[2] * B[6]) * id; m->A[5] = (B[2] * B[3] - B[0] * B[5]) * id;
    m->A[6] = c02 * id; m->A[7] = (B[1] * B[6] - B[0] * B[7]) * id; m->A[8] = (B[0] * B[4] - B[1] * B[3]) * id;
    m->tmag = 0.0;
    for (int a = 0; a < 3; ++a) {
        m->tv[a] = (double)t[a] / (double)vs;
        const double at = m->tv[a] < 0 ? -m->tv[a] : m->tv[a];
        m->tmag = m->tmag > at ? m->tmag : at;
    }
    return true;
}

#endif /* GSDF_POSED_H_ */
