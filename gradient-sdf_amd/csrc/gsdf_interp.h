/*
 * gsdf_interp.h -- interpolateImage of the reference's photometric code (PhotometricOptimizer.cpp:57-77) over a float BGR
 * keyframe image on the device.  ColorUpsampler.cpp:57-82 is the same function plus a branch for rows >= img.rows, which its
 * callers never reach (they sample only inside [0,W) x [0,H)).  Shared by the PhotoBA sweeps (gsdf_ba.hip) and the colour pass
 * (gsdf_color.hip): one definition, moved here unchanged.
 */
#ifndef GSDF_INTERP_H_
#define GSDF_INTERP_H_

#include "gsdf_math.h"

#include <hip/hip_runtime.h>

struct ba_img { int W, H; const float* p; };
__device__ __forceinline__ const float* ba_px(const ba_img& im, int row, int col) { return im.p + ((size_t)row * im.W + col) * 3; }

/* interpolateImage(m = row, n = col) -- :57-77 (weights in double, BGR -> RGB) */
__device__ __forceinline__ gsdf_v3 ba_interp(float m, float n, const ba_img& im) {
    const int x = (int)floorf(m), y = (int)floorf(n);
    float t[3];
    if ((x + 1) < im.H && (y + 1) < im.W) {
        const double w1 = (y + 1.0 - n) * (m - x), w2 = (y + 1.0 - n) * (x + 1.0 - m), w3 = (n - y) * (m - x), w4 = (n - y) * (x + 1.0 - m);
        const float *a = ba_px(im, x + 1, y), *b = ba_px(im, x, y), *c = ba_px(im, x + 1, y + 1), *d = ba_px(im, x, y + 1);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            t[k] = (((float)(w1 * (double)a[k]) + (float)(w2 * (double)b[k])) + (float)(w3 * (double)c[k])) + (float)(w4 * (double)d[k]);
    } else if (y >= im.W && (x + 1) < im.H) {
        const int yc = min(y, im.W - 1);
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = (float)((double)(m - x) * (double)ba_px(im, x + 1, yc)[k]) + (float)((x + 1.0 - m) * (double)ba_px(im, x, yc)[k]);
    } else {
        const float* a = ba_px(im, min(x, im.H - 1), min(y, im.W - 1));
        t[0] = a[0]; t[1] = a[1]; t[2] = a[2];
    }
    return gsdf_v3{ t[2], t[1], t[0] };
}

#endif /* GSDF_INTERP_H_ */
