/*
 * gsdf_sample.h -- MapGradPixelSdf::weights + ::tsdf at ONE point (MapGradPixelSdf.h:109-125) on the device: the body of
 * k_query (gsdf_kernels.hip), moved here unchanged so that the point registration (k_align_pass, gsdf_align.hip) evaluates
 * exactly what gsdf_query returns -- one definition, two callers.
 */
#ifndef GSDF_SAMPLE_H_
#define GSDF_SAMPLE_H_

#include "gsdf_math.h"
#include "gsdf_table.h"

#if defined(__HIPCC__)
/* w = 0 marks a missing voxel (no block, beyond the key range, or weight 0): phi and g are then 0.
 * Otherwise g = 1.2f * normalized(grad sum) (:113) and phi = the return expression of :114. */
__device__ __forceinline__ void gsdf_grad_sample(const gsdf_table& tab, float vs, float inv_vs, gsdf_v3 p, float& ow, float& od,
                                                 gsdf_v3& og) {
    const int vx = gsdf_float2vox1(inv_vs, p.x), vy = gsdf_float2vox1(inv_vs, p.y), vz = gsdf_float2vox1(inv_vs, p.z);
    ow = 0.f; od = 0.f;
    og = gsdf_v3{ 0.f, 0.f, 0.f };
    if (gsdf_key_in_range(vx, vy, vz)) {
        const gsdf_payload* sl = gsdf_find(tab, gsdf_key_pack(vx, vy, vz));
        if (sl && sl->w > 0.f) {
            ow = sl->w;
            const gsdf_v3 gn = gsdf_normalized3(gsdf_v3{ sl->gx, sl->gy, sl->gz });
            og = gsdf_v3{ 1.2f * gn.x, 1.2f * gn.y, 1.2f * gn.z };
            const gsdf_v3 d = { vs * (float)vx - p.x, vs * (float)vy - p.y, vs * (float)vz - p.z };
            od = gsdf_tsdf_phi(sl->s / sl->w, gn, d);                                  /* :114 */
        }
    }
}
#endif

#endif /* GSDF_SAMPLE_H_ */
