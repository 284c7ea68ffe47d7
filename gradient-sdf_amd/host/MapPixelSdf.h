/*
 * MapPixelSdf -- the plain voxel-hash SDF of the reference (cpp/include/sdf_tracker/MapPixelSdf.h:52-157), the baseline the
 * Gradient-SDF paper compares against (--scan-type base-sdf), as a facade over the C-ABI: a gsdf_ctx of type GSDF_MAP_BASE.
 *
 * The map is fused exactly as MapGradPixelSdf's (MapPixelSdfOmp.cpp:163-186 visits the same voxels with the same weight,
 * truncation and running mean as MapGradPixelSdf.cpp:86-118), so the context handling, update(), the frame entries and the
 * mesh are MapGradPixelSdf's; tsdf() / weights() are interp3 (MapPixelSdf.cpp:43-111) on the device, and the text exports
 * have no gradient.  RigidPointOptimizer works on either map through Sdf*.
 */
#ifndef GSDF_HOST_MAP_PIXEL_SDF_H_
#define GSDF_HOST_MAP_PIXEL_SDF_H_

#include "MapGradPixelSdf.h"

class MapPixelSdf : public MapGradPixelSdf {
public:
    /* MapPixelSdf(voxel_size) / MapPixelSdf(voxel_size, T) -- MapPixelSdf.h:86-100 (T defaults to Sdf()'s 0.05, Sdf.h:97-98);
     * capacity/device as MapGradPixelSdf's */
    explicit MapPixelSdf(float voxel_size, float T = 0.05f, int capacity_log2 = 22, int device = 0, int max_capacity_log2 = 28)
        : MapGradPixelSdf(GSDF_MAP_BASE, voxel_size, T, capacity_log2, device, max_capacity_log2) {}

    float tsdf(Vec3f point, Vec3f* grad_ptr) const override;          /* MapPixelSdf.h:108-116 */
    float weights(Vec3f point) const override;                         /* MapPixelSdf.h:118-143 */

    bool extract_pc(std::string filename) override;                    /* MapPixelSdf.cpp:242-277 */
    bool save_sdf(std::string filename) override;                      /* MapPixelSdf.cpp:285-347 */
    /* extract_mesh, extract_mesh_indexed (plain and filtered), mesh_components and gradient_analysis: MapGradPixelSdf's (MapPixelSdf.cpp:192-240 runs the same marching
     * cubes over the same dist values; the fusion stores the same gradient sums).
     * select_box / select_weight / select_points / select_invert / select_clear / select_count / select_export, erase_selected,
     * compact, crop and prune: MapGradPixelSdf's as well (the selection reads keys and weights, which both map types store alike) */
};

#endif
