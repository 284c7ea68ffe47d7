/* MapPixelSdf facade: the queries forward to gsdf_query on a GSDF_MAP_BASE context (include/gsdf.h). */
#include "MapPixelSdf.h"

#include "exports.h"

float MapPixelSdf::weights(Vec3f point) const {
    float d, g[3], w;
    query1(point, &d, g, &w);
    return w;
}

float MapPixelSdf::tsdf(Vec3f point, Vec3f* grad_ptr) const {
    float d, g[3], w;
    query1(point, &d, g, &w);                                          /* interp3(point, -T_, grad) */
    if (grad_ptr) *grad_ptr = Vec3f(g[0], g[1], g[2]);
    return d;
}

bool MapPixelSdf::extract_pc(std::string filename) { return gsdf_exports::write_points_ply(handle(), voxel_size(), filename, nullptr); }
bool MapPixelSdf::save_sdf(std::string filename) { return gsdf_exports::write_sdf_txt(handle(), voxel_size(), filename, false); }
