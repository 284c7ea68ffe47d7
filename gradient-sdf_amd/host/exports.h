/*
 * exports.h -- the file exports of MapGradPixelSdf (cpp/include/sdf_tracker/MapGradPixelSdf.cpp:124-296) over a gsdf_ctx:
 * mesh PLY (extract_mesh -> LayeredMarchingCubesNoColor), point-cloud PLY (extract_pc), sparse sdf text files (save_sdf).
 */
#ifndef GSDF_HOST_EXPORTS_H_
#define GSDF_HOST_EXPORTS_H_

#include <string>
#include <vector>

#include "../../include/gsdf.h"

namespace gsdf_exports {
/* extract_pc -- MapGradPixelSdf.cpp:177-220; *n_rows (nullable) = points written */
bool write_cloud_ply(gsdf_ctx* ctx, float voxel_size, const std::string& filename, long* n_rows);
/* extract_pc -- MapPixelSdf.cpp:242-277: voxel centres only (weight >= 5, |dist| < sqrt(3) vs) */
bool write_points_ply(gsdf_ctx* ctx, float voxel_size, const std::string& filename, long* n_rows);
/* save_sdf -- MapGradPixelSdf.cpp:222-296; normals = false: MapPixelSdf.cpp:285-347 (no _sdf_n* files) */
bool write_sdf_txt(gsdf_ctx* ctx, float voxel_size, const std::string& filename, bool normals = true);
/* extract_mesh -- MapGradPixelSdf.cpp:124-175, marching cubes on the device; *n_faces (nullable) = faces written */
bool write_mesh_ply(gsdf_ctx* ctx, float voxel_size, const std::string& filename, long* n_faces);
/* the same surface as an indexed mesh with gradient normals (gsdf_extract_mesh_indexed; not in the reference), binary PLY
 * (MarchingCubes::saveIndexedPly); *n_vertices / *n_faces (nullable) = what was written.  false for an empty mesh, like write_mesh_ply */
bool write_indexed_mesh_ply(gsdf_ctx* ctx, const std::string& filename, long* n_vertices, long* n_faces);
/* that mesh without its small components (gsdf_extract_mesh_indexed_filtered: min_faces >= 1, or GSDF_MESH_KEEP_LARGEST), binary
 * PLY; nullable: *n_components / *n_kept = components found / kept, *n_faces / *n_faces_all = faces written / of the whole mesh.
 * false for a mesh that keeps no face */
bool write_filtered_mesh_ply(gsdf_ctx* ctx, const std::string& filename, int64_t min_faces, long* n_components, long* n_kept,
                             long* n_faces, long* n_faces_all);
/* the component table of the indexed mesh (gsdf_mesh_components) as text: one row `id faces vertices minx miny minz maxx maxy maxz`
 * per component behind a `#` line; *n_components (nullable) = rows written */
bool write_mesh_components_txt(gsdf_ctx* ctx, const std::string& filename, long* n_components);
/* the thresholds of matlab/GradientAnalysisSpheres.m:155, d = 0.001 : 0.001 : trunc_dist, as floats; the count forgives the
 * float rounding of trunc_dist by a thousandth of a step (5 voxels of 0.02 m are 0.099999994: 100 thresholds) */
std::vector<float> gradient_ladder(float trunc_dist);
/* the gradient-accuracy table (gsdf_gradient_stats; matlab/phi_statistics.m) as text: one block per estimator (stored,
 * central, forward, backward) behind a `# estimator` line, rows `d count mean median rmse p95`; spheres4 = rows cx cy cz R */
bool write_gradient_stats_txt(gsdf_ctx* ctx, const std::vector<float>& spheres4, const std::vector<float>& thresholds,
                              const std::string& filename);
}

#endif
