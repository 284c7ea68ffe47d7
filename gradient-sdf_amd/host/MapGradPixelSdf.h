/*
 * MapGradPixelSdf -- the Gradient-SDF voxel hash map of the reference
 * (cpp/include/sdf_tracker/MapGradPixelSdf.h:51-151) as a facade over the C-ABI: the map lives in
 * HBM inside a gsdf_ctx, every method is one include/gsdf.h call.
 */
#ifndef GSDF_HOST_MAP_GRAD_PIXEL_SDF_H_
#define GSDF_HOST_MAP_GRAD_PIXEL_SDF_H_

#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gsdf.h"
#include "Sdf.h"
#include "SdfVoxel.h"

class RigidPointOptimizer;

class MapGradPixelSdf : public Sdf {
    friend class RigidPointOptimizer;            /* like Sdf.h:58 */
    gsdf_ctx* ctx_ = nullptr;
    float voxel_size_, T_;
    int frame_w_ = 0, frame_h_ = 0;
    void ensure_frame(const DepthImage& depth, const Mat3f& K, NormalEstimator* NEst);
    void check(int rc, const char* what) const;

public:
    /* MapGradPixelSdf(voxel_size, T) -- MapGradPixelSdf.h:99-103; capacity/device are new */
    /* capacity_log2: 2^c voxel records to start with; the table doubles by itself as the map grows, up to 2^max_capacity_log2
     * (8 GiB of records at 28; pass max == capacity for a fixed table, which then reports GSDF_ERR_TABLE_FULL when it overflows) */
    MapGradPixelSdf(float voxel_size, float T, int capacity_log2 = 22, int device = 0, int max_capacity_log2 = 28);
    ~MapGradPixelSdf() override;
    MapGradPixelSdf(const MapGradPixelSdf&) = delete;
    MapGradPixelSdf& operator=(const MapGradPixelSdf&) = delete;

    float tsdf(Vec3f point, Vec3f* grad_ptr) const override;          /* MapGradPixelSdf.h:109-115 */
    float weights(Vec3f point) const override;                         /* MapGradPixelSdf.h:117-125 */
    SdfVoxel getSdf(Vec3i idx) const;                                  /* MapGradPixelSdf.h:127-129 */
    void update(const ColorImage& color, const DepthImage& depth, const Mat3f K, const SE3& pose,
                NormalEstimator* NEst) override;                       /* MapGradPixelSdf.cpp:43-122 */
    void set_zmin(float z_min) override { zmin_ = z_min; gsdf_set_zrange(ctx_, zmin_, zmax_); }
    void set_zmax(float z_max) override { zmax_ = z_max; gsdf_set_zrange(ctx_, zmin_, zmax_); }

    SdfLrMap get_tsdf() const;                                         /* MapGradPixelSdf.h:133-138 (by value) */
    /* vis_ (MapGradPixelSdf.h:70,140-142): opt-in here, call before the first update() */
    void enable_vis(int max_frames) { check(gsdf_enable_vis(ctx_, max_frames), "gsdf_enable_vis"); }
    /* sorted (z,y,x) arrays: keys int32[n][3], payload float[n][5] = dist,gx,gy,gz,weight */
    void export_arrays(std::vector<int32_t>& keys, std::vector<float>& payload) const;
    int64_t size() const;
    int64_t frame_counter() const;

    /* voxel-hash raycaster (BASELINE.json north_star; the reference has none): depth (camera z, 0 = no hit)
     * and camera-frame normals (3 planes, may be null) of the map seen from `pose` through K */
    void raycast(const Mat3f& K, const SE3& pose, int W, int H, float* depth_out, float* normals_out) const;

    bool extract_pc(std::string filename) override;                    /* MapGradPixelSdf.cpp:177-220 */
    /* extract_pc's rows (MapGradPixelSdf.cpp:182-195) in memory: x y z nx ny nz per row, (z, y, x) key order (gsdf_surface_cloud);
     * false on a MapPixelSdf or an error (gsdf_last_error) */
    bool surface_cloud(std::vector<float>& rows6) const;
    /* this += other resampled on this map's grid under `pose` (other's frame -> this map's: what
     * RigidPointOptimizer::optimize_points leaves in pose() after registering other's surface_cloud against this map):
     * gsdf_merge_from_posed, not in the reference.  Nullable: voxels that received a contribution, blocks they lie in.  false
     * when the library refuses (a MapPixelSdf on either side, enable_vis, different voxel size or truncation, no room) or reports
     * keys beyond the packable range (the rest is merged then); gsdf_last_error says which */
    bool merge_from(const MapGradPixelSdf& other, const SE3& pose, int64_t* n_voxels = nullptr, int64_t* n_blocks = nullptr);
    /* Removing voxels (include/gsdf.h, "REMOVING VOXELS"; not in the reference, whose map only grows): the context's one
     * selection -- select_box (closed box of voxel centres), select_weight (w_min <= w < w_max), select_points (centres within
     * radius of a point; pose, nullable, moves the points first), each combined by op = GSDF_SEL_REPLACE / ADD / INTERSECT /
     * SUBTRACT, select_invert, select_clear --, its consumers select_count and select_export (sorted (z, y, x), payload as
     * export_arrays or raw sums), erase_selected (member records zeroed, block keys stay) and compact (the table rebuilt without
     * its empty blocks; 0 keeps the capacity).  crop = box, invert, erase, compact; prune = weight [0, min_weight), erase,
     * compact.  Nullable counts as in the C entries.  false when the library refuses (gsdf_last_error says why: a lost
     * selection after the table grew, a NaN bound, a radius beyond 16 voxels, no room for compact).  MapPixelSdf inherits them */
    bool select_box(const Vec3f& lo, const Vec3f& hi, int op = GSDF_SEL_REPLACE, int64_t* n = nullptr);
    bool select_weight(float w_min, float w_max, int op = GSDF_SEL_REPLACE, int64_t* n = nullptr);
    bool select_points(const std::vector<float>& pts3, float radius, const SE3* pose = nullptr, int op = GSDF_SEL_REPLACE, int64_t* n = nullptr);
    bool select_invert(int64_t* n = nullptr);
    bool select_clear();
    bool select_count(int64_t* n_voxels, int64_t* n_blocks = nullptr) const;
    bool select_export(std::vector<int32_t>& keys, std::vector<float>& payload, bool raw_sums = false) const;
    bool erase_selected(int64_t* n_voxels = nullptr, int64_t* n_blocks_emptied = nullptr);
    bool compact(int new_capacity_log2 = 0, int64_t* n_blocks_dropped = nullptr);
    bool crop(const Vec3f& lo, const Vec3f& hi);
    bool prune(float min_weight);
    bool save_sdf(std::string filename) override;                      /* MapGradPixelSdf.cpp:222-296 */
    bool extract_mesh(std::string filename) override;                  /* MapGradPixelSdf.cpp:124-175 */
    /* the same surface as an indexed mesh with a gradient normal per vertex, binary PLY (gsdf_extract_mesh_indexed; not in the
     * reference).  MapPixelSdf inherits it: a base context stores the same gradient sums */
    bool extract_mesh_indexed(std::string filename);
    /* ... without its small connected components (gsdf_extract_mesh_indexed_filtered): min_faces >= 1 keeps the components of at
     * least that many faces, GSDF_MESH_KEEP_LARGEST the largest alone.  Nullable: components found / kept, faces written / of the
     * whole mesh.  false when no face is kept or the file cannot be written */
    bool extract_mesh_indexed(std::string filename, int64_t min_faces, long* n_components = nullptr, long* n_kept = nullptr,
                              long* n_faces = nullptr, long* n_faces_all = nullptr);
    /* the components of the indexed mesh (gsdf_mesh_components): an id per vertex and per face, per component faces / vertices
     * and the box min x y z, max x y z.  false when the library refuses */
    struct MeshComponents {
        std::vector<int32_t> vertex_comp, face_comp, counts;             /* counts: 2 per component */
        std::vector<float> bbox;                                         /* 6 per component */
        int64_t n_components = 0;
    };
    bool mesh_components(MeshComponents& out) const;
    /* ... its table written as text (gsdf_exports::write_mesh_components_txt) */
    bool save_mesh_components(std::string filename) const;
    /* the gradient-accuracy table of a sphere scene (gsdf_gradient_stats; matlab/GradientAnalysisSpheres.m, phi_statistics.m):
     * spheres4 = rows cx cy cz R, thresholds ascending; stats = [4 estimators][thresholds][count, mean, median, rmse, p95].
     * false when the library refuses the arguments.  MapPixelSdf inherits it */
    bool gradient_analysis(const std::vector<float>& spheres4, const std::vector<float>& thresholds, std::vector<double>& stats) const;
    /* ... written as text (gsdf_exports::write_gradient_stats_txt) */
    bool save_gradient_analysis(const std::vector<float>& spheres4, const std::vector<float>& thresholds, std::string filename) const;

    /* fix the frame size / intrinsics / normal-estimator window before driving the *_dev entries directly (update() does
     * it on the first frame) */
    void prepare(int W, int H, const Mat3f& K, NormalEstimator* NEst);
    gsdf_ctx* handle() const { return ctx_; }
    float voxel_size() const { return voxel_size_; }
    float trunc_dist() const { return T_; }

protected:
    /* a context of another map type (gsdf_set_map_type): MapPixelSdf */
    MapGradPixelSdf(int map_type, float voxel_size, float T, int capacity_log2, int device, int max_capacity_log2);
    void query1(const Vec3f& point, float* d, float* g, float* w) const;

private:
    float zmin_ = 0.5f, zmax_ = 3.5f;                                  /* Sdf.h:67-68 */
};

#endif
