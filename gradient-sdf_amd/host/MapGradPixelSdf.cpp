/* MapGradPixelSdf facade: every method forwards to the C-ABI (include/gsdf.h). */
#include "MapGradPixelSdf.h"

#include <algorithm>
#include <cmath>
#include <fstream>
#include <iostream>
#include <limits>

#include "exports.h"

void MapGradPixelSdf::check(int rc, const char* what) const {
    if (rc != GSDF_OK) throw std::runtime_error(std::string(what) + ": " + gsdf_last_error());
}

MapGradPixelSdf::MapGradPixelSdf(float voxel_size, float T, int capacity_log2, int device, int max_capacity_log2)
    : voxel_size_(voxel_size), T_(T) {
    check(gsdf_create(&ctx_, voxel_size, T, capacity_log2, device), "gsdf_create");
    /* tsdf_ of the reference grows as the scan does (MapGradPixelSdf.h:65-68): so does this map, up to max_capacity_log2 */
    if (max_capacity_log2 > capacity_log2) check(gsdf_set_auto_grow(ctx_, max_capacity_log2), "gsdf_set_auto_grow");
}

MapGradPixelSdf::MapGradPixelSdf(int map_type, float voxel_size, float T, int capacity_log2, int device, int max_capacity_log2)
    : voxel_size_(voxel_size), T_(T) {
    check(gsdf_create(&ctx_, voxel_size, T, capacity_log2, device), "gsdf_create");
    /* (the destructor does not run when a constructor throws) */
    if (gsdf_set_map_type(ctx_, map_type) != GSDF_OK) {
        const std::string e = gsdf_last_error();
        gsdf_destroy(ctx_);
        throw std::runtime_error("gsdf_set_map_type: " + e);
    }
    if (max_capacity_log2 > capacity_log2) check(gsdf_set_auto_grow(ctx_, max_capacity_log2), "gsdf_set_auto_grow");
}

MapGradPixelSdf::~MapGradPixelSdf() { gsdf_destroy(ctx_); }

void MapGradPixelSdf::query1(const Vec3f& point, float* d, float* g, float* w) const {
    check(gsdf_query(ctx_, point.data(), 1, d, g, w), "gsdf_query");
}

void MapGradPixelSdf::ensure_frame(const DepthImage& depth, const Mat3f& K, NormalEstimator* NEst) {
    if (frame_w_ == depth.cols && frame_h_ == depth.rows) return;
    const int win = NEst ? NEst->window : 11;
    check(gsdf_normals_init(ctx_, depth.cols, depth.rows, NEst ? NEst->K.data() : K.data(), win), "gsdf_normals_init");
    frame_w_ = depth.cols; frame_h_ = depth.rows;
}

void MapGradPixelSdf::prepare(int W, int H, const Mat3f& K, NormalEstimator* NEst) {
    if (frame_w_ == W && frame_h_ == H) return;
    check(gsdf_normals_init(ctx_, W, H, NEst ? NEst->K.data() : K.data(), NEst ? NEst->window : 11), "gsdf_normals_init");
    frame_w_ = W; frame_h_ = H;
}

void MapGradPixelSdf::update(const ColorImage&, const DepthImage& depth, const Mat3f K, const SE3& pose,
                             NormalEstimator* NEst) {
    if (!NEst) {   /* MapGradPixelSdf.cpp:55-58 */
        std::cerr << "No normal estimation possible - cannot update SDF volume!" << std::endl;
        return;
    }
    ensure_frame(depth, K, NEst);
    const Mat3f R = pose.rotationMatrix();           /* :62 */
    const Vec3f t = pose.translation();              /* :64 */
    check(gsdf_update(ctx_, depth.data(), R.data(), t.data()), "gsdf_update");
    std::cout << "Current frame counter: " << frame_counter() << std::endl;   /* :121 */
}

float MapGradPixelSdf::weights(Vec3f point) const {
    float d, g[3], w;
    check(gsdf_query(ctx_, point.data(), 1, &d, g, &w), "gsdf_query");
    return w;
}

float MapGradPixelSdf::tsdf(Vec3f point, Vec3f* grad_ptr) const {
    float d, g[3], w;
    check(gsdf_query(ctx_, point.data(), 1, &d, g, &w), "gsdf_query");
    if (!(w > 0.f)) throw std::out_of_range("MapGradPixelSdf::tsdf: voxel not in map");   /* tsdf_.at(idx) */
    if (grad_ptr) *grad_ptr = Vec3f(g[0], g[1], g[2]);
    return d;
}

void MapGradPixelSdf::raycast(const Mat3f& K, const SE3& pose, int W, int H, float* depth_out, float* normals_out) const {
    const Mat3f R = pose.rotationMatrix();
    const Vec3f t = pose.translation();
    check(gsdf_raycast(ctx_, K.m, R.m, t.data(), W, H, zmin_, zmax_, depth_out, normals_out), "gsdf_raycast");
}

int64_t MapGradPixelSdf::size() const {
    int64_t n = 0;
    check(gsdf_count(ctx_, &n), "gsdf_count");
    return n;
}

int64_t MapGradPixelSdf::frame_counter() const {
    gsdf_stats st;
    check(gsdf_get_stats(ctx_, &st), "gsdf_get_stats");
    return st.frames;
}

void MapGradPixelSdf::export_arrays(std::vector<int32_t>& keys, std::vector<float>& payload) const {
    const int64_t n = size();
    keys.resize((size_t)n * 3);
    payload.resize((size_t)n * 5);
    int64_t got = 0;
    if (n) check(gsdf_export(ctx_, keys.data(), payload.data(), n, &got, 1, 0), "gsdf_export");
}

SdfLrMap MapGradPixelSdf::get_tsdf() const {
    std::vector<int32_t> k;
    std::vector<float> p;
    export_arrays(k, p);
    SdfLrMap m;
    m.reserve(k.size() / 3);
    for (size_t i = 0; i < k.size() / 3; ++i) {
        SdfVoxel v;
        v.dist = p[5 * i];
        v.grad = Vec3f(p[5 * i + 1], p[5 * i + 2], p[5 * i + 3]);
        v.weight = p[5 * i + 4];
        m.emplace(Vec3i(k[3 * i], k[3 * i + 1], k[3 * i + 2]), v);
    }
    return m;
}

/* getSdf -- MapGradPixelSdf.h:127-129: tsdf_.at(idx), i.e. the stored voxel (dist, RAW gradient sum, weight) */
SdfVoxel MapGradPixelSdf::getSdf(Vec3i idx) const {
    const int32_t key[3] = { idx[0], idx[1], idx[2] };
    float p[5];
    int32_t found = 0;
    check(gsdf_get_voxels(ctx_, key, 1, p, &found), "gsdf_get_voxels");
    if (!found) throw std::out_of_range("MapGradPixelSdf::getSdf: voxel not in map");   /* .at() */
    SdfVoxel v;
    v.dist = p[0]; v.grad = Vec3f(p[1], p[2], p[3]); v.weight = p[4];
    return v;
}

/* extract_pc / save_sdf / extract_mesh -- MapGradPixelSdf.cpp:124-296: the writers live in exports.cpp (also reachable
 * from C through capi_host.cpp for hosts that hold a bare gsdf_ctx) */
bool MapGradPixelSdf::extract_pc(std::string filename) { return gsdf_exports::write_cloud_ply(ctx_, voxel_size_, filename, nullptr); }
bool MapGradPixelSdf::surface_cloud(std::vector<float>& rows6) const {
    int64_t n = 0;
    if (gsdf_surface_cloud(ctx_, nullptr, 0, &n) != GSDF_OK) return false;
    rows6.assign((size_t)n * 6, 0.f);
    return n == 0 || gsdf_surface_cloud(ctx_, rows6.data(), n, &n) == GSDF_OK;
}
bool MapGradPixelSdf::merge_from(const MapGradPixelSdf& other, const SE3& pose, int64_t* n_voxels, int64_t* n_blocks) {
    /* the pose goes as the 7 floats SE3 holds, like RigidPointOptimizer::optimize_points hands its pose_ to gsdf_align_points */
    return gsdf_merge_from_posed(ctx_, other.ctx_, pose.pose7(), n_voxels, n_blocks) == GSDF_OK;
}
/* removing voxels: the selection, erase, compact (include/gsdf.h; not in the reference) */
bool MapGradPixelSdf::select_box(const Vec3f& lo, const Vec3f& hi, int op, int64_t* n) { return gsdf_select_box(ctx_, lo.data(), hi.data(), op, n) == GSDF_OK; }
bool MapGradPixelSdf::select_weight(float w_min, float w_max, int op, int64_t* n) { return gsdf_select_weight(ctx_, w_min, w_max, op, n) == GSDF_OK; }
bool MapGradPixelSdf::select_points(const std::vector<float>& pts3, float radius, const SE3* pose, int op, int64_t* n) {
    return gsdf_select_points(ctx_, pts3.data(), (int64_t)(pts3.size() / 3), pose ? pose->pose7() : nullptr, radius, op, n) == GSDF_OK;
}
bool MapGradPixelSdf::select_invert(int64_t* n) { return gsdf_select_invert(ctx_, n) == GSDF_OK; }
bool MapGradPixelSdf::select_clear() { return gsdf_select_clear(ctx_) == GSDF_OK; }
bool MapGradPixelSdf::select_count(int64_t* n_voxels, int64_t* n_blocks) const { return gsdf_select_count(ctx_, n_voxels, n_blocks) == GSDF_OK; }
bool MapGradPixelSdf::select_export(std::vector<int32_t>& keys, std::vector<float>& payload, bool raw_sums) const {
    int64_t n = 0;
    if (gsdf_select_export(ctx_, nullptr, nullptr, 0, &n, raw_sums ? 1 : 0) != GSDF_OK) return false;
    keys.assign((size_t)n * 3, 0);
    payload.assign((size_t)n * 5, 0.f);
    return n == 0 || gsdf_select_export(ctx_, keys.data(), payload.data(), n, &n, raw_sums ? 1 : 0) == GSDF_OK;
}
bool MapGradPixelSdf::erase_selected(int64_t* n_voxels, int64_t* n_blocks_emptied) { return gsdf_erase_selected(ctx_, n_voxels, n_blocks_emptied) == GSDF_OK; }
bool MapGradPixelSdf::compact(int new_capacity_log2, int64_t* n_blocks_dropped) { return gsdf_compact(ctx_, new_capacity_log2, n_blocks_dropped) == GSDF_OK; }
bool MapGradPixelSdf::crop(const Vec3f& lo, const Vec3f& hi) { return select_box(lo, hi) && select_invert() && erase_selected() && compact(); }
bool MapGradPixelSdf::prune(float min_weight) { return select_weight(0.f, min_weight) && erase_selected() && compact(); }
bool MapGradPixelSdf::save_sdf(std::string filename) { return gsdf_exports::write_sdf_txt(ctx_, voxel_size_, filename); }
bool MapGradPixelSdf::extract_mesh(std::string filename) { return gsdf_exports::write_mesh_ply(ctx_, voxel_size_, filename, nullptr); }
bool MapGradPixelSdf::extract_mesh_indexed(std::string filename) { return gsdf_exports::write_indexed_mesh_ply(ctx_, filename, nullptr, nullptr); }
bool MapGradPixelSdf::extract_mesh_indexed(std::string filename, int64_t min_faces, long* n_components, long* n_kept, long* n_faces,
                                           long* n_faces_all) {
    return gsdf_exports::write_filtered_mesh_ply(ctx_, filename, min_faces, n_components, n_kept, n_faces, n_faces_all);
}
bool MapGradPixelSdf::mesh_components(MeshComponents& out) const {
    int64_t nv = 0, nf = 0, nc = 0;
    if (gsdf_mesh_components(ctx_, 0.f, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 0, &nv, &nf, &nc) != GSDF_OK) return false;
    out.vertex_comp.assign((size_t)nv, 0); out.face_comp.assign((size_t)nf, 0);
    out.counts.assign((size_t)nc * 2, 0); out.bbox.assign((size_t)nc * 6, 0.f);
    out.n_components = nc;
    if (nf == 0) return true;
    return gsdf_mesh_components(ctx_, 0.f, nullptr, out.vertex_comp.data(), out.face_comp.data(), nv, nf, out.counts.data(), out.bbox.data(), nc,
                                &nv, &nf, &nc) == GSDF_OK;
}
bool MapGradPixelSdf::save_mesh_components(std::string filename) const { return gsdf_exports::write_mesh_components_txt(ctx_, filename, nullptr); }
bool MapGradPixelSdf::gradient_analysis(const std::vector<float>& spheres4, const std::vector<float>& thresholds, std::vector<double>& stats) const {
    if (spheres4.empty() || spheres4.size() % 4 != 0 || thresholds.empty()) return false;
    stats.assign(4 * thresholds.size() * 5, 0.0);
    return gsdf_gradient_stats(ctx_, spheres4.data(), (int)(spheres4.size() / 4), thresholds.data(), (int)thresholds.size(), stats.data()) == GSDF_OK;
}
bool MapGradPixelSdf::save_gradient_analysis(const std::vector<float>& spheres4, const std::vector<float>& thresholds, std::string filename) const {
    return gsdf_exports::write_gradient_stats_txt(ctx_, spheres4, thresholds, filename);
}
