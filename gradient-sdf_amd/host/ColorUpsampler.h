/*
 * ColorUpsampler -- sub-voxel colours of the reference (cpp/include/ps_optimizer/ColorUpsampler.h/.cpp with SdfVoxelHr,
 * sdf_voxel/SdfVoxel.h:61-112) as a facade over the C-ABI (gsdf_color_*).  main_photo_ba.cpp:300-311 builds it from the map
 * PhotoBA refined, calls computeColor() and writes the coloured cloud with extractCloud().
 *
 * The Hr voxels and their colours are computed on the GPU in one pass over the HBM table, at construction: that is where the
 * reference copies the map into its SdfHrMap (init :136-162), so later changes of the map do not reach the result, here as there.
 * computeColor() is kept for the reference's call sequence; the snapshot it would fill is already filled.
 * The map must have been fused with visibility tracking (MapGradPixelSdf::enable_vis()); at most 64 keyframes.
 * extractMesh (HrLayeredMarchingCubes) lives in HrLayeredMarchingCubes.h, as a free function over the same snapshot.
 */
#ifndef GSDF_HOST_COLOR_UPSAMPLER_H_
#define GSDF_HOST_COLOR_UPSAMPLER_H_

#include <fstream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "MapGradPixelSdf.h"
#include "PhotometricOptimizer.h"

class ColorUpsampler {
    MapGradPixelSdf* tSDF_;
    size_t num_frames_ = 0;
    size_t num_voxels_ = 0;

    void check(int rc, const char* what) const {
        if (rc != GSDF_OK) throw std::runtime_error(std::string(what) + ": " + gsdf_last_error());
    }

public:
    /* ColorUpsampler(sdf_lr, vis_map, images, poses, frame_idx, voxel_size, K) -- .cpp:117-133; the map brings its vis_ vectors,
     * voxel size and intrinsics.  The reference is handed the pre-BA key poses (main_photo_ba.cpp:295,300): pass the poses to
     * colour with, which need not be the ones PhotoBA ended with. */
    ColorUpsampler(MapGradPixelSdf* tSDF, const std::vector<std::shared_ptr<ColorImageF>>& images, const std::vector<Mat4f>& poses,
                   const std::vector<int>& frame_idx)
        : tSDF_(tSDF), num_frames_(frame_idx.size()) {
        const size_t n = frame_idx.size();
        if (!n || images.size() != n || poses.size() != n) throw std::runtime_error("ColorUpsampler: images / poses / keyframes differ in length");
        std::vector<float> img, P(16 * n);
        for (size_t i = 0; i < n; ++i) {
            img.insert(img.end(), images[i]->bgr.begin(), images[i]->bgr.end());
            for (int k = 0; k < 16; ++k) P[16 * i + k] = poses[i].m[k];
        }
        int64_t nv = 0;
        check(gsdf_color_compute(tSDF_->handle(), (int)n, img.data(), P.data(), frame_idx.data(), &nv), "gsdf_color_compute");
        num_voxels_ = (size_t)nv;
    }

    size_t getFrameNumber() const { return num_frames_; }                 /* .h:107 */
    size_t getVoxelNumber() const { return num_voxels_; }                 /* .h:112 */

    /* computeColor -- .cpp:334-377: done on the device at construction (see above) */
    void computeColor() {}

    /* extractCloud -- .cpp:251-330: "<filename>.ply", ASCII, one row per kept sub-voxel (point, normal, int(255 * colour)) */
    bool extractCloud(std::string filename) {
        filename += ".ply";                                                /* :255 */
        int64_t n = 0;
        check(gsdf_color_cloud(tSDF_->handle(), nullptr, 0, &n), "gsdf_color_cloud");
        std::vector<float> rows((size_t)n * 9);
        if (n) check(gsdf_color_cloud(tSDF_->handle(), rows.data(), n, &n), "gsdf_color_cloud");
        std::ofstream f(filename.c_str());
        if (!f.is_open()) return false;
        f << "ply" << std::endl << "format ascii 1.0" << std::endl << "element vertex " << n << std::endl
          << "property float x" << std::endl << "property float y" << std::endl << "property float z" << std::endl
          << "property float nx" << std::endl << "property float ny" << std::endl << "property float nz" << std::endl
          << "property uchar red" << std::endl << "property uchar green" << std::endl << "property uchar blue" << std::endl
          << "end_header" << std::endl;
        for (int64_t i = 0; i < n; ++i) {
            const float* p = &rows[9 * (size_t)i];
            f << p[0] << " " << p[1] << " " << p[2] << " " << p[3] << " " << p[4] << " " << p[5] << " " << int(255 * p[6]) << " "
              << int(255 * p[7]) << " " << int(255 * p[8]) << std::endl;
        }
        return true;
    }
};

#endif
