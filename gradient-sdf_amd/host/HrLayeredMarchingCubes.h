/*
 * HrLayeredMarchingCubes -- the coloured sub-voxel mesh of the reference (cpp/include/mesh/HrLayeredMarchingCubes.h/.cpp) as a
 * facade over the C-ABI (gsdf_color_mesh), and extractMesh, the body of ColorUpsampler::extractMesh (ColorUpsampler.cpp:240-249)
 * as a free function.
 *
 * The reference hands computeIsoSurface the ColorUpsampler's SdfHrMap; here that map is the colour snapshot the context holds
 * after gsdf_color_compute (a ColorUpsampler was constructed on the map), so computeIsoSurface takes the map.  The surface is
 * extracted on the GPU; see include/gsdf.h for what is reproduced and for the one deliberate deviation (getColor reads green and
 * blue at the cell's own index).
 */
#ifndef GSDF_HOST_HR_LAYERED_MARCHING_CUBES_H_
#define GSDF_HOST_HR_LAYERED_MARCHING_CUBES_H_

#include <cstdint>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "MapGradPixelSdf.h"
#include "mat.h"

class HrLayeredMarchingCubes {
    Vec3f voxelSize_;                     /* kept for the reference's signature: the snapshot carries its own voxel size */
    std::vector<float> vertices_;         /* 3 per vertex, 3 vertices per face, no de-duplication (addVertex :807-814) */
    std::vector<uint8_t> colors_;         /* 3 per vertex */

public:
    explicit HrLayeredMarchingCubes(const Vec3f& voxelSize) : voxelSize_(voxelSize) {}                 /* .h:61 */
    explicit HrLayeredMarchingCubes(float voxel_size) : voxelSize_(voxel_size, voxel_size, voxel_size) {}

    /* computeIsoSurface -- .cpp:359-585 over the snapshot of the last gsdf_color_compute on this map */
    bool computeIsoSurface(MapGradPixelSdf* map_with_snapshot, float isoValue = 0.f) {
        if (!map_with_snapshot) return false;                              /* :361 */
        vertices_.clear();
        colors_.clear();
        int64_t n = 0;
        if (gsdf_color_mesh(map_with_snapshot->handle(), isoValue, nullptr, nullptr, 0, &n) != GSDF_OK)
            throw std::runtime_error(std::string("gsdf_color_mesh: ") + gsdf_last_error());
        vertices_.resize((size_t)n * 9);
        colors_.resize((size_t)n * 9);
        if (n && gsdf_color_mesh(map_with_snapshot->handle(), isoValue, vertices_.data(), colors_.data(), n, &n) != GSDF_OK)
            throw std::runtime_error(std::string("gsdf_color_mesh: ") + gsdf_last_error());
        return true;
    }

    const Vec3f& voxelSize() const { return voxelSize_; }
    size_t getVertexNumber() const { return vertices_.size() / 3; }
    size_t getFaceNumber() const { return vertices_.size() / 9; }

    /* savePly -- .cpp:824-864 */
    bool savePly(const std::string& filename) const {
        if (vertices_.empty()) return false;
        std::ofstream plyFile(filename.c_str());
        if (!plyFile.is_open()) return false;
        const size_t nv = vertices_.size() / 3;
        plyFile << "ply" << std::endl << "format ascii 1.0" << std::endl << "element vertex " << nv << std::endl
                << "property float x" << std::endl << "property float y" << std::endl << "property float z" << std::endl
                << "property uchar red" << std::endl << "property uchar green" << std::endl << "property uchar blue" << std::endl
                << "element face " << (int)(nv / 3) << std::endl << "property list uchar int vertex_indices" << std::endl
                << "end_header" << std::endl;
        for (size_t i = 0; i < nv; ++i) {
            const float* p = &vertices_[3 * i];
            const uint8_t* c = &colors_[3 * i];
            plyFile << p[0] << " " << p[1] << " " << p[2] << " " << (int)c[0] << " " << (int)c[1] << " " << (int)c[2] << std::endl;
        }
        for (size_t i = 0; i < nv / 3; ++i)
            plyFile << "3 " << (int)(3 * i) << " " << (int)(3 * i + 1) << " " << (int)(3 * i + 2) << std::endl;
        plyFile.close();
        return true;
    }
};

/* ColorUpsampler::extractMesh -- ColorUpsampler.cpp:240-249: "<filename>.ply" of the map's colour snapshot */
inline bool extractMesh(MapGradPixelSdf* map_with_snapshot, std::string filename) {
    const float vs = map_with_snapshot->voxel_size();
    HrLayeredMarchingCubes lmc(Vec3f(vs, vs, vs));
    lmc.computeIsoSurface(map_with_snapshot);
    const bool success = lmc.savePly(filename + ".ply");
    if (success) std::cout << "Mesh " << filename << ".ply successfully saved." << std::endl;
    return success;
}

#endif
