/*
 * color_mesh_selftest -- runs the coloured sub-voxel mesh (host/HrLayeredMarchingCubes.h, the facade for
 * cpp/include/mesh/HrLayeredMarchingCubes.h) from C++ the way ColorUpsampler::extractMesh does (ColorUpsampler.cpp:240-249): fuse
 * a few frames with vis_ on, build the ColorUpsampler (the colour snapshot), write the mesh.  Needs a GPU;
 * tests/test_gpu_hr_mesh.py writes the inputs and compares the PLY with one written from the numpy restatement
 * (tests/hr_mesh_ref.py) of the snapshot this program dumps.
 *
 *   color_mesh_selftest <dir> W H n voxel_size trunc_voxels
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  images.bin (n*H*W*3 f32, BGR)  poses.bin (n*16 f32)
 *   writes <dir>/mesh.ply, and the snapshot: snap_keys.bin (m*3 i32), snap_rows.bin (m*37 f32), in gsdf_color_export order
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "ColorUpsampler.h"
#include "HrLayeredMarchingCubes.h"
#include "Image.h"
#include "MapGradPixelSdf.h"

static bool read_bin(const std::string& path, std::vector<float>& v, size_t n) {
    std::ifstream f(path, std::ios::binary);
    v.resize(n);
    return f.good() && f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float))).good();
}
template <class T>
static bool write_bin(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    return f.good() && f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T))).good();
}

int main(int argc, char** argv) {
    if (argc < 7) { std::cerr << "usage: color_mesh_selftest <dir> W H n voxel_size trunc_voxels" << std::endl; return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, images, P;
    if (!read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) || !read_bin(dir + "images.bin", images, n * N * 3) ||
        !read_bin(dir + "poses.bin", P, (size_t)n * 16)) {
        std::cerr << "color_mesh_selftest: cannot read the inputs in " << dir << std::endl;
        return 2;
    }
    try {
        Mat3f K;
        for (int i = 0; i < 9; ++i) K.m[i] = Kb[i];
        NormalEstimator NEst(W, H, K, 2 * 5 + 1);
        MapGradPixelSdf map(vs, trunc * vs, 20, 0, 20);
        map.enable_vis(64);
        ColorImage color;
        std::vector<Mat4f> poses((size_t)n);
        std::vector<std::shared_ptr<ColorImageF>> imgs;
        std::vector<int> keyframes;
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < 16; ++k) poses[i].m[k] = P[(size_t)i * 16 + k];
            DepthImage d;
            d.rows = H; d.cols = W;
            d.buf.assign(depth.begin() + (long)(i * N), depth.begin() + (long)((i + 1) * N));
            map.update(color, d, K, SE3(poses[i]), &NEst);
            auto im = std::make_shared<ColorImageF>();
            im->rows = H; im->cols = W;
            im->bgr.assign(images.begin() + (long)(i * N * 3), images.begin() + (long)((i + 1) * N * 3));
            imgs.push_back(im);
            keyframes.push_back(i);
        }
        ColorUpsampler up(&map, imgs, poses, keyframes);                   /* the snapshot */
        up.computeColor();
        if (!extractMesh(&map, dir + "mesh")) { std::cerr << "color_mesh_selftest: cannot write the mesh" << std::endl; return 1; }
        HrLayeredMarchingCubes lmc(vs);
        lmc.computeIsoSurface(&map);
        const int64_t m = (int64_t)up.getVoxelNumber();
        std::vector<int32_t> keys((size_t)m * 3);
        std::vector<float> rows((size_t)m * 37);
        int64_t got = 0;
        if (gsdf_color_export(map.handle(), keys.data(), rows.data(), m, &got) != GSDF_OK) throw std::runtime_error(gsdf_last_error());
        if (!write_bin(dir + "snap_keys.bin", keys) || !write_bin(dir + "snap_rows.bin", rows))
            throw std::runtime_error("cannot write the snapshot files");
        std::printf("hr_voxels %lld faces %zu vertices %zu\n", (long long)m, lmc.getFaceNumber(), lmc.getVertexNumber());
    } catch (const std::exception& e) {
        std::cerr << "color_mesh_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("color_mesh_selftest: OK\n");
    return 0;
}
