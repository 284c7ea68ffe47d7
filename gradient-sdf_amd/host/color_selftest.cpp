/*
 * color_selftest -- runs ColorUpsampler (host/ColorUpsampler.h, the facade for cpp/include/ps_optimizer/ColorUpsampler.h) from
 * C++ the way main_photo_ba.cpp:237-311 does: fuse at the given poses with vis_ on, PhotoBA from the start poses, then the colour
 * pass with those pre-BA poses and the refined distances, and extractCloud.  Needs a GPU; tests/test_gpu_color_upsampler.py writes
 * the inputs and compares the PLY with one written from the numpy restatement of the state this program leaves behind.
 *
 *   color_selftest <dir> W H n voxel_size trunc_voxels ba_iterations
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  images.bin (n*H*W*3 f32, BGR)  poses_true.bin / poses_start.bin (n*16 f32)
 *   writes <dir>/cloud.ply, and the map after PhotoBA: state_keys.bin (m*3 i32), state_payload.bin (m*5 f32), state_vis.bin
 *          (m*2 u32), in gsdf_export(sorted = 1) order
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "ColorUpsampler.h"
#include "Image.h"
#include "MapGradPixelSdf.h"
#include "PhotometricOptimizer.h"

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
    if (argc < 8) { std::cerr << "usage: color_selftest <dir> W H n voxel_size trunc_voxels ba_iterations" << std::endl; return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]), iters = atoi(argv[7]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, images, Pt, Ps;
    if (!read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) || !read_bin(dir + "images.bin", images, n * N * 3) ||
        !read_bin(dir + "poses_true.bin", Pt, (size_t)n * 16) || !read_bin(dir + "poses_start.bin", Ps, (size_t)n * 16)) {
        std::cerr << "color_selftest: cannot read the inputs in " << dir << std::endl;
        return 2;
    }
    try {
        Mat3f K;
        for (int i = 0; i < 9; ++i) K.m[i] = Kb[i];
        NormalEstimator NEst(W, H, K, 2 * 5 + 1);
        MapGradPixelSdf map(vs, trunc * vs, 20, 0, 20);
        map.enable_vis(64);
        ColorImage color;
        std::vector<Mat4f> truth((size_t)n), start((size_t)n);
        std::vector<std::shared_ptr<ColorImageF>> imgs;
        std::vector<int> keyframes;
        for (int i = 0; i < n; ++i) {
            for (int k = 0; k < 16; ++k) { truth[i].m[k] = Pt[(size_t)i * 16 + k]; start[i].m[k] = Ps[(size_t)i * 16 + k]; }
            DepthImage d;
            d.rows = H; d.cols = W;
            d.buf.assign(depth.begin() + (long)(i * N), depth.begin() + (long)((i + 1) * N));
            map.update(color, d, K, SE3(truth[i]), &NEst);
            auto im = std::make_shared<ColorImageF>();
            im->rows = H; im->cols = W;
            im->bgr.assign(images.begin() + (long)(i * N * 3), images.begin() + (long)((i + 1) * N * 3));
            imgs.push_back(im);
            keyframes.push_back(i);
        }
        OptSettings settings;
        settings.max_it = iters;
        PhotometricOptimizer opt(&map, settings);                      /* main_photo_ba.cpp:300-306 */
        opt.setImages(imgs);
        opt.setPoses(start);
        opt.setKeyframes(keyframes);
        opt.optimize();
        ColorUpsampler up(&map, imgs, start, keyframes);               /* :300-307: the pre-BA key poses, the refined distances */
        up.computeColor();
        if (!up.extractCloud(dir + "cloud")) { std::cerr << "color_selftest: cannot write the cloud" << std::endl; return 1; }
        const int64_t m = map.size();
        std::vector<int32_t> keys((size_t)m * 3), vkeys((size_t)m * 3);
        std::vector<float> pay((size_t)m * 5);
        std::vector<uint32_t> vis((size_t)m * 2);
        int64_t got = 0;
        if (gsdf_export(map.handle(), keys.data(), pay.data(), m, &got, 1, 0) != GSDF_OK ||
            gsdf_export_vis(map.handle(), vkeys.data(), vis.data(), 2, m, &got) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        if (!write_bin(dir + "state_keys.bin", keys) || !write_bin(dir + "state_payload.bin", pay) || !write_bin(dir + "state_vis.bin", vis))
            throw std::runtime_error("cannot write the state files");
        std::printf("frames %zu hr_voxels %zu voxels %lld\n", up.getFrameNumber(), up.getVoxelNumber(), (long long)m);
    } catch (const std::exception& e) {
        std::cerr << "color_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("color_selftest: OK\n");
    return 0;
}
