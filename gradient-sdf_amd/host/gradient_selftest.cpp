/*
 * gradient_selftest -- runs the gradient-accuracy analysis (gsdf_gradient_stats / gsdf_gradient_angles) from C++ through the
 * facade: fuse a few frames, MapGradPixelSdf::gradient_analysis (or MapPixelSdf's, with `base`) on the ladder of
 * matlab/GradientAnalysisSpheres.m:155, the text table, and the per-voxel rows of the C-ABI call.  Needs a GPU;
 * tests/test_gpu_gradient_analysis.py writes the inputs and compares the outputs with the numpy restatement
 * (tests/gradient_analysis_ref.py) of the map this program exports.
 *
 *   gradient_selftest <dir> W H n voxel_size trunc_voxels [base]
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)  spheres.bin (m*4 f32)
 *   writes <dir>/gradient_stats.txt, the statistics as the facade returned them: stats.bin (4*n_thr*5 f64), thresholds.bin
 *          (n_thr f32), the map: map_keys.bin (v*3 i32), map_payload.bin (v*5 f32), in gsdf_export's sorted order, and the arrays
 *          of gsdf_gradient_angles: angle_keys.bin (v*3 i32), angle_rows.bin (v*5 f32)
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "Image.h"
#include "MapGradPixelSdf.h"
#include "MapPixelSdf.h"
#include "exports.h"

static bool read_bin(const std::string& path, std::vector<float>& v, size_t n) {
    std::ifstream f(path, std::ios::binary);
    v.resize(n);
    return f.good() && f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float))).good();
}
static bool read_all(const std::string& path, std::vector<float>& v) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f.good()) return false;
    const std::streamsize bytes = f.tellg();
    f.seekg(0);
    v.resize((size_t)bytes / sizeof(float));
    return f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(float))).good();
}
template <class T>
static bool write_bin(const std::string& path, const std::vector<T>& v) {
    std::ofstream f(path, std::ios::binary);
    return f.good() && f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T))).good();
}

int main(int argc, char** argv) {
    if (argc < 7) { std::cerr << "usage: gradient_selftest <dir> W H n voxel_size trunc_voxels [base]" << std::endl; return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const bool base = argc > 7 && std::string(argv[7]) == "base";
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, P, spheres;
    if (!read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) || !read_bin(dir + "poses.bin", P, (size_t)n * 16) ||
        !read_all(dir + "spheres.bin", spheres) || spheres.empty() || spheres.size() % 4 != 0) {
        std::cerr << "gradient_selftest: cannot read the inputs in " << dir << std::endl;
        return 2;
    }
    try {
        Mat3f K;
        for (int i = 0; i < 9; ++i) K.m[i] = Kb[i];
        NormalEstimator NEst(W, H, K, 2 * 5 + 1);
        std::unique_ptr<MapGradPixelSdf> map;
        if (base) map.reset(new MapPixelSdf(vs, trunc * vs, 18, 0, 18));
        else map.reset(new MapGradPixelSdf(vs, trunc * vs, 18, 0, 18));
        ColorImage color;
        for (int i = 0; i < n; ++i) {
            Mat4f pose;
            for (int k = 0; k < 16; ++k) pose.m[k] = P[(size_t)i * 16 + k];
            DepthImage d;
            d.rows = H; d.cols = W;
            d.buf.assign(depth.begin() + (long)(i * N), depth.begin() + (long)((i + 1) * N));
            map->update(color, d, K, SE3(pose), &NEst);
        }
        const std::vector<float> thr = gsdf_exports::gradient_ladder(map->trunc_dist());
        std::vector<double> stats;
        if (!map->gradient_analysis(spheres, thr, stats)) throw std::runtime_error(gsdf_last_error());
        if (!map->save_gradient_analysis(spheres, thr, dir + "gradient_stats.txt")) throw std::runtime_error("cannot write the table");
        /* what the facade must refuse: no spheres, half a row, no thresholds, descending thresholds */
        std::vector<double> none;
        std::vector<float> down(thr.rbegin(), thr.rend());
        if (map->gradient_analysis({}, thr, none) || map->gradient_analysis({ 0.f, 0.f }, thr, none) || map->gradient_analysis(spheres, {}, none) ||
            map->gradient_analysis(spheres, down, none))
            throw std::runtime_error("gradient_analysis accepted arguments it must refuse");
        int64_t nv = 0;
        if (gsdf_gradient_angles(map->handle(), spheres.data(), (int)(spheres.size() / 4), nullptr, nullptr, 0, &nv) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        std::vector<int32_t> akeys((size_t)nv * 3);
        std::vector<float> arows((size_t)nv * 5);
        if (nv && gsdf_gradient_angles(map->handle(), spheres.data(), (int)(spheres.size() / 4), akeys.data(), arows.data(), nv, &nv) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        std::vector<int32_t> keys;
        std::vector<float> payload;
        map->export_arrays(keys, payload);
        if (keys != akeys) throw std::runtime_error("gsdf_gradient_angles and gsdf_export disagree about the keys");
        /* the count at the last threshold of the stored estimator cannot exceed the voxels */
        if (stats[(thr.size() - 1) * 5] > (double)nv) throw std::runtime_error("more angles counted than voxels");
        if (!write_bin(dir + "stats.bin", stats) || !write_bin(dir + "thresholds.bin", thr) || !write_bin(dir + "map_keys.bin", keys) ||
            !write_bin(dir + "map_payload.bin", payload) || !write_bin(dir + "angle_keys.bin", akeys) || !write_bin(dir + "angle_rows.bin", arows))
            throw std::runtime_error("cannot write the dump files");
        std::printf("voxels %lld thresholds %zu stored median at the last threshold %.4f central %.4f\n", (long long)nv, thr.size(),
                    stats[(thr.size() - 1) * 5 + 2], stats[(thr.size() + thr.size() - 1) * 5 + 2]);
    } catch (const std::exception& e) {
        std::cerr << "gradient_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("gradient_selftest: OK\n");
    return 0;
}
