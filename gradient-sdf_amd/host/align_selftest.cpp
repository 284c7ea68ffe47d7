/*
 * align_selftest -- map-to-map registration from C++ through the facade: fuse two maps A and B from a dumped stream, take B's
 * surface cloud (MapGradPixelSdf::surface_cloud), move it into a source frame by the inverse of a pose read from a file, and
 * register it against A (RigidPointOptimizer::optimize_points) from the identity.  Needs a GPU;
 * tests/test_gpu_align_points.py writes the inputs and compares the outputs with the Python path on the same points.
 *
 *   align_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)  displace.bin (7 f32: tx ty tz qx qy qz qw, source -> map)
 *   fuses  frames [a0, a1) into A and [b0, b1) into B
 *   writes <dir>/cloud.bin (m*6 f32, B's rows)  src.bin (m*3 f32, the displaced points: R^T (x - t))  pose.bin (7 f32, the result)
 *          result.txt ("converged passes points")
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "Image.h"
#include "MapGradPixelSdf.h"
#include "MapPixelSdf.h"
#include "RigidOptimizer.h"

static bool read_bin(const std::string& path, std::vector<float>& v, size_t n) {
    std::ifstream f(path, std::ios::binary);
    v.resize(n);
    return f.good() && f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(float))).good();
}
static bool write_bin(const std::string& path, const float* p, size_t n) {
    std::ofstream f(path, std::ios::binary);
    return f.good() && f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(float))).good();
}

int main(int argc, char** argv) {
    if (argc < 12) {
        std::cerr << "usage: align_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold" << std::endl;
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const int a0 = atoi(argv[7]), a1 = atoi(argv[8]), b0 = atoi(argv[9]), b1 = atoi(argv[10]);
    const float conv = (float)atof(argv[11]);
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, P, disp;
    if (n < 1 || a0 < 0 || a1 > n || b0 < 0 || b1 > n || !read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) ||
        !read_bin(dir + "poses.bin", P, (size_t)n * 16) || !read_bin(dir + "displace.bin", disp, 7)) {
        std::cerr << "align_selftest: cannot read the inputs in " << dir << std::endl;
        return 2;
    }
    try {
        Mat3f K;
        for (int i = 0; i < 9; ++i) K.m[i] = Kb[i];
        NormalEstimator NEst(W, H, K, 2 * 5 + 1);
        MapGradPixelSdf A(vs, trunc * vs, 19, 0, 19), B(vs, trunc * vs, 19, 0, 19);
        ColorImage color;
        auto fuse = [&](MapGradPixelSdf& map, int f0, int f1) {
            for (int i = f0; i < f1; ++i) {
                Mat4f pose;
                for (int k = 0; k < 16; ++k) pose.m[k] = P[(size_t)i * 16 + k];
                DepthImage d;
                d.rows = H; d.cols = W;
                d.buf.assign(depth.begin() + (long)(i * N), depth.begin() + (long)((i + 1) * N));
                map.update(color, d, K, SE3(pose), &NEst);
            }
        };
        fuse(A, a0, a1);
        fuse(B, b0, b1);
        std::vector<float> cloud;
        if (!B.surface_cloud(cloud)) throw std::runtime_error(gsdf_last_error());
        const size_t m = cloud.size() / 6;
        /* the source frame: x_src = R^T (x - t) in double, rounded once */
        float Rf[9];
        gsdf_quat_to_R(disp.data() + 3, Rf);
        std::vector<float> src(m * 3);
        for (size_t i = 0; i < m; ++i) {
            const double d[3] = { (double)cloud[6 * i] - disp[0], (double)cloud[6 * i + 1] - disp[1], (double)cloud[6 * i + 2] - disp[2] };
            for (int c = 0; c < 3; ++c) src[3 * i + c] = (float)((double)Rf[c] * d[0] + (double)Rf[3 + c] * d[1] + (double)Rf[6 + c] * d[2]);
        }
        RigidPointOptimizer opt(25, conv, 1.f, &A);
        const bool converged = opt.optimize_points(src.data(), m);
        /* what the facade must refuse: a plain-SDF map has no stored-gradient query for point sets and no extract_pc rows */
        MapPixelSdf base(vs, trunc * vs, 16, 0, 16);
        std::vector<float> none;
        if (base.surface_cloud(none)) throw std::runtime_error("surface_cloud accepted a MapPixelSdf");
        bool refused = false;
        try { RigidPointOptimizer bopt(&base); bopt.optimize_points(src.data(), m); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) throw std::runtime_error("optimize_points accepted a MapPixelSdf");
        if (!write_bin(dir + "cloud.bin", cloud.data(), cloud.size()) || !write_bin(dir + "src.bin", src.data(), src.size()) ||
            !write_bin(dir + "pose.bin", opt.pose().pose7(), 7))
            throw std::runtime_error("cannot write the dump files");
        std::ofstream r(dir + "result.txt");
        r << (converged ? 1 : 0) << " " << opt.last_passes() << " " << m << std::endl;
        if (!r.good()) throw std::runtime_error("cannot write result.txt");
        std::printf("points %zu converged %d passes %d\n", m, converged ? 1 : 0, opt.last_passes());
    } catch (const std::exception& e) {
        std::cerr << "align_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("align_selftest: OK\n");
    return 0;
}
