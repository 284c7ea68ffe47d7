/*
 * align_multi_selftest -- multi-start map-to-map registration from C++ through the facade: fuse two maps A and B from a dumped
 * stream, take B's surface cloud (MapGradPixelSdf::surface_cloud), move it into a source frame by the inverse of a pose read
 * from a file, take the grid of starts around the identity with the cloud's centroid as pivot (gsdf_align_starts), and register
 * from all of them at once against A (RigidPointOptimizer::optimize_points_multi, min_count = half the points).  Needs a GPU;
 * tests/test_gpu_align_multi.py writes the inputs and compares the outputs with the Python path on the same points and starts.
 *
 *   align_multi_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold rot_step_rad rot_k trans_step trans_k
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)  displace.bin (7 f32: tx ty tz qx qy qz qw, source -> map)
 *   fuses  frames [a0, a1) into A and [b0, b1) into B
 *   writes <dir>/src.bin (p*3 f32, the displaced points: R^T (x - t))  starts.bin (m*7 f32)  multi_poses.bin (m*7 f32, the results)
 *          multi_result.txt (line 1: "best m points", line 2: the m converged flags, line 3: the m pass counts)
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
    if (argc < 16) {
        std::cerr << "usage: align_multi_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold rot_step_rad rot_k trans_step trans_k"
                  << std::endl;
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const int a0 = atoi(argv[7]), a1 = atoi(argv[8]), b0 = atoi(argv[9]), b1 = atoi(argv[10]);
    const float conv = (float)atof(argv[11]);
    const float rot_step = (float)atof(argv[12]), trans_step = (float)atof(argv[14]);
    const int rot_k = atoi(argv[13]), trans_k = atoi(argv[15]);
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, P, disp;
    if (n < 1 || a0 < 0 || a1 > n || b0 < 0 || b1 > n || !read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) ||
        !read_bin(dir + "poses.bin", P, (size_t)n * 16) || !read_bin(dir + "displace.bin", disp, 7)) {
        std::cerr << "align_multi_selftest: cannot read the inputs in " << dir << std::endl;
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
        const size_t np = cloud.size() / 6;
        if (np == 0) throw std::runtime_error("B's surface cloud is empty");
        /* the source frame: x_src = R^T (x - t) in double, rounded once */
        float Rf[9];
        gsdf_quat_to_R(disp.data() + 3, Rf);
        std::vector<float> src(np * 3);
        double cen[3] = { 0, 0, 0 };
        for (size_t i = 0; i < np; ++i) {
            const double d[3] = { (double)cloud[6 * i] - disp[0], (double)cloud[6 * i + 1] - disp[1], (double)cloud[6 * i + 2] - disp[2] };
            for (int c = 0; c < 3; ++c) {
                src[3 * i + c] = (float)((double)Rf[c] * d[0] + (double)Rf[3 + c] * d[1] + (double)Rf[6 + c] * d[2]);
                cen[c] += (double)src[3 * i + c];
            }
        }
        const float identity[7] = { 0, 0, 0, 0, 0, 0, 1 };
        const float pivot[3] = { (float)(cen[0] / (double)np), (float)(cen[1] / (double)np), (float)(cen[2] / (double)np) };
        int m = 0;
        if (gsdf_align_starts(identity, pivot, rot_step, rot_k, trans_step, trans_k, nullptr, 0, &m) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        std::vector<float> starts((size_t)m * 7);
        if (gsdf_align_starts(identity, pivot, rot_step, rot_k, trans_step, trans_k, starts.data(), m, &m) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        RigidPointOptimizer opt(25, conv, 1.f, &A);
        const float before[7] = { 0.5f, 0, 0, 0, 0, 0, 1 };
        opt.set_pose(SE3::from_pose7(before));
        const int best = opt.optimize_points_multi(src.data(), np, starts.data(), m, (int64_t)(np / 2));
        const SE3 result = opt.pose();
        const float* got = result.pose7();
        const float* want = best >= 0 ? opt.multi_poses().data() + (size_t)best * 7 : before;
        for (int i = 0; i < 7; ++i)
            if (got[i] != want[i]) throw std::runtime_error("pose() is not the picked run's pose (or was touched without a pick)");
        if (best >= 0 && opt.last_passes() != opt.multi_passes()[(size_t)best]) throw std::runtime_error("last_passes() is not the picked run's");
        /* what the facade must refuse: a plain-SDF map has no stored-gradient query for point sets */
        MapPixelSdf base(vs, trunc * vs, 16, 0, 16);
        bool refused = false;
        try { RigidPointOptimizer bopt(&base); bopt.optimize_points_multi(src.data(), np, starts.data(), m, 1); } catch (const std::runtime_error&) { refused = true; }
        if (!refused) throw std::runtime_error("optimize_points_multi accepted a MapPixelSdf");
        if (!write_bin(dir + "src.bin", src.data(), src.size()) || !write_bin(dir + "starts.bin", starts.data(), starts.size()) ||
            !write_bin(dir + "multi_poses.bin", opt.multi_poses().data(), opt.multi_poses().size()))
            throw std::runtime_error("cannot write the dump files");
        std::ofstream r(dir + "multi_result.txt");
        r << best << " " << m << " " << np << "\n";
        for (int h = 0; h < m; ++h) r << opt.multi_converged()[(size_t)h] << (h + 1 < m ? " " : "\n");
        for (int h = 0; h < m; ++h) r << opt.multi_passes()[(size_t)h] << (h + 1 < m ? " " : "\n");
        r.flush();
        if (!r.good()) throw std::runtime_error("cannot write multi_result.txt");
        std::printf("points %zu starts %d best %d\n", np, m, best);
    } catch (const std::exception& e) {
        std::cerr << "align_multi_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("align_multi_selftest: OK\n");
    return 0;
}
