/*
 * align_robust_selftest -- the robust map-to-map registration from C++ through the facade: fuse two maps A and B from a dumped
 * stream, take B's surface cloud (MapGradPixelSdf::surface_cloud), move it into a source frame by the inverse of a pose read from
 * a file, and register it against A from the identity three times: with the default loss (L2, RigidPointOptimizer::optimize_points
 * on the plain entry), with RigidPointOptimizer::set_loss(loss, scale), and from a grid of starts with that loss
 * (optimize_points_multi, the floor of the weight sum = half the points).  Then the residuals of the points under the robust pose
 * (RigidPointOptimizer::residuals).  Needs a GPU; tests/test_gpu_align_robust.py writes the inputs and compares the outputs with
 * the Python path on the same points.
 *
 *   align_robust_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold loss scale trans_step trans_k
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)  displace.bin (7 f32: tx ty tz qx qy qz qw, source -> map)
 *   fuses  frames [a0, a1) into A and [b0, b1) into B
 *   writes <dir>/src.bin (p*3 f32, the displaced points: R^T (x - t))  l2_pose.bin, robust_pose.bin (7 f32 each)
 *          res_phi.bin, res_w.bin (p f32 each)  starts.bin, multi_poses.bin (m*7 f32 each)
 *          robust_result.txt (line 1: "points", line 2: the L2 run's "converged passes", line 3: the robust run's, line 4:
 *          "best m", line 5: the m converged flags, line 6: the m pass counts)
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
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
        std::cerr << "usage: align_robust_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold loss scale trans_step trans_k"
                  << std::endl;
        return 2;
    }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const int a0 = atoi(argv[7]), a1 = atoi(argv[8]), b0 = atoi(argv[9]), b1 = atoi(argv[10]);
    const float conv = (float)atof(argv[11]);
    const int loss = atoi(argv[12]);
    const float scale = (float)atof(argv[13]), trans_step = (float)atof(argv[14]);
    const int trans_k = atoi(argv[15]);
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, P, disp;
    if (n < 1 || a0 < 0 || a1 > n || b0 < 0 || b1 > n || !read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) ||
        !read_bin(dir + "poses.bin", P, (size_t)n * 16) || !read_bin(dir + "displace.bin", disp, 7)) {
        std::cerr << "align_robust_selftest: cannot read the inputs in " << dir << std::endl;
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
        RigidPointOptimizer opt(25, conv, 1.f, &A);
        if (opt.loss() != 0) throw std::runtime_error("the default loss is not L2");
        /* what set_loss must refuse, leaving the loss as it was */
        int refused = 0;
        const float nan = std::numeric_limits<float>::quiet_NaN();
        for (const auto& bad : { std::pair<int, float>{ -1, scale }, { 5, scale }, { loss, 0.f }, { loss, -scale }, { loss, nan } }) {
            try { opt.set_loss(bad.first, bad.second); } catch (const std::invalid_argument&) { ++refused; }
        }
        if (refused != 5 || opt.loss() != 0) throw std::runtime_error("set_loss accepted a bad loss or scale");
        /* 1. the default: the plain entry */
        opt.set_pose(SE3::from_pose7(identity));
        const bool conv_l2 = opt.optimize_points(src.data(), np);
        const int passes_l2 = opt.last_passes();
        const SE3 pose_l2 = opt.pose();
        /* 2. the same call with the loss */
        opt.set_loss(loss, scale);
        if (opt.loss() != loss || opt.loss_scale() != scale) throw std::runtime_error("set_loss did not take");
        opt.set_pose(SE3::from_pose7(identity));
        const bool conv_r = opt.optimize_points(src.data(), np);
        const int passes_r = opt.last_passes();
        const SE3 pose_r = opt.pose();
        /* 3. the residuals under the robust pose */
        std::vector<float> phi, w;
        opt.residuals(src.data(), np, pose_r, phi, w);
        if (phi.size() != np || w.size() != np) throw std::runtime_error("residuals() did not size its outputs");
        /* 4. the grid of starts with the loss */
        const float pivot[3] = { (float)(cen[0] / (double)np), (float)(cen[1] / (double)np), (float)(cen[2] / (double)np) };
        int m = 0;
        if (gsdf_align_starts(identity, pivot, 0.f, 0, trans_step, trans_k, nullptr, 0, &m) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        std::vector<float> starts((size_t)m * 7);
        if (gsdf_align_starts(identity, pivot, 0.f, 0, trans_step, trans_k, starts.data(), m, &m) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        const int best = opt.optimize_points_multi(src.data(), np, starts.data(), m, (int64_t)(np / 2));
        if (best >= 0) {
            const SE3 result = opt.pose();
            for (int i = 0; i < 7; ++i)
                if (result.pose7()[i] != opt.multi_poses()[(size_t)best * 7 + i]) throw std::runtime_error("pose() is not the picked run's pose");
        }
        /* what the facade must refuse: a plain-SDF map has no stored-gradient query for point sets */
        MapPixelSdf base(vs, trunc * vs, 16, 0, 16);
        int base_refused = 0;
        RigidPointOptimizer bopt(&base);
        bopt.set_loss(loss, scale);
        try { bopt.optimize_points(src.data(), np); } catch (const std::runtime_error&) { ++base_refused; }
        try { bopt.residuals(src.data(), np, pose_r, phi, w); } catch (const std::runtime_error&) { ++base_refused; }
        if (base_refused != 2) throw std::runtime_error("the robust calls accepted a MapPixelSdf");
        opt.residuals(src.data(), np, pose_r, phi, w);
        if (!write_bin(dir + "src.bin", src.data(), src.size()) || !write_bin(dir + "l2_pose.bin", pose_l2.pose7(), 7) ||
            !write_bin(dir + "robust_pose.bin", pose_r.pose7(), 7) || !write_bin(dir + "res_phi.bin", phi.data(), np) ||
            !write_bin(dir + "res_w.bin", w.data(), np) || !write_bin(dir + "starts.bin", starts.data(), starts.size()) ||
            !write_bin(dir + "multi_poses.bin", opt.multi_poses().data(), opt.multi_poses().size()))
            throw std::runtime_error("cannot write the dump files");
        std::ofstream r(dir + "robust_result.txt");
        r << np << "\n" << (conv_l2 ? 1 : 0) << " " << passes_l2 << "\n" << (conv_r ? 1 : 0) << " " << passes_r << "\n" << best << " " << m << "\n";
        for (int h = 0; h < m; ++h) r << opt.multi_converged()[(size_t)h] << (h + 1 < m ? " " : "\n");
        for (int h = 0; h < m; ++h) r << opt.multi_passes()[(size_t)h] << (h + 1 < m ? " " : "\n");
        r.flush();
        if (!r.good()) throw std::runtime_error("cannot write robust_result.txt");
        std::printf("points %zu loss %d scale %g: L2 %d passes, robust %d passes, starts %d best %d\n", np, loss, (double)scale, passes_l2,
                    passes_r, m, best);
    } catch (const std::exception& e) {
        std::cerr << "align_robust_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("align_robust_selftest: OK\n");
    return 0;
}
