/*
 * merge_posed_selftest -- registration AND merge of two maps from C++ through the facade; continues align_selftest: fuse two
 * maps A and B from a dumped stream, take B's surface cloud (MapGradPixelSdf::surface_cloud), move it into a source frame by the
 * inverse of a pose read from a file, register it against A (RigidPointOptimizer::optimize_points) from the identity, and merge
 * B into A under the pose that came out (MapGradPixelSdf::merge_from(other, pose)).  Needs a GPU;
 * tests/test_gpu_merge_posed.py writes the inputs and compares the outputs with the Python path under the same pose.
 *
 *   merge_posed_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)  displace.bin (7 f32: tx ty tz qx qy qz qw, source -> map)
 *   fuses  frames [a0, a1) into A and [b0, b1) into B
 *   writes <dir>/pose.bin (7 f32, the recovered pose)  merge.txt ("n_voxels n_blocks count_before count_after")
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
        std::cerr << "usage: merge_posed_selftest <dir> W H n voxel_size trunc_voxels a0 a1 b0 b1 conv_threshold" << std::endl;
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
        std::cerr << "merge_posed_selftest: cannot read the inputs in " << dir << std::endl;
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
        /* the source frame: x_src = R^T (x - t) in double, rounded once (as align_selftest) */
        float Rf[9];
        gsdf_quat_to_R(disp.data() + 3, Rf);
        std::vector<float> src(m * 3);
        for (size_t i = 0; i < m; ++i) {
            const double d[3] = { (double)cloud[6 * i] - disp[0], (double)cloud[6 * i + 1] - disp[1], (double)cloud[6 * i + 2] - disp[2] };
            for (int c = 0; c < 3; ++c) src[3 * i + c] = (float)((double)Rf[c] * d[0] + (double)Rf[3 + c] * d[1] + (double)Rf[6 + c] * d[2]);
        }
        RigidPointOptimizer opt(25, conv, 1.f, &A);
        const bool converged = opt.optimize_points(src.data(), m);
        /* what the facade must refuse: a plain-SDF map has no stored gradient to rotate, on either side */
        MapPixelSdf base(vs, trunc * vs, 16, 0, 16);
        int64_t nv = -1, nb = -1;
        if (A.merge_from(base, opt.pose(), &nv, &nb) || nv != 0 || nb != 0) throw std::runtime_error("merge_from accepted a MapPixelSdf as the source");
        if (base.merge_from(B, opt.pose())) throw std::runtime_error("merge_from accepted a MapPixelSdf as the destination");
        const int64_t before = A.size(), frames_a = A.frame_counter(), frames_b = B.frame_counter();
        if (!A.merge_from(B, opt.pose(), &nv, &nb)) throw std::runtime_error(std::string("merge_from: ") + gsdf_last_error());
        const int64_t after = A.size();
        if (A.frame_counter() != frames_a + frames_b) throw std::runtime_error("frame_counter is not the sum of both maps'");
        if (nv <= 0 || nb <= 0 || after < before || after > before + nv) throw std::runtime_error("the counts do not fit count()");
        if (!write_bin(dir + "pose.bin", opt.pose().pose7(), 7)) throw std::runtime_error("cannot write pose.bin");
        std::ofstream r(dir + "merge.txt");
        r << nv << " " << nb << " " << before << " " << after << std::endl;
        if (!r.good()) throw std::runtime_error("cannot write merge.txt");
        const float* p = opt.pose().pose7();
        std::printf("points %zu converged %d passes %d\n", m, converged ? 1 : 0, opt.last_passes());
        std::printf("pose %.6f %.6f %.6f  %.6f %.6f %.6f %.6f\n", p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
        std::printf("n_voxels %lld n_blocks %lld count %lld -> %lld\n", (long long)nv, (long long)nb, (long long)before, (long long)after);
    } catch (const std::exception& e) {
        std::cerr << "merge_posed_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("merge_posed_selftest: OK\n");
    return 0;
}
