/*
 * indexed_mesh_selftest -- runs the indexed iso-surface mesh (gsdf_extract_mesh_indexed) from C++ through the facade: fuse a few
 * frames, MapGradPixelSdf::extract_mesh_indexed (or MapPixelSdf's, with `base`), and the C-ABI call itself next to
 * gsdf_extract_mesh.  Needs a GPU; tests/test_gpu_indexed_mesh.py writes the inputs and compares the PLY and the dumps with the
 * numpy restatement (tests/indexed_mesh_ref.py) of the map this program exports.
 *
 *   indexed_mesh_selftest <dir> W H n voxel_size trunc_voxels [base]
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)
 *   writes <dir>/mesh_indexed.ply, the map: map_keys.bin (m*3 i32), map_payload.bin (m*5 f32), in gsdf_export's sorted order,
 *          and the arrays of the C-ABI call: mesh_v.bin, mesh_n.bin (nv*3 f32), mesh_f.bin (nf*3 i32)
 *
 *   indexed_mesh_selftest --ply-only <file>
 *   no GPU: a tetrahedron through MarchingCubes::saveIndexedPly, and the inputs the writer refuses (tests/test_indexed_mesh.py)
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
#include "MarchingCubes.h"

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

static int ply_only(const std::string& file) {
    const std::vector<float> v = { 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.5f };
    const std::vector<float> n = { -0.5f, -0.5f, -0.5f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, -0.f };
    const std::vector<int32_t> f = { 0, 2, 1, 0, 1, 3, 1, 2, 3, 0, 3, 2 };
    std::vector<int32_t> bad = f;
    bad[5] = 4;                                                            /* an id outside the vertices */
    const std::vector<float> fewer(n.begin(), n.end() - 3);
    if (MarchingCubes::saveIndexedPly(file + ".refused", v, n, bad) || MarchingCubes::saveIndexedPly(file + ".refused", v, fewer, f) ||
        MarchingCubes::saveIndexedPly(file + ".refused", v, n, std::vector<int32_t>(f.begin(), f.end() - 1))) {
        std::cerr << "indexed_mesh_selftest: saveIndexedPly accepted arrays that do not fit together" << std::endl;
        return 1;
    }
    if (!MarchingCubes::saveIndexedPly(file, v, n, f)) { std::cerr << "indexed_mesh_selftest: cannot write " << file << std::endl; return 1; }
    std::printf("indexed_mesh_selftest: OK\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "--ply-only") return ply_only(argv[2]);
    if (argc < 7) { std::cerr << "usage: indexed_mesh_selftest <dir> W H n voxel_size trunc_voxels [base] | --ply-only <file>" << std::endl; return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const bool base = argc > 7 && std::string(argv[7]) == "base";
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, P;
    if (!read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) || !read_bin(dir + "poses.bin", P, (size_t)n * 16)) {
        std::cerr << "indexed_mesh_selftest: cannot read the inputs in " << dir << std::endl;
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
        if (!map->extract_mesh_indexed(dir + "mesh_indexed.ply")) throw std::runtime_error("cannot write the indexed mesh");
        int64_t nv = 0, nf = 0, nt = 0;
        if (gsdf_extract_mesh_indexed(map->handle(), 0.f, nullptr, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) != GSDF_OK ||
            gsdf_extract_mesh(map->handle(), 0.f, nullptr, nullptr, 0, &nt) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        if (nf != nt) throw std::runtime_error("the indexed mesh and the soup differ in their face count");
        std::vector<float> v((size_t)nv * 3), nr((size_t)nv * 3);
        std::vector<int32_t> f((size_t)nf * 3);
        if (gsdf_extract_mesh_indexed(map->handle(), 0.f, nullptr, v.data(), nr.data(), f.data(), nv, nf, &nv, &nf) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        std::vector<char> used((size_t)nv, 0);
        for (int64_t i = 0; i < nf; ++i) {
            const int32_t a = f[3 * i], b = f[3 * i + 1], c = f[3 * i + 2];
            if (a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) throw std::runtime_error("a vertex id outside [0, n_vertices)");
            if (a == b || a == c || b == c) throw std::runtime_error("a face names a vertex twice");
            used[a] = used[b] = used[c] = 1;
        }
        for (char u : used) if (!u) throw std::runtime_error("a vertex no face uses");
        std::vector<int32_t> keys;
        std::vector<float> payload;
        map->export_arrays(keys, payload);
        if (!write_bin(dir + "map_keys.bin", keys) || !write_bin(dir + "map_payload.bin", payload) || !write_bin(dir + "mesh_v.bin", v) ||
            !write_bin(dir + "mesh_n.bin", nr) || !write_bin(dir + "mesh_f.bin", f))
            throw std::runtime_error("cannot write the dump files");
        std::printf("voxels %zu vertices %lld faces %lld\n", keys.size() / 3, (long long)nv, (long long)nf);
    } catch (const std::exception& e) {
        std::cerr << "indexed_mesh_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("indexed_mesh_selftest: OK\n");
    return 0;
}
