/*
 * mesh_components_selftest -- runs the connected components of the indexed mesh (gsdf_mesh_components) and the filtered mesh
 * (gsdf_extract_mesh_indexed_filtered) from C++ through the facade: fuse a few frames, MapGradPixelSdf::mesh_components and
 * ::extract_mesh_indexed(filename, min_faces) (or MapPixelSdf's, with `base`).  Needs a GPU; tests/test_gpu_mesh_components.py
 * writes the inputs and compares the dumps and the PLY with the numpy restatement (tests/mesh_components_ref.py) of the map this
 * program exports.
 *
 *   mesh_components_selftest <dir> W H n voxel_size trunc_voxels min_faces|largest [base]
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)
 *   writes <dir>/mesh_indexed_clean.ply, components.txt, the map: map_keys.bin (m*3 i32), map_payload.bin (m*5 f32), in
 *          gsdf_export's sorted order, and the component arrays: comp_v.bin (nv i32), comp_f.bin (nf i32), comp_counts.bin
 *          (C*2 i32), comp_bbox.bin (C*6 f32)
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
    if (argc < 8) { std::cerr << "usage: mesh_components_selftest <dir> W H n voxel_size trunc_voxels min_faces|largest [base]" << std::endl; return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const int64_t min_faces = std::string(argv[7]) == "largest" ? (int64_t)GSDF_MESH_KEEP_LARGEST : (int64_t)atoll(argv[7]);
    const bool base = argc > 8 && std::string(argv[8]) == "base";
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, P;
    if (!read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) || !read_bin(dir + "poses.bin", P, (size_t)n * 16)) {
        std::cerr << "mesh_components_selftest: cannot read the inputs in " << dir << std::endl;
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
        MapGradPixelSdf::MeshComponents cc;
        if (!map->mesh_components(cc)) throw std::runtime_error(gsdf_last_error());
        if (!map->save_mesh_components(dir + "components.txt")) throw std::runtime_error("cannot write the component table");
        long n_comp = 0, n_kept = 0, n_faces = 0, n_all = 0;
        if (!map->extract_mesh_indexed(dir + "mesh_indexed_clean.ply", min_faces, &n_comp, &n_kept, &n_faces, &n_all))
            throw std::runtime_error("cannot write the filtered mesh");
        /* what must hold whatever the map is: the tables add up, a face lies in the component of each of its vertices */
        int64_t nv = 0, nf = 0;
        if (gsdf_extract_mesh_indexed(map->handle(), 0.f, nullptr, nullptr, nullptr, nullptr, 0, 0, &nv, &nf) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        std::vector<float> v((size_t)nv * 3);
        std::vector<int32_t> f((size_t)nf * 3);
        if (gsdf_extract_mesh_indexed(map->handle(), 0.f, nullptr, v.data(), nullptr, f.data(), nv, nf, &nv, &nf) != GSDF_OK)
            throw std::runtime_error(gsdf_last_error());
        if ((int64_t)cc.vertex_comp.size() != nv || (int64_t)cc.face_comp.size() != nf || n_comp != (long)cc.n_components || n_all != (long)nf)
            throw std::runtime_error("the component arrays do not fit the indexed mesh");
        long long sum_f = 0, sum_v = 0;
        for (int64_t i = 0; i < cc.n_components; ++i) { sum_f += cc.counts[2 * i]; sum_v += cc.counts[2 * i + 1]; }
        if (sum_f != nf || sum_v != nv) throw std::runtime_error("the component counts do not add up to the mesh");
        for (int64_t i = 0; i < nf; ++i)
            for (int k = 0; k < 3; ++k)
                if (cc.vertex_comp[(size_t)f[3 * i + k]] != cc.face_comp[(size_t)i]) throw std::runtime_error("a face lies in two components");
        if (nv > 0 && cc.vertex_comp[0] != 0) throw std::runtime_error("vertex 0 is not in component 0");
        std::vector<int32_t> keys;
        std::vector<float> payload;
        map->export_arrays(keys, payload);
        if (!write_bin(dir + "map_keys.bin", keys) || !write_bin(dir + "map_payload.bin", payload) || !write_bin(dir + "comp_v.bin", cc.vertex_comp) ||
            !write_bin(dir + "comp_f.bin", cc.face_comp) || !write_bin(dir + "comp_counts.bin", cc.counts) || !write_bin(dir + "comp_bbox.bin", cc.bbox))
            throw std::runtime_error("cannot write the dump files");
        std::printf("voxels %zu vertices %lld faces %lld\n", keys.size() / 3, (long long)nv, (long long)nf);
        std::printf("Mesh components: %ld, kept %ld, faces %ld of %ld\n", n_comp, n_kept, n_faces, n_all);
    } catch (const std::exception& e) {
        std::cerr << "mesh_components_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("mesh_components_selftest: OK\n");
    return 0;
}
