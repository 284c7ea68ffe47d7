/*
 * erase_selftest -- the take-out round trip of the selection entries from C++ through the facade: fuse a few frames, select a box
 * of the map (MapGradPixelSdf::select_box, or MapPixelSdf's with `base`), take the members out (select_export with raw sums),
 * erase_selected, compact, and put them back with gsdf_merge_raw.  Checked here, in bytes: the export after the erase is the old
 * one minus the members; compact leaves it unchanged and drops the emptied blocks; after the merge the keys are the old ones and
 * the sums equal as floats, with equal bits except the sign of a zero (0 + (-0) is +0).  Also: a selection is lost when the
 * table grows.  Needs a GPU; tests/test_gpu_erase.py writes the inputs.
 *
 *   erase_selftest <dir> W H n voxel_size trunc_voxels [base]
 *   reads  <dir>/K.bin (9 f32)  depth.bin (n*H*W f32)  poses.bin (n*16 f32)
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct RawMap { std::vector<int32_t> keys; std::vector<float> pay; };
static RawMap export_raw(const MapGradPixelSdf& m) {
    RawMap r;
    int64_t n = m.size(), got = 0;
    r.keys.resize((size_t)n * 3);
    r.pay.resize((size_t)n * 5);
    if (n && gsdf_export(m.handle(), r.keys.data(), r.pay.data(), n, &got, 1, 1) != GSDF_OK) throw std::runtime_error(gsdf_last_error());
    return r;
}
template <class T>
static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static void require(bool ok, const char* what) { if (!ok) throw std::runtime_error(what); }

int main(int argc, char** argv) {
    if (argc < 7) { std::cerr << "usage: erase_selftest <dir> W H n voxel_size trunc_voxels [base]" << std::endl; return 2; }
    const std::string dir = std::string(argv[1]) + "/";
    const int W = atoi(argv[2]), H = atoi(argv[3]), n = atoi(argv[4]);
    const float vs = (float)atof(argv[5]), trunc = (float)atof(argv[6]);
    const bool base = argc > 7 && std::string(argv[7]) == "base";
    const size_t N = (size_t)W * H;
    std::vector<float> Kb, depth, P;
    if (!read_bin(dir + "K.bin", Kb, 9) || !read_bin(dir + "depth.bin", depth, n * N) || !read_bin(dir + "poses.bin", P, (size_t)n * 16)) {
        std::cerr << "erase_selftest: cannot read the inputs in " << dir << std::endl;
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
        const RawMap before = export_raw(*map);
        const size_t nvox = before.keys.size() / 3;
        require(nvox > 1000, "the map is too small for the round trip");
        /* the box: the middle third of the map's extent in x, faces on voxel centres (closed comparison) */
        int lo_i = before.keys[0], hi_i = before.keys[0];
        for (size_t i = 0; i < nvox; ++i) { lo_i = std::min(lo_i, before.keys[3 * i]); hi_i = std::max(hi_i, before.keys[3 * i]); }
        const int a = lo_i + (hi_i - lo_i) / 3, b = lo_i + 2 * (hi_i - lo_i) / 3;
        const float inf = 1e30f;
        int64_t n_sel = 0, n_cnt = 0, n_cnt_blocks = 0;
        require(map->select_box(Vec3f(vs * (float)a, -inf, -inf), Vec3f(vs * (float)b, inf, inf), GSDF_SEL_REPLACE, &n_sel), gsdf_last_error());
        require(map->select_count(&n_cnt, &n_cnt_blocks) && n_cnt == n_sel, "select_count disagrees with select_box");
        /* what the box must hold, from the export */
        RawMap want, rest;
        for (size_t i = 0; i < nvox; ++i) {
            RawMap& to = (before.keys[3 * i] >= a && before.keys[3 * i] <= b) ? want : rest;
            to.keys.insert(to.keys.end(), before.keys.begin() + (long)(3 * i), before.keys.begin() + (long)(3 * i + 3));
            to.pay.insert(to.pay.end(), before.pay.begin() + (long)(5 * i), before.pay.begin() + (long)(5 * i + 5));
        }
        require(!want.keys.empty() && !rest.keys.empty(), "the box holds nothing or everything");
        RawMap taken;
        require(map->select_export(taken.keys, taken.pay, true), gsdf_last_error());
        require(same_bytes(taken.keys, want.keys) && same_bytes(taken.pay, want.pay), "select_export is not the box's part of the export");
        int64_t n_erased = 0, n_emptied = 0, n_dropped = 0;
        require(map->erase_selected(&n_erased, &n_emptied), gsdf_last_error());
        require(n_erased == n_sel && n_emptied > 0 && n_emptied <= n_cnt_blocks, "erase_selected's counts");
        require(map->select_count(&n_cnt) && n_cnt == 0, "the selection is not none after the erase");
        RawMap after = export_raw(*map);
        require(same_bytes(after.keys, rest.keys) && same_bytes(after.pay, rest.pay), "the export after the erase is not the old one minus the members");
        require(map->compact(0, &n_dropped), gsdf_last_error());
        require(n_dropped == n_emptied, "compact did not drop the emptied blocks");
        after = export_raw(*map);
        require(same_bytes(after.keys, rest.keys) && same_bytes(after.pay, rest.pay), "compact changed the export");
        require(gsdf_merge_raw(map->handle(), taken.keys.data(), taken.pay.data(), (int64_t)(taken.keys.size() / 3)) == GSDF_OK, gsdf_last_error());
        after = export_raw(*map);
        require(same_bytes(after.keys, before.keys), "the keys after the put-back differ");
        for (size_t i = 0; i < after.pay.size(); ++i) {
            uint32_t x, y;
            std::memcpy(&x, &after.pay[i], 4);
            std::memcpy(&y, &before.pay[i], 4);
            require(after.pay[i] == before.pay[i] && (x == y || (before.pay[i] == 0.f && (x ^ y) == 0x80000000u)), "a sum changed in the round trip");
        }
        /* a rehash loses the selection; clear starts over */
        require(map->select_weight(0.f, inf), gsdf_last_error());
        require(gsdf_grow(map->handle(), 19) == GSDF_OK, gsdf_last_error());
        require(!map->select_count(&n_cnt) && std::string(gsdf_last_error()).find("lost") != std::string::npos, "the selection survived gsdf_grow");
        require(map->select_clear() && map->select_count(&n_cnt) && n_cnt == 0, "select_clear");
        std::printf("voxels %zu taken %lld blocks emptied %lld\n", nvox, (long long)n_erased, (long long)n_emptied);
    } catch (const std::exception& e) {
        std::cerr << "erase_selftest: " << e.what() << std::endl;
        return 1;
    }
    std::printf("erase_selftest: OK\n");
    return 0;
}
