// The host half of the volume skeleton (csrc/volume_skeleton.cpp with MIUNET_NO_DEVICE: mi_unet_volume_skeleton_host,
// mi_unet_volume_skeleton_derive and mi_unet_volume_skeleton_simple_host) as a stand-alone program, so that it can run under
// -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_skeleton_host_test.cpp <csrc>/volume_skeleton.cpp
// Cases: a 5 x 7 x 9 block that fills its volume (odd sizes, every face at the border) and thins to one voxel; a line, which stays as
// it is; a line with a second id beside it and values outside 1 .. m; anisotropic units and the layer of "nothing" round the volume; a
// stop after one pass; a few codes of the simple-point test; refused calls.  The numbers are checked against facts that hold by
// construction; tests/test_volume_skeleton_cpu.py compares the same entry points with the reference.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_unet.h"

namespace miunet {
static std::string g_err;
int engine_fail(int code, const std::string &msg) { g_err = msg; return code; }
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main()
{
    const int units[3] = { 1, 1, 1 };
    {   // the full block: one component without a hole thins to one voxel, which is isolated
        const int D = 5, H = 7, W = 9;
        const size_t n = (size_t)D * H * W;
        std::vector<int32_t> ids(n, 1), out(n, -1), r2(n, -1);
        mi_unet_vskel t;
        mi_unet_vskel_info info;
        CHECK(mi_unet_volume_skeleton_host(ids.data(), D, H, W, 1, units, nullptr, out.data(), r2.data(), &t, &info) == MI_UNET_OK);
        CHECK(t.voxels_in == (int64_t)n && t.voxels == 1 && t.isolated == 1 && t.ends == 0 && t.junctions == 0);
        CHECK(info.stable == 1 && info.deleted == (int64_t)n - 1 && info.passes >= 2);
        int64_t left = 0, at = -1;
        for (size_t i = 0; i < n; ++i)
            if (out[i]) { ++left; at = (int64_t)i; CHECK(out[i] == 1 && r2[i] == t.r2_min); } else CHECK(r2[i] == 0);
        CHECK(left == 1 && t.r2_min == t.r2_max && t.r2_sum == t.r2_min);
        // the radius comes from the layer round the volume alone: the square of the distance to the nearest face
        const int z = (int)(at / (H * W)), y = (int)(at / W % H), x = (int)(at % W);
        const int dz = std::min(z + 1, D - z), dy = std::min(y + 1, H - y), dx = std::min(x + 1, W - x), dmin = std::min(dz, std::min(dy, dx));
        CHECK(t.r2_min == dmin * dmin);
        // thinning the skeleton again changes nothing and takes one pass; the voxel now stands alone: a radius of one step
        std::vector<int32_t> again(n, -1);
        mi_unet_vskel t2;
        CHECK(mi_unet_volume_skeleton_host(out.data(), D, H, W, 1, units, nullptr, again.data(), nullptr, &t2, &info) == MI_UNET_OK);
        CHECK(again == out && info.passes == 1 && info.deleted == 0 && info.stable == 1 && t2.voxels_in == 1 && t2.r2_min == 1 && t2.r2_max == 1);
        // one pass only: not stable, something is left to delete
        const mi_unet_vskel_opts one_pass{ 1, 0 };
        CHECK(mi_unet_volume_skeleton_host(ids.data(), D, H, W, 1, units, &one_pass, nullptr, nullptr, &t2, &info) == MI_UNET_OK);
        CHECK(info.passes == 1 && info.stable == 0 && t2.voxels > 1 && t2.voxels < (int64_t)n && t2.r2_min == 0 && t2.r2_max == 0 && t2.r2_sum == 0);
    }
    {   // a line of 6 along x with id 2, a voxel of id 1 diagonally beside its end (no same-object neighbour of it), a value above m and
        // a negative one: nothing is deleted
        const int D = 3, H = 4, W = 8;
        const size_t n = (size_t)D * H * W;
        auto idx = [&](int z, int y, int x) { return ((size_t)z * H + y) * W + x; };
        std::vector<int32_t> ids(n, 0), out(n, -1), r2(n, -1);
        for (int x = 1; x < 7; ++x) ids[idx(1, 1, x)] = 2;
        ids[idx(2, 2, 7)] = 1;
        ids[idx(0, 3, 0)] = 5;
        ids[idx(0, 0, 0)] = -4;
        const int u[3] = { 2, 3, 5 };
        mi_unet_vskel t[3];
        mi_unet_vskel_info info;
        CHECK(mi_unet_volume_skeleton_host(ids.data(), D, H, W, 3, u, nullptr, out.data(), r2.data(), t, &info) == MI_UNET_OK);
        CHECK(info.passes == 1 && info.deleted == 0 && info.stable == 1);
        CHECK(t[1].voxels_in == 6 && t[1].voxels == 6 && t[1].ends == 2 && t[1].junctions == 0 && t[1].links[0] == 5 && t[1].links[1] == 0);
        CHECK(t[0].voxels == 1 && t[0].isolated == 1 && t[2].voxels_in == 0 && t[2].voxels == 0 && t[2].r2_min == 0 && t[2].r2_sum == 0);
        CHECK(out[idx(0, 3, 0)] == 0 && out[idx(0, 0, 0)] == 0 && out[idx(1, 1, 3)] == 2 && out[idx(2, 2, 7)] == 1);
        // every voxel of the line has a free x neighbour row: the nearest other voxel is one step in x (2), y (3) or z (5) away -> 4, but
        // at x = 6 the voxel of id 1 at (2, 2, 7) is sqrt(4 + 9 + 25) away and the y neighbour is nearer; the id-1 voxel is at the border: 2^2
        CHECK(t[1].r2_min == 4 && t[1].r2_max == 9 && r2[idx(1, 1, 1)] == 4 && r2[idx(1, 1, 3)] == 9 && t[0].r2_min == 4 && t[0].r2_max == 4);
        mi_unet_vskel_metrics m;
        const double sp[3] = { 0.5, 0.75, 1.25 };
        CHECK(mi_unet_volume_skeleton_derive(&t[1], sp, 0.25, &m) == MI_UNET_OK);
        CHECK(m.length_mm == 5 * 0.5 && m.loops == 0 && m.radius_min_mm == 2 * 0.25 && m.radius_max_mm == 3 * 0.25);
        CHECK(m.radius_rms_mm == std::sqrt((double)t[1].r2_sum / 6.0) * 0.25);
        CHECK(mi_unet_volume_skeleton_derive(&t[2], sp, 0.25, &m) == MI_UNET_OK && m.length_mm == 0 && m.loops == 0 && m.radius_rms_mm == 0);
        const double bad[3] = { 0.5, 0.0, 1.25 };
        CHECK(mi_unet_volume_skeleton_derive(&t[1], bad, 0.25, &m) == MI_UNET_EARG && mi_unet_volume_skeleton_derive(&t[1], sp, 0.0, &m) == MI_UNET_EARG);
        CHECK(mi_unet_volume_skeleton_derive(nullptr, sp, 0.25, &m) == MI_UNET_EARG);
    }
    {   // the simple-point test: no neighbour; one neighbour; two opposite face neighbours (the object falls apart); all 26 (no
        // background face neighbour); all but one face neighbour (a dent: simple); the first word as a whole
        uint32_t w = 0;
        auto simple = [&](uint32_t code) {
            uint32_t bits = 0;
            if (mi_unet_volume_skeleton_simple_host(code >> 5, 1, &bits) != MI_UNET_OK) return -1;
            return (int)(bits >> (code & 31) & 1u);
        };
        const uint32_t x_minus = 1u << 12, x_plus = 1u << 13, all = (1u << 26) - 1u;
        CHECK(simple(0) == 0 && simple(x_minus) == 1 && simple(x_minus | x_plus) == 0 && simple(all) == 0 && simple(all & ~x_plus) == 1);
        CHECK(mi_unet_volume_skeleton_simple_host(0, 1, &w) == MI_UNET_OK && (w & 1u) == 0 && (w >> 1 & 1u) == 1);
        CHECK(mi_unet_volume_skeleton_simple_host(1u << 21, 1, &w) == MI_UNET_EARG && mi_unet_volume_skeleton_simple_host(0, 0, &w) == MI_UNET_EARG);
        CHECK(mi_unet_volume_skeleton_simple_host(0, 1, nullptr) == MI_UNET_EARG);
    }
    std::vector<int32_t> ids(2 * 3 * 4, 1);
    mi_unet_vskel keep;
    std::memset(&keep, 0x55, sizeof keep);
    mi_unet_vskel_info info{ 7, 7, 7 };
    const int zero_unit[3] = { 1, 0, 1 }, big_unit[3] = { 1, 1, 15447 };      // (3 * 15447 = 46341)
    const mi_unet_vskel_opts bad_passes{ -1, 1 }, bad_radius{ 0, 2 };
    CHECK(mi_unet_volume_skeleton_host(nullptr, 2, 3, 4, 1, units, nullptr, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(mi_unet_volume_skeleton_host(ids.data(), 0, 3, 4, 1, units, nullptr, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(mi_unet_volume_skeleton_host(ids.data(), 2, 3, 4, 0, units, nullptr, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(mi_unet_volume_skeleton_host(ids.data(), 2, 3, 4, 4097, units, nullptr, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(mi_unet_volume_skeleton_host(ids.data(), 2, 3, 4, 1, zero_unit, nullptr, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(mi_unet_volume_skeleton_host(ids.data(), 2, 3, 4, 1, big_unit, nullptr, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(mi_unet_volume_skeleton_host(ids.data(), 2, 3, 4, 1, units, &bad_passes, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(mi_unet_volume_skeleton_host(ids.data(), 2, 3, 4, 1, units, &bad_radius, nullptr, nullptr, &keep, &info) == MI_UNET_EARG);
    CHECK(reinterpret_cast<const uint8_t *>(&keep)[0] == 0x55 && info.passes == 7 && miunet::g_err.rfind("mi_unet_volume_skeleton_host:", 0) == 0);
    std::printf("volume_skeleton_host_test ok\n");
    return 0;
}
