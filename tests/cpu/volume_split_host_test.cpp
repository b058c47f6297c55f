// The host half of the volume split (csrc/volume_split.cpp with MIUNET_NO_DEVICE: mi_unet_volume_split_host and
// mi_unet_volume_split_derive) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_split_host_test.cpp <csrc>/volume_split.cpp
// Cases: two 5 x 5 x 5 blocks of a 5 x 7 x 15 volume (odd sizes) joined by a bridge of one voxel's width, split by a ball of radius 1
// under every connectivity and under two spacings; the identity; cores that are dropped; a table shorter than the plane; a second
// value; the empty plane; refused calls.  The numbers are checked against facts that hold by construction; tests/test_volume_split_cpu.py
// compares the same entry points with the reference.
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
    const int D = 5, H = 7, W = 15;
    const size_t n = (size_t)D * H * W;
    std::vector<uint8_t> vol(n, 0);
    auto idx = [&](int z, int y, int x) { return ((size_t)z * H + y) * W + x; };
    for (int z = 0; z < 5; ++z)
        for (int y = 1; y < 6; ++y)
            for (int x = 0; x < 5; ++x) vol[idx(z, y, x)] = vol[idx(z, y, x + 10)] = 1;     // two blocks of 125 voxels
    for (int x = 5; x < 10; ++x) vol[idx(2, 3, x)] = 1;                                   // the bridge: 5 voxels
    vol[idx(0, 0, 14)] = 2;                                                               // one voxel of a second value
    const int values[2] = { 1, 2 }, units[3] = { 1, 1, 1 };
    for (int conn : { 6, 18, 26 }) {
        const mi_unet_vsplit_opts o{ conn, 1, 1 };
        std::vector<int32_t> ids(2 * n);
        mi_unet_vcomp table[2][4];
        mi_unet_vpiece info[2][4];
        mi_unet_vsplit_stat st[2];
        int32_t found[2], rounds[2] = { 9, 9 };
        CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, values, 2, units, &o, ids.data(), &table[0][0], &info[0][0], 4, found, st, rounds) == MI_UNET_OK);
        // the ball of radius 1 is the 6-neighbourhood and only voxels inside the volume constrain (x = 0, x = 14 and z = 0, 4 are
        // faces of the volume): the left core is x 0..3, y 2..4, z 0..4 = 60 voxels and the block's voxel at the bridge, whose
        // neighbour on the bridge is set; the right core is its mirror image; no voxel of the bridge stays
        CHECK(found[0] == 2 && st[0].cores == 2 && st[0].cores_kept == 2 && st[0].coreless == 0 && st[0].pieces == 2);
        CHECK(st[0].in_voxels == 255 && st[0].core_voxels == 122 && st[0].value == 1 && rounds[0] == 0);
        // the bridge's voxels x = 5..9 lie 1, 2, 3 from the left core and 3, 2, 1 from the right: the middle one ties and goes to
        // the smaller marker: the left piece has 125 + 3, the right 125 + 2
        CHECK(table[0][0].voxels == 128 && table[0][1].voxels == 127 && table[0][0].first == (int32_t)idx(0, 1, 0) && table[0][0].kept == 1);
        CHECK(table[0][0].x1 == 7 && table[0][1].x0 == 8 && table[0][2].voxels == 0 && table[0][0].value == 1);
        CHECK(info[0][0].core_voxels == 61 && info[0][0].core_first == (int32_t)idx(0, 2, 0) && info[0][0].reach == 3 && info[0][1].reach == 2);
        CHECK(info[0][0].cut_x == 1 && info[0][1].cut_x == 1 && info[0][0].cut_y == 0 && info[0][0].cut_z == 0);
        CHECK(ids[idx(2, 3, 7)] == 1 && ids[idx(2, 3, 8)] == 2 && ids[idx(0, 0, 0)] == 0 && ids[idx(4, 5, 14)] == 2);
        // the second value: a single voxel, whose erosion by the 6-neighbourhood is empty (its neighbours inside the volume are not
        // set): a coreless piece
        CHECK(found[1] == 1 && st[1].cores == 0 && st[1].coreless == 1 && info[1][0].core_first == -1 && table[1][0].voxels == 1);
        CHECK(table[1][0].faces_x == 2 && info[1][0].cut_x == 0 && ids[n + idx(0, 0, 14)] == 1 && ids[n] == 0);
    }
    {   // anisotropic: B(5) under (3, 4, 5) is the 6-neighbourhood and the four diagonals in x and y, so the block's voxel at the
        // bridge is no core; a step in x costs 3: the bridge's voxels lie 6 .. 18 from the left core's x = 3, the tie is at 12
        const int u[3] = { 3, 4, 5 }, one[1] = { 1 };
        const mi_unet_vsplit_opts o{ 6, 5, 1 };
        mi_unet_vcomp t[2];
        mi_unet_vpiece p[2];
        mi_unet_vsplit_stat st;
        int32_t found = -1;
        CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, u, &o, nullptr, t, p, 2, &found, &st, nullptr) == MI_UNET_OK);
        CHECK(found == 2 && t[0].voxels == 128 && t[1].voxels == 127 && p[0].reach == 12 && p[1].reach == 9 && st.max_reach == 12);
        mi_unet_vpiece_metrics m;
        const double sp[3] = { 0.3, 0.4, 0.5 };
        CHECK(mi_unet_volume_split_derive(&p[0], sp, 0.1, &m) == MI_UNET_OK && m.reach_mm == 12 * 0.1 && m.cut_mm2 == 1 * 0.4 * 0.5);
        const double bad[3] = { 0.3, 0.0, 0.5 };
        CHECK(mi_unet_volume_split_derive(&p[0], bad, 0.1, &m) == MI_UNET_EARG && mi_unet_volume_split_derive(&p[0], sp, 0.0, &m) == MI_UNET_EARG);
        CHECK(mi_unet_volume_split_derive(nullptr, sp, 0.1, &m) == MI_UNET_EARG);
    }
    {   // the identity (default options): one piece, the component; then min_core above every core: one coreless piece
        const int one[1] = { 1 };
        mi_unet_vcomp t, c;
        mi_unet_vpiece p;
        int32_t found = -1;
        CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, units, nullptr, nullptr, &t, &p, 1, &found, nullptr, nullptr) == MI_UNET_OK);
        CHECK(found == 1 && t.voxels == 255 && p.core_voxels == 255 && p.reach == 0 && p.cut_x == 0 && p.core_first == t.first);
        c = t;
        const mi_unet_vsplit_opts o{ 26, 1, 62 };
        CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, units, &o, nullptr, &t, &p, 1, &found, nullptr, nullptr) == MI_UNET_OK);
        CHECK(found == 1 && std::memcmp(&t, &c, sizeof t) == 0 && p.core_first == -1 && p.core_voxels == 0 && p.reach == 0);
    }
    {   // a table of one under a plane of two pieces; the empty plane
        const int one[1] = { 1 }, three[1] = { 3 };
        const mi_unet_vsplit_opts o{ 18, 1, 1 };
        std::vector<int32_t> ids(n);
        mi_unet_vcomp t;
        int32_t found = -1;
        CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, units, &o, ids.data(), &t, nullptr, 1, &found, nullptr, nullptr) == MI_UNET_OK);
        CHECK(found == 2 && t.voxels == 128 && ids[idx(2, 3, 7)] == 1 && ids[idx(2, 3, 8)] == -1);
        std::memset(&t, 0x55, sizeof t);
        CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, three, 1, units, &o, ids.data(), &t, nullptr, 1, &found, nullptr, nullptr) == MI_UNET_OK);
        CHECK(found == 0 && t.voxels == 0 && t.sz == 0 && ids[idx(2, 3, 7)] == 0);
    }
    mi_unet_vcomp keep;
    std::memset(&keep, 0x55, sizeof keep);
    int32_t found = 77;
    const int twice[2] = { 1, 1 }, one[1] = { 1 }, zero_unit[3] = { 1, 0, 1 };
    const mi_unet_vsplit_opts bad_conn{ 7, 0, 1 }, bad_core{ 26, 0, -1 }, bad_neck{ 26, 46341, 1 };
    CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, twice, 2, units, nullptr, nullptr, &keep, nullptr, 1, &found, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, zero_unit, nullptr, nullptr, &keep, nullptr, 1, &found, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, units, &bad_conn, nullptr, &keep, nullptr, 1, &found, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, units, &bad_core, nullptr, &keep, nullptr, 1, &found, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, units, &bad_neck, nullptr, &keep, nullptr, 1, &found, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_volume_split_host(vol.data(), D, H, W, one, 1, units, nullptr, nullptr, &keep, nullptr, 0, &found, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(reinterpret_cast<const uint8_t *>(&keep)[0] == 0x55 && found == 77 && !miunet::g_err.empty());
    std::printf("volume_split_host_test ok\n");
    return 0;
}
