// The host half of the volume components (csrc/volume.cpp with MIUNET_NO_DEVICE: mi_unet_volume_components_host and
// mi_unet_volume_derive) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_host_test.cpp <csrc>/volume.cpp
// Cases: 5 x 9 x 13 (odd sizes) with two values, three connectivities, a filter, a table shorter than the plane, out aliasing masks, the
// empty volume, a refused call.  The numbers are checked against facts that hold by construction; tests/test_volume_cpu.py compares the
// same entry points with the reference.
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
    const int D = 5, H = 9, W = 13;
    const size_t n = (size_t)D * H * W;
    std::vector<uint8_t> vol(n, 0);
    auto at = [&](int z, int y, int x) -> uint8_t & { return vol[((size_t)z * H + y) * W + x]; };
    for (int z = 0; z < 2; ++z)
        for (int y = 0; y < 3; ++y)
            for (int x = 0; x < 4; ++x) at(z, y, x) = 1;                 // 24 voxels at the origin
    for (int z = 2; z < 4; ++z)
        for (int y = 3; y < 6; ++y)
            for (int x = 4; x < 8; ++x) at(z, y, x) = 1;                 // 24 voxels, touching the first block at one corner only
    at(4, 8, 12) = 1;                                                   // the last voxel of the volume
    at(2, 8, 12) = 2; at(3, 0, 0) = 2;                                  // the end of a slice and the start of the next one
    const int values[2] = { 1, 2 };
    for (int conn : { 6, 18, 26 }) {
        const mi_unet_volume_opts o{ conn, 0, 0 };
        std::vector<uint8_t> out(2 * n);
        std::vector<int32_t> ids(2 * n);
        mi_unet_vcomp table[2][4];
        int32_t found[2], kept[2];
        CHECK(mi_unet_volume_components_host(vol.data(), D, H, W, values, 2, &o, out.data(), ids.data(), &table[0][0], 4, found, kept) == MI_UNET_OK);
        CHECK(found[0] == (conn == 26 ? 2 : 3) && kept[0] == found[0] && found[1] == 2 && kept[1] == 2);
        CHECK(table[0][0].voxels == (conn == 26 ? 48 : 24) && table[0][0].first == 0 && table[0][0].value == 1 && table[0][0].kept == 1);
        CHECK(table[0][found[0] - 1].voxels == 1 && table[0][found[0] - 1].first == (int32_t)n - 1);
        CHECK(table[0][3].voxels == 0 && table[0][3].value == 0);                                   // all-zero behind the plane's components
        CHECK(table[1][0].voxels == 1 && table[1][0].first == (2 * H + 8) * W + 12 && table[1][1].first == 3 * H * W);
        CHECK(std::memcmp(out.data(), vol.data(), n) != 0 && out[0] == 1 && out[n + (2 * H + 8) * W + 12] == 2 && out[n] == 0);
        CHECK(ids[0] == 1 && ids[n - 1] == found[0] && ids[n + 3 * H * W] == 2 && ids[1 * H * W] == 1);
        if (conn == 6) {
            CHECK(table[0][0].faces_x == 2 * 2 * 3 && table[0][0].faces_y == 2 * 2 * 4 && table[0][0].faces_z == 2 * 3 * 4);
            CHECK(table[0][0].sx == 24 * 3 / 2 && table[0][0].x1 == 3 && table[0][0].y1 == 2 && table[0][0].z1 == 1 && table[0][1].z0 == 2);
        }
    }
    {   // keep the largest across the size tie, into a table of one, out aliasing masks
        std::vector<uint8_t> io(vol);
        const int one[1] = { 1 };
        const mi_unet_volume_opts o{ 18, 2, 1 };
        mi_unet_vcomp t;
        int32_t found = -1, kept = -1;
        CHECK(mi_unet_volume_components_host(io.data(), D, H, W, one, 1, &o, io.data(), nullptr, &t, 1, &found, &kept) == MI_UNET_OK);
        CHECK(found == 3 && kept == 1 && t.voxels == 24 && t.first == 0 && t.kept == 1);
        size_t set = 0;
        for (uint8_t b : io) set += b == 1;
        CHECK(set == 24 && io[0] == 1 && io[n - 1] == 0 && io[(2 * H + 8) * W + 12] == 0);
        mi_unet_vcomp_metrics m;
        const double sp[3] = { 0.7, 0.7, 3.0 };
        CHECK(mi_unet_volume_derive(&t, sp, &m) == MI_UNET_OK && m.volume_mm3 == 24.0 * 0.7 * 0.7 * 3.0 && m.extent_z_mm == 6.0);
        CHECK(m.cx_mm == (1.5 + 0.5) * 0.7 && m.cz_mm == (0.5 + 0.5) * 3.0);
        const double bad[3] = { 0.7, 0.0, 3.0 };
        CHECK(mi_unet_volume_derive(&t, bad, &m) == MI_UNET_EARG && mi_unet_volume_derive(nullptr, sp, &m) == MI_UNET_EARG);
    }
    {   // the empty volume, default options
        std::vector<uint8_t> none(n, 0), out(n, 9);
        mi_unet_vcomp t[2];
        std::memset(t, 0x55, sizeof t);
        int32_t found = -1, kept = -1;
        const int one[1] = { 1 };
        CHECK(mi_unet_volume_components_host(none.data(), D, H, W, one, 1, nullptr, out.data(), nullptr, t, 2, &found, &kept) == MI_UNET_OK);
        CHECK(found == 0 && kept == 0 && t[0].voxels == 0 && t[1].sz == 0 && out[0] == 0 && out[n - 1] == 0);
    }
    mi_unet_vcomp keep;
    std::memset(&keep, 0x55, sizeof keep);
    int32_t found = 77, kept = 77;
    const int twice[2] = { 1, 1 };
    CHECK(mi_unet_volume_components_host(vol.data(), D, H, W, twice, 2, nullptr, nullptr, nullptr, &keep, 1, &found, &kept) == MI_UNET_EARG);
    CHECK(reinterpret_cast<const uint8_t *>(&keep)[0] == 0x55 && found == 77 && !miunet::g_err.empty());
    std::printf("volume_host_test ok\n");
    return 0;
}
