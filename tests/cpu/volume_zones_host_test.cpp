// The host half of the volume zones (csrc/volume_zones.cpp with MIUNET_NO_DEVICE: mi_unet_volume_zones_host and the two feature
// functions) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_zones_host_test.cpp <csrc>/volume_zones.cpp
// Cases: a 4 x 4 image worked by hand; 5 x 7 x 9 (odd sizes) with a box, a row that reaches both ends, the last voxel of the volume and
// ids that belong to no component; exact-size buffers (an overrun is the sanitizer's to find); each output NULL; a list that is cut;
// clamping; the features; refused calls.  The numbers are checked against facts that hold by construction;
// tests/test_volume_zones_cpu.py compares the same entry points with the reference.
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
    {   // one slice; levels are the values; the tables are worked out in tests/volume_zones_ref.py
        const uint16_t img[16] = { 0, 0, 1, 1, 0, 0, 1, 2, 3, 1, 2, 2, 3, 3, 2, 2 };
        const int32_t ids[16] = { 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 };
        const uint32_t want[4][4] = { { 4, 6, 0, 0 }, { 9, 2, 1, 0 }, { 5, 6, 1, 0 }, { 6, 3, 0, 0 } };
        const uint32_t hist[4] = { 4, 4, 5, 3 };
        const mi_unet_vzone zone_want[4] = { { 0, 0, 0, 4 }, { 2, 0, 1, 4 }, { 7, 0, 2, 5 }, { 8, 0, 3, 3 } };
        const mi_unet_vzones_opts o = { MI_UNET_VTEX_WIDTH, 4, 0, 1, 4 };
        mi_unet_vzones t;
        uint32_t rlm[16], axial[16];
        mi_unet_vzone zones[6];
        int found = -1;
        CHECK(mi_unet_volume_zones_host(ids, img, 1, 4, 4, 1, &o, &t, rlm, axial, zones, 6, &found) == MI_UNET_OK);
        for (int l = 0; l < 4; ++l)
            for (int j = 0; j < 4; ++j) CHECK(axial[l * 4 + j] == want[l][j] && rlm[l * 4 + j] == want[l][j] + (j ? 0 : 9 * hist[l]));
        CHECK(found == 4 && std::memcmp(zones, zone_want, sizeof zone_want) == 0);
        CHECK(zones[4].size == 0 && zones[5].first == 0 && zones[5].size == 0);
        CHECK(t.voxels == 16 && t.imin == 0 && t.imax == 3 && t.longest_run == 3 && t.zones == 4 && t.largest_zone == 5);
        CHECK(t.runs_axial == 43 && t.runs == 43 + 9 * 16 && t.clamped == 0 && t.clamped_axial == 0);
        mi_unet_vzone_features f;
        CHECK(mi_unet_volume_zones_run_features(&t, axial, 4, 4, 4, &f) == MI_UNET_OK);
        CHECK(std::fabs(f.percentage - 43.0 / 64.0) < 1e-15);
        CHECK(std::fabs(f.short_emphasis - (24.0 + 17.0 / 4.0 + 2.0 / 9.0) / 43.0) < 1e-15);         // 24 runs of 1, 17 of 2, 2 of 3
        CHECK(std::fabs(f.long_emphasis - (24.0 + 17.0 * 4.0 + 2.0 * 9.0) / 43.0) < 1e-15);
        CHECK(std::fabs(f.grey_nonuniformity - (100.0 + 144.0 + 144.0 + 81.0) / 43.0) < 1e-13);       // 10, 12, 12 and 9 runs a level
        CHECK(mi_unet_volume_zones_zone_features(&t, zones, found, 0, 4, &f) == MI_UNET_OK);
        CHECK(f.percentage == 0.25 && f.entropy == 2.0 && f.grey_nonuniformity == 1.0 && f.size_nonuniformity == (4.0 + 1.0 + 1.0) / 4.0);
        CHECK(f.grey_variance == 1.25 && f.size_variance == 0.5);                                     // levels 1 .. 4; sizes 4, 4, 5, 3
        CHECK(mi_unet_volume_zones_zone_features(&t, zones, found, 1, 4, &f) == MI_UNET_OK && std::isnan(f.entropy) && std::isnan(f.percentage));
    }
    const int D = 5, H = 7, W = 9;
    const size_t n = (size_t)D * H * W;
    std::vector<int32_t> ids(n, 0);
    std::vector<uint16_t> inten(n, 500);
    auto at = [&](int z, int y, int x) -> int32_t & { return ids[((size_t)z * H + y) * W + x]; };
    for (int z = 1; z <= 2; ++z)
        for (int y = 1; y <= 3; ++y)
            for (int x = 1; x <= 4; ++x) at(z, y, x) = 1;               // a 2 x 3 x 4 box at one level
    for (int x = 0; x < W; ++x) at(4, 0, x) = 2;                        // a whole row: its neighbours would lie outside the volume
    at(4, 6, 8) = 3;                                                    // the last voxel of the volume
    at(0, 0, 0) = -1; at(0, 0, 1) = 5; at(0, 0, 2) = 4097;              // no component
    const int m = 4, L = 8, R = 4;
    const mi_unet_vzones_opts o = { MI_UNET_VTEX_COUNT, L, 0, 1, R };
    std::vector<mi_unet_vzones> t(m);
    std::vector<uint32_t> rlm((size_t)m * L * R), axial((size_t)m * L * R);
    std::vector<mi_unet_vzone> zones(3);
    int found = -1;
    CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, m, &o, t.data(), rlm.data(), axial.data(), zones.data(), 3, &found) == MI_UNET_OK);
    CHECK(found == 3 && zones[0].component == 0 && zones[0].size == 24 && zones[0].first == (1 * H + 1) * W + 1 && zones[0].level == 0);
    CHECK(zones[1].component == 1 && zones[1].size == 9 && zones[1].first == 4 * H * W && zones[2].component == 2 && zones[2].first == (int)n - 1);
    CHECK(t[0].voxels == 24 && t[0].longest_run == 4 && t[0].zones == 1 && t[0].largest_zone == 24 && t[0].clamped == 0);
    CHECK(t[1].voxels == 9 && t[1].longest_run == 9 && t[1].clamped == 1 && t[1].clamped_axial == 1 && t[1].runs == 1 + 12 * 9 && t[1].runs_axial == 1 + 3 * 9);
    CHECK(rlm[(size_t)(1 * L + 0) * R + 3] == 1 && rlm[(size_t)(1 * L + 0) * R + 0] == 12 * 9);
    CHECK(t[2].voxels == 1 && t[2].runs == 13 && t[2].runs_axial == 4 && t[2].longest_run == 1 && t[2].imin == 500);
    CHECK(t[3].voxels == 0 && t[3].runs == 0 && t[3].zones == 0 && t[3].imin == 0 && t[3].imax == 0);
    {   // along x the box holds 2 * 3 runs of 4; every row of its table adds up to the entry
        CHECK(axial[(size_t)(0 * L + 0) * R + 3] >= 6);
        for (int r = 0; r < m; ++r) {
            int64_t sum = 0, sum_a = 0;
            for (int c = 0; c < L * R; ++c) { sum += rlm[(size_t)r * L * R + c]; sum_a += axial[(size_t)r * L * R + c]; }
            CHECK(sum == t[r].runs && sum_a == t[r].runs_axial);
        }
    }
    {   // each output NULL; a list of one; the same entries otherwise
        std::vector<mi_unet_vzones> u(m);
        mi_unet_vzone one;
        int f2 = -1;
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, m, &o, u.data(), nullptr, axial.data(), &one, 1, &f2) == MI_UNET_OK);
        CHECK(f2 == 3 && one.size == 24 && u[1].runs == 0 && u[1].clamped == 0 && u[1].longest_run == 0 && u[1].runs_axial == 28 && u[1].zones == 1);
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, m, &o, u.data(), rlm.data(), nullptr, nullptr, 0, nullptr) == MI_UNET_OK);
        CHECK(u[1].runs == 109 && u[1].runs_axial == 0 && u[1].clamped_axial == 0 && u[1].zones == 0 && u[1].largest_zone == 0 && u[1].longest_run == 9);
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, m, nullptr, u.data(), nullptr, nullptr, nullptr, 0, nullptr) == MI_UNET_OK);
        CHECK(u[0].voxels == 24 && u[0].runs == 0 && u[0].zones == 0);
    }
    {   // refused calls write nothing
        mi_unet_vzones poison;
        std::memset(&poison, 0x55, sizeof poison);
        mi_unet_vzones u = poison;
        int f2 = 77;
        mi_unet_vzone z;
        const mi_unet_vzones_opts bad_run = { 0, 8, 0, 1, 1 }, bad_cells = { 0, 64, 0, 1, 8192 };
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, 1, &bad_run, &u, nullptr, nullptr, nullptr, 0, nullptr) == MI_UNET_EARG);
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, 9, &bad_cells, &u, nullptr, nullptr, nullptr, 0, nullptr) == MI_UNET_EARG);
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, 1, nullptr, &u, nullptr, nullptr, &z, 1, nullptr) == MI_UNET_EARG);
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, 1, nullptr, &u, nullptr, nullptr, nullptr, 1, &f2) == MI_UNET_EARG);
        CHECK(mi_unet_volume_zones_host(ids.data(), inten.data(), D, H, W, 1, nullptr, &u, nullptr, nullptr, &z, 0, &f2) == MI_UNET_EARG);
        CHECK(miunet::g_err.rfind("mi_unet_volume_zones_host:", 0) == 0 && f2 == 77 && std::memcmp(&u, &poison, sizeof u) == 0);
        mi_unet_vzone_features f;
        std::memset(&f, 0x55, sizeof f);
        const mi_unet_vzone_features fp = f;
        const mi_unet_vzone bad_level = { 0, 0, 8, 1 }, bad_size = { 0, 0, 0, 0 }, other = { 0, 1, 99, -5 };
        CHECK(mi_unet_volume_zones_zone_features(&t[0], &bad_level, 1, 0, 8, &f) == MI_UNET_EARG);
        CHECK(mi_unet_volume_zones_zone_features(&t[0], &bad_size, 1, 0, 8, &f) == MI_UNET_EARG);
        CHECK(mi_unet_volume_zones_zone_features(&t[3], zones.data(), 3, 3, 8, &f) == MI_UNET_EARG);          // no voxels
        CHECK(mi_unet_volume_zones_run_features(&t[0], rlm.data(), L, R, 5, &f) == MI_UNET_EARG);
        CHECK(mi_unet_volume_zones_run_features(&t[0], rlm.data(), L, 1, 13, &f) == MI_UNET_EARG);
        CHECK(std::memcmp(&f, &fp, sizeof f) == 0);
        CHECK(mi_unet_volume_zones_zone_features(&t[0], &other, 1, 0, 8, &f) == MI_UNET_OK && std::isnan(f.entropy));    // a record of another component is not read
    }
    std::printf("volume_zones_host_test ok\n");
    return 0;
}
