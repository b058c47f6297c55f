// The host half of the volume neighbourhoods (csrc/volume_nbhood.cpp with MIUNET_NO_DEVICE: mi_unet_volume_nbhood_host and
// mi_unet_volume_nbhood_derive) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_nbhood_host_test.cpp <csrc>/volume_nbhood.cpp
// Cases: a 4 x 4 image worked by hand; 5 x 7 x 9 (odd sizes) with a box, a row that reaches both ends, the last voxel of the volume and
// ids that belong to no component; exact-size buffers (an overrun is the sanitizer's to find); each output NULL; clamping; the
// features; refused calls.  The numbers are checked against facts that hold by construction; tests/test_volume_nbhood_cpu.py compares
// the same entry points with the reference.
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
    {   // one slice; levels are the values minus 1; the tables are worked out in tests/volume_nbhood_ref.py
        const uint16_t img[16] = { 0, 1, 1, 2, 0, 1, 2, 2, 3, 1, 3, 0, 3, 0, 1, 2 };
        const int32_t ids[16] = { 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 };
        const uint64_t diff_want[4][9] = { { 0, 0, 0, 2, 0, 27, 0, 0, 0 }, { 0, 0, 0, 0, 0, 5, 0, 0, 8 }, { 0, 0, 0, 3, 0, 2, 0, 0, 5 }, { 0, 0, 0, 5, 0, 10, 0, 0, 15 } };
        const uint32_t count_want[4][9] = { { 0, 0, 0, 1, 0, 3, 0, 0, 0 }, { 0, 0, 0, 0, 0, 3, 0, 0, 2 }, { 0, 0, 0, 2, 0, 1, 0, 0, 1 }, { 0, 0, 0, 1, 0, 1, 0, 0, 1 } };
        const mi_unet_vnbhood_opts o = { MI_UNET_VTEX_WIDTH, 4, 0, 1, 0, 2 };
        mi_unet_vnbhood t;
        uint32_t count[4 * 27], dep[4 * 27], count_a[4 * 9], dep_a[4 * 9], dzm[4 * 2], dzm_a[4 * 2];
        uint64_t diff[4 * 27], diff_a[4 * 9];
        const mi_unet_vnbhood_out out = { count, diff, dep, count_a, diff_a, dep_a, dzm, dzm_a };
        CHECK(mi_unet_volume_nbhood_host(ids, img, 1, 4, 4, 1, &o, &t, &out) == MI_UNET_OK);
        for (int l = 0; l < 4; ++l)
            for (int c = 0; c < 27; ++c) {
                CHECK(count[l * 27 + c] == (c < 9 ? count_want[l][c] : 0u) && diff[l * 27 + c] == (c < 9 ? diff_want[l][c] : 0u));
                if (c < 9) CHECK(count_a[l * 9 + c] == count_want[l][c] && diff_a[l * 9 + c] == diff_want[l][c] && dep_a[l * 9 + c] == dep[l * 27 + c]);
            }
        CHECK(dep[0 * 27 + 0] == 2 && dep[0 * 27 + 1] == 2 && dep[1 * 27 + 3] == 1 && dep[2 * 27 + 2] == 3 && dep[3 * 27 + 1] == 2);
        CHECK(t.voxels == 16 && t.imin == 0 && t.imax == 3 && t.valid == 16 && t.valid_axial == 16 && t.dependence_max == 4);
        CHECK(t.zones == 8 && t.deepest == 1 && t.deepest_axial == 2 && t.clamped == 0 && t.clamped_axial == 0);
        CHECK(dzm[0] == 3 && dzm[2] == 1 && dzm[4] == 2 && dzm[6] == 2 && dzm[1] + dzm[3] + dzm[5] + dzm[7] == 0);
        // in the slice only the four pixels in the middle lie 2 deep, and each belongs to a zone that reaches the border, except the 4
        // at (2, 2), a zone of its own
        CHECK(dzm_a[3 * 2 + 1] == 1 && dzm_a[3 * 2 + 0] == 1 && dzm_a[0] == 3 && dzm_a[1] == 0);
        mi_unet_vnbhood_features f;
        const mi_unet_vnbhood_out rows = out;                                       // (one component: its rows are the tables)
        CHECK(mi_unet_volume_nbhood_derive(&t, &rows, 4, 2, 1, &f) == MI_UNET_OK);
        CHECK(std::fabs(f.coarseness - 0.27122474925836) < 1e-13 && std::fabs(f.contrast - 0.18065863715277) < 1e-13);
        CHECK(std::fabs(f.busyness - 1.13445512820512) < 1e-13 && std::fabs(f.complexity - 5.20294725529100) < 1e-13);
        CHECK(std::fabs(f.strength - 1.21535181236673) < 1e-13 && f.dependence_energy == 34.0 / 256.0 && f.ngldm.percentage == 1.0);
        CHECK(f.gldzm.percentage == 0.5 && std::fabs(f.gldzm.long_emphasis - (7.0 + 4.0) / 8.0) < 1e-15);
        CHECK(mi_unet_volume_nbhood_derive(&t, &rows, 4, 2, 0, &f) == MI_UNET_OK && f.gldzm.long_emphasis == 1.0);
        const mi_unet_vnbhood_out none = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
        CHECK(mi_unet_volume_nbhood_derive(&t, &none, 4, 2, 0, &f) == MI_UNET_OK && std::isnan(f.coarseness) && std::isnan(f.ngldm.entropy) &&
              std::isnan(f.dependence_energy) && std::isnan(f.gldzm.percentage));
    }
    const int D = 5, H = 7, W = 9;
    const size_t n = (size_t)D * H * W;
    std::vector<int32_t> ids(n, 0);
    std::vector<uint16_t> inten(n, 500);
    auto at = [&](int z, int y, int x) -> int32_t & { return ids[((size_t)z * H + y) * W + x]; };
    for (int z = 1; z <= 3; ++z)
        for (int y = 1; y <= 5; ++y)
            for (int x = 1; x <= 7; ++x) at(z, y, x) = 1;               // a 3 x 5 x 7 box at one level: its centre lies 2 deep, in the slice 3
    for (int x = 0; x < W; ++x) at(4, 0, x) = 2;                        // a whole row at the volume's edge
    at(4, 6, 8) = 3;                                                    // the last voxel of the volume
    at(0, 0, 0) = -1; at(0, 0, 1) = 5; at(0, 0, 2) = 4097;              // no component
    const int m = 4, L = 8, Dm = 2;
    const mi_unet_vnbhood_opts o = { MI_UNET_VTEX_COUNT, L, 0, 1, 0, Dm };
    std::vector<mi_unet_vnbhood> t(m);
    std::vector<uint32_t> count((size_t)m * L * 27), dep((size_t)m * L * 27), count_a((size_t)m * L * 9), dep_a((size_t)m * L * 9);
    std::vector<uint64_t> diff((size_t)m * L * 27), diff_a((size_t)m * L * 9);
    std::vector<uint32_t> dzm((size_t)m * L * Dm), dzm_a((size_t)m * L * Dm);
    const mi_unet_vnbhood_out out = { count.data(), diff.data(), dep.data(), count_a.data(), diff_a.data(), dep_a.data(), dzm.data(), dzm_a.data() };
    CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, m, &o, t.data(), &out) == MI_UNET_OK);
    CHECK(t[0].voxels == 105 && t[0].valid == 105 && t[0].zones == 1 && t[0].deepest == 2 && t[0].deepest_axial == 3 && t[0].dependence_max == 27);
    CHECK(count[26] == 1 * 3 * 5 && dep[26] == 15 && count_a[8] == 3 * 3 * 5 && t[0].clamped == 0 && dzm[0] == 1 && dzm_a[0] == 1);
    CHECK(t[1].voxels == 9 && t[1].valid == 9 && count[(size_t)(1 * L) * 27 + 1] == 2 && count[(size_t)(1 * L) * 27 + 2] == 7 && t[1].deepest == 1);
    CHECK(t[2].voxels == 1 && t[2].valid == 0 && t[2].valid_axial == 0 && count[(size_t)(2 * L) * 27 + 0] == 1 && t[2].dependence_max == 1 && t[2].zones == 1);
    CHECK(t[3].voxels == 0 && t[3].zones == 0 && t[3].imin == 0 && t[3].imax == 0 && t[3].deepest == 0 && t[3].dependence_max == 0);
    for (size_t c = 0; c < diff.size(); ++c) CHECK(diff[c] == 0);                   // one level everywhere
    {   // each output NULL in turn; the entry's fields of the table that is missing are 0, the others what they were
        for (int skip = 0; skip < 6; ++skip) {
            mi_unet_vnbhood_out part = out;
            if (skip == 0) part.ngt_count = nullptr, part.ngt_diff = nullptr;
            if (skip == 1) part.dep = nullptr;
            if (skip == 2) part.ngt_count_axial = nullptr, part.ngt_diff_axial = nullptr;
            if (skip == 3) part.dep_axial = nullptr;
            if (skip == 4) part.dzm = nullptr;
            if (skip == 5) part.dzm_axial = nullptr;
            std::vector<mi_unet_vnbhood> u(m);
            CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, m, &o, u.data(), &part) == MI_UNET_OK);
            CHECK(u[0].voxels == 105 && u[0].valid == (skip == 0 ? 0 : 105) && u[0].dependence_max == (skip == 1 ? 0 : 27));
            CHECK(u[0].valid_axial == (skip == 2 ? 0 : 105) && u[0].deepest == (skip == 4 ? 0 : 2) && u[0].deepest_axial == (skip == 5 ? 0 : 3) && u[0].zones == 1);
        }
        std::vector<mi_unet_vnbhood> u(m);
        CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, m, nullptr, u.data(), nullptr) == MI_UNET_OK);
        CHECK(u[0].voxels == 105 && u[0].valid == 0 && u[0].zones == 0 && u[0].deepest == 0 && u[1].imin == 500);
    }
    {   // Dm = 1: the box is one zone at distance 1 and is not clamped; a voxel of another level in its centre is a zone 2 deep and is
        std::vector<uint16_t> two = inten;
        two[((size_t)2 * H + 3) * W + 4] = 9000;
        const mi_unet_vnbhood_opts o1 = { MI_UNET_VTEX_COUNT, L, 0, 1, 0, 1 };
        std::vector<uint32_t> z1((size_t)m * L), z1a((size_t)m * L);
        const mi_unet_vnbhood_out part = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, z1.data(), z1a.data() };
        std::vector<mi_unet_vnbhood> u(m);
        CHECK(mi_unet_volume_nbhood_host(ids.data(), two.data(), D, H, W, m, &o1, u.data(), &part) == MI_UNET_OK);
        CHECK(u[0].zones == 2 && u[0].clamped == 1 && u[0].clamped_axial == 1 && z1[0] == 1 && z1[L - 1] == 1 && u[0].imax == 9000);
    }
    {   // refused calls write nothing
        mi_unet_vnbhood poison;
        std::memset(&poison, 0x55, sizeof poison);
        mi_unet_vnbhood u = poison;
        const mi_unet_vnbhood_opts bad_alpha = { 0, 8, 0, 1, 8, 32 }, bad_dist = { 0, 8, 0, 1, 0, 4097 }, bad_cells = { 0, 64, 0, 1, 0, 4096 };
        uint32_t word = 77;
        const mi_unet_vnbhood_out lone = { &word, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
        CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, 1, &bad_alpha, &u, nullptr) == MI_UNET_EARG);
        CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, 1, &bad_dist, &u, nullptr) == MI_UNET_EARG);
        CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, 17, &bad_cells, &u, nullptr) == MI_UNET_EARG);
        CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, 1, nullptr, &u, &lone) == MI_UNET_EARG);
        CHECK(mi_unet_volume_nbhood_host(ids.data(), inten.data(), D, H, W, 1, nullptr, nullptr, nullptr) == MI_UNET_EARG);
        CHECK(miunet::g_err.rfind("mi_unet_volume_nbhood_host:", 0) == 0 && word == 77 && std::memcmp(&u, &poison, sizeof u) == 0);
        mi_unet_vnbhood_features f;
        std::memset(&f, 0x55, sizeof f);
        const mi_unet_vnbhood_features fp = f;
        CHECK(mi_unet_volume_nbhood_derive(&t[3], &out, L, Dm, 0, &f) == MI_UNET_EARG);              // no voxels
        CHECK(mi_unet_volume_nbhood_derive(&t[0], &out, 1, Dm, 0, &f) == MI_UNET_EARG);
        CHECK(mi_unet_volume_nbhood_derive(&t[0], &out, L, 0, 0, &f) == MI_UNET_EARG);
        CHECK(mi_unet_volume_nbhood_derive(&t[0], &lone, L, Dm, 0, &f) == MI_UNET_EARG);
        CHECK(miunet::g_err.rfind("mi_unet_volume_nbhood_derive:", 0) == 0 && std::memcmp(&f, &fp, sizeof f) == 0);
        CHECK(mi_unet_volume_nbhood_derive(&t[0], &out, L, Dm, 0, &f) == MI_UNET_OK && f.coarseness == 1e6 && f.contrast == 0.0 && f.gldzm.percentage == 1.0 / 105.0);
    }
    std::printf("volume_nbhood_host_test ok\n");
    return 0;
}
