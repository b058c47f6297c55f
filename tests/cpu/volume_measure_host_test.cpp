// The host half of the volume measurement (csrc/volume_measure.cpp with MIUNET_NO_DEVICE: mi_unet_volume_measure_host and
// mi_unet_volume_measure_derive) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_measure_host_test.cpp <csrc>/volume_measure.cpp
// Cases: 5 x 7 x 9 (odd sizes) with a box, a bar that reaches both ends of a row, the last voxel of the volume and ids that belong to no
// component; exact-size buffers (an overrun is the sanitizer's to find); with and without intensity; the cap; m = 4096; the derived
// shape; refused calls.  The numbers are checked against facts that hold by construction; tests/test_volume_measure_cpu.py compares the
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
    const int D = 5, H = 7, W = 9;
    const size_t n = (size_t)D * H * W;
    std::vector<int32_t> ids(n, 0);
    std::vector<uint16_t> inten(n);
    for (size_t i = 0; i < n; ++i) inten[i] = (uint16_t)(i * 211 % 65536);
    auto at = [&](int z, int y, int x) -> int32_t & { return ids[((size_t)z * H + y) * W + x]; };
    auto index = [&](int z, int y, int x) { return (int32_t)(((size_t)z * H + y) * W + x); };
    for (int z = 1; z <= 2; ++z)
        for (int y = 1; y <= 3; ++y)
            for (int x = 1; x <= 4; ++x) at(z, y, x) = 1;               // a 2 x 3 x 4 box: 24 voxels, 6 rows of 2 run ends
    for (int x = 0; x < W; ++x) at(4, 0, x) = 2;                        // a whole row: its run ends are the volume's border
    at(4, 6, 8) = 3;                                                    // the last voxel of the volume
    at(0, 0, 0) = -1; at(0, 0, 1) = 5; at(0, 0, 2) = 4097;              // no component
    inten[index(4, 6, 8)] = 65535;
    const int units[3] = { 2, 3, 5 };
    mi_unet_vmeasure t[4];
    CHECK(mi_unet_volume_measure_host(ids.data(), inten.data(), D, H, W, 4, units, nullptr, t) == MI_UNET_OK);
    CHECK(t[0].voxels == 24 && t[0].ends == 12 && t[1].voxels == 9 && t[1].ends == 2 && t[2].voxels == 1 && t[2].ends == 1);
    CHECK(t[0].sx == 6 * (1 + 2 + 3 + 4) && t[0].sy == 8 * (1 + 2 + 3) && t[0].sz == 12 * (1 + 2));
    CHECK(t[0].sxx == 6 * (1 + 4 + 9 + 16) && t[0].syy == 8 * (1 + 4 + 9) && t[0].szz == 12 * (1 + 4));
    CHECK(t[0].sxy == 2 * (1 + 2 + 3 + 4) * (1 + 2 + 3) && t[0].sxz == 3 * (1 + 2 + 3 + 4) * (1 + 2) && t[0].syz == 4 * (1 + 2 + 3) * (1 + 2));
    CHECK(t[0].d2 == 6 * 6 + 6 * 6 + 5 * 5 && t[0].dp == index(1, 1, 1) && t[0].dq == index(2, 3, 4));     // four diagonals tie: the first
    CHECK(t[0].a_d2 == 6 * 6 + 6 * 6 && t[0].a_p == index(1, 1, 1) && t[0].a_q == index(1, 3, 4));
    CHECK(t[1].d2 == 16 * 16 && t[1].dp == index(4, 0, 0) && t[1].dq == index(4, 0, 8) && t[1].a_d2 == t[1].d2 && t[1].a_q == t[1].dq);
    CHECK(t[2].d2 == 0 && t[2].dp == index(4, 6, 8) && t[2].dq == t[2].dp && t[2].a_d2 == 0 && t[2].a_p == t[2].dp && t[2].a_q == t[2].dp);
    CHECK(t[2].imin == 65535 && t[2].imax == 65535 && t[2].si == 65535 && t[2].sii == 65535LL * 65535LL);
    int64_t si = 0;
    for (int x = 0; x < W; ++x) si += inten[index(4, 0, x)];
    CHECK(t[1].si == si && t[1].imin <= t[1].imax);
    mi_unet_vmeasure zero;
    std::memset(&zero, 0, sizeof zero);
    CHECK(std::memcmp(&t[3], &zero, sizeof zero) == 0);                 // an id that no voxel carries

    // no intensity; a cap of 2 skips the box only; a cap of 0 skips all; m = 4096
    mi_unet_vmeasure u[3];
    mi_unet_vmeasure_opts o = { 2 };
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 3, units, &o, u) == MI_UNET_OK);
    CHECK(u[0].d2 == -1 && u[0].dp == -1 && u[0].dq == -1 && u[0].a_d2 == -1 && u[0].a_p == -1 && u[0].a_q == -1 && u[0].ends == 12 && u[0].sx == t[0].sx);
    CHECK(u[1].d2 == t[1].d2 && u[2].d2 == 0 && u[1].imin == 0 && u[1].imax == 0 && u[1].si == 0 && u[1].sii == 0);
    o.max_ends = 0;
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 3, units, &o, u) == MI_UNET_OK);
    CHECK(u[0].d2 == -1 && u[1].d2 == -1 && u[2].a_q == -1 && u[2].voxels == 1);
    std::vector<mi_unet_vmeasure> big(4096);
    CHECK(mi_unet_volume_measure_host(ids.data(), inten.data(), D, H, W, 4096, units, nullptr, big.data()) == MI_UNET_OK);
    CHECK(std::memcmp(big.data(), t, 3 * sizeof zero) == 0 && big[4].voxels == 1 && big[4095].voxels == 0);             // id 5 is a component now

    // one voxel that is the whole volume
    const int32_t one = 1;
    CHECK(mi_unet_volume_measure_host(&one, nullptr, 1, 1, 1, 1, units, nullptr, u) == MI_UNET_OK);
    CHECK(u[0].voxels == 1 && u[0].ends == 1 && u[0].d2 == 0 && u[0].dp == 0 && u[0].dq == 0);

    // the derived shape of the box: centroid, axes along z, y, x by extent in mm (2 x 2.5, 3 x 1.5, 4 x 1: variances 2.08, 1.69, 1.33), diameters
    mi_unet_vmeasure_shape s;
    CHECK(mi_unet_volume_measure_derive(&t[0], units, 0.5, &s) == MI_UNET_OK);
    CHECK(std::fabs(s.cx_mm - 3.0 * 1.0) < 1e-12 && std::fabs(s.cy_mm - 2.5 * 1.5) < 1e-12 && std::fabs(s.cz_mm - 2.0 * 2.5) < 1e-12);
    const double var[3] = { 4.0 * 2.5 * 2.5 / 12.0, 9.0 * 1.5 * 1.5 / 12.0, 16.0 * 1.0 * 1.0 / 12.0 };             // z, y, x: (extent in mm)^2 / 12
    for (int i = 0; i < 3; ++i) CHECK(std::fabs(s.axis_mm[i] - 2.0 * std::sqrt(5.0 * var[i])) < 1e-12);
    CHECK(std::fabs(s.axis_dir[0][2] - 1.0) < 1e-12 && std::fabs(s.axis_dir[1][1] - 1.0) < 1e-12 && std::fabs(s.axis_dir[2][0] - 1.0) < 1e-12);
    CHECK(std::fabs(s.diameter_mm - std::sqrt(97.0) * 0.5) < 1e-12 && std::fabs(s.axial_diameter_mm - std::sqrt(72.0) * 0.5) < 1e-12);
    CHECK(mi_unet_volume_measure_derive(&u[0], units, 0.5, &s) == MI_UNET_OK && s.std == 0.0 && s.diameter_mm == 0.0);
    o.max_ends = 0;
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 1, units, &o, u) == MI_UNET_OK);
    CHECK(mi_unet_volume_measure_derive(&u[0], units, 0.5, &s) == MI_UNET_OK && std::isnan(s.diameter_mm) && std::isnan(s.axial_diameter_mm));

    // refused calls
    const int bad_units[3] = { 1, 0, 1 }, far[3] = { 1, 1, 46341 };
    o.max_ends = -1;
    CHECK(mi_unet_volume_measure_host(nullptr, nullptr, D, H, W, 3, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, 0, H, W, 3, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, 8193, 3, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 0, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 4097, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 3, bad_units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 3, far, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_measure_host(ids.data(), nullptr, D, H, W, 3, units, &o, u) == MI_UNET_EARG && miunet::g_err.find("max_ends") != std::string::npos);
    CHECK(mi_unet_volume_measure_derive(&zero, units, 0.5, &s) == MI_UNET_EARG && mi_unet_volume_measure_derive(&t[0], units, 0.0, &s) == MI_UNET_EARG);
    std::printf("volume_measure_host_test ok\n");
    return 0;
}
