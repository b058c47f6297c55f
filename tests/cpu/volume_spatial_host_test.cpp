// The host half of the volume spatial statistics (csrc/volume_spatial.cpp with MIUNET_NO_DEVICE: mi_unet_volume_spatial_host and
// mi_unet_volume_spatial_derive) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_spatial_host_test.cpp <csrc>/volume_spatial.cpp
// Cases: 5 x 7 x 9 (odd sizes) with a box, a whole row, the last voxel of the volume and ids that belong to no component; exact-size
// buffers (an overrun is the sanitizer's to find); a ball that reaches past every face; the cap; m = 4096; the derived numbers; refused
// calls.  The numbers are checked against facts that hold by construction; tests/test_volume_spatial_cpu.py compares the same entry
// points with the reference.
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
    for (size_t i = 0; i < n; ++i) inten[i] = (uint16_t)(i * 211 % 60000);
    auto at = [&](int z, int y, int x) -> int32_t & { return ids[((size_t)z * H + y) * W + x]; };
    auto index = [&](int z, int y, int x) { return (int32_t)(((size_t)z * H + y) * W + x); };
    for (int z = 1; z <= 2; ++z)
        for (int y = 1; y <= 3; ++y)
            for (int x = 1; x <= 4; ++x) at(z, y, x) = 1;               // a 2 x 3 x 4 box: 24 voxels, 276 pairs
    for (int x = 0; x < W; ++x) at(4, 0, x) = 2;                        // a whole row
    at(4, 6, 8) = 3;                                                    // the last voxel of the volume
    at(0, 0, 0) = -1; at(0, 0, 1) = 5; at(0, 0, 2) = 4097;              // no component
    inten[index(4, 6, 8)] = 65535;
    const int units[3] = { 2, 3, 5 };
    mi_unet_vspatial t[4];
    mi_unet_vspatial_opts o = { 1000, 6 };                              // B(6): ex = 3, ey = 2, ez = 1
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 4, units, &o, t) == MI_UNET_OK);
    CHECK(t[0].voxels == 24 && t[0].searched == 1 && t[0].pairs == 276 && t[1].voxels == 9 && t[1].pairs == 36 && t[2].voxels == 1);
    CHECK(t[2].searched == 0 && t[2].pairs == 0 && t[2].s0 == 0.0 && t[2].s1 == 0.0 && t[2].s2 == 0.0 && t[2].s3 == 0.0);
    CHECK(t[0].sx == 6 * (1 + 2 + 3 + 4) && t[0].sy == 8 * (1 + 2 + 3) && t[0].sz == 12 * (1 + 2));
    int64_t si = 0, six = 0, imax = 0;
    for (int x = 0; x < W; ++x) { si += inten[index(4, 0, x)]; six += (int64_t)x * inten[index(4, 0, x)]; imax = std::max<int64_t>(imax, inten[index(4, 0, x)]); }
    CHECK(t[1].si == si && t[1].six == six && t[1].siy == 0 && t[1].siz == 4 * si && t[1].imax == imax && t[1].imin <= t[1].imax);
    CHECK(t[1].centre == (2 * si + 9) / 18 && t[1].reserved == 0);
    // the row's pairs lie 2 (x_j - x_i) apart: s0 = sum over the gaps g = 1 .. 8 of (9 - g) / (2 g)
    double s0 = 0.0;
    for (int g = 1; g <= 8; ++g) s0 += (9 - g) / (2.0 * g);
    CHECK(std::fabs(t[1].s0 - s0) < 1e-13 && t[1].s3 > 0.0);
    // the last voxel: its sphere is cut on three faces; the single voxel carries both peaks
    CHECK(t[2].gp_at == index(4, 6, 8) && t[2].lp_at == t[2].gp_at && t[2].gp_n == t[2].lp_n && t[2].gp_sum == t[2].lp_sum);
    // (rows of B(6) that stay inside: dz = 0 with dy = 0, -1, -2: hx = 3, 2, 0; dz = -1 with dy = 0, -1: hx = 1, 0; each cut to x <= 8)
    CHECK(t[2].gp_n == 4 + 3 + 1 + 2 + 1 && t[2].imin == 65535 && t[2].si == 65535);
    mi_unet_vspatial zero;
    std::memset(&zero, 0, sizeof zero);
    CHECK(std::memcmp(&t[3], &zero, sizeof zero) == 0);                 // an id that no voxel carries

    // peak_r = 0: both peaks are the first voxel that carries imax
    mi_unet_vspatial u[3];
    o.peak_r = 0;
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, units, &o, u) == MI_UNET_OK);
    for (int r = 0; r < 3; ++r) CHECK(u[r].gp_n == 1 && u[r].gp_sum == u[r].imax && u[r].gp_at == u[r].lp_at && inten[u[r].gp_at] == u[r].imax);
    CHECK(u[0].s0 == t[0].s0 && u[0].s2 == t[0].s2);                    // the pair sums do not depend on the ball

    // a cap of 9 skips the box only; a cap of 0 skips all; the rest of the entry stays; m = 4096
    o.max_voxels = 9;
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, units, &o, u) == MI_UNET_OK);
    CHECK(u[0].searched == 0 && u[0].pairs == 0 && u[0].s0 == 0.0 && u[0].s3 == 0.0 && u[0].sx == t[0].sx && u[0].centre == t[0].centre);
    CHECK(u[1].searched == 1 && u[1].s0 == t[1].s0 && u[1].s1 == t[1].s1);
    o.max_voxels = 0;
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, units, &o, u) == MI_UNET_OK);
    CHECK(u[0].searched == 0 && u[1].searched == 0 && u[1].s0 == 0.0 && u[1].si == t[1].si && u[1].gp_n == 1);
    std::vector<mi_unet_vspatial> big(4096);
    o.max_voxels = 1000; o.peak_r = 6;
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 4096, units, &o, big.data()) == MI_UNET_OK);
    CHECK(std::memcmp(big.data(), t, 3 * sizeof zero) == 0 && big[4].voxels == 1 && big[4095].voxels == 0);             // id 5 is a component now

    // one voxel that is the whole volume, under the default options
    const int32_t one = 1;
    const uint16_t v7 = 7;
    CHECK(mi_unet_volume_spatial_host(&one, &v7, 1, 1, 1, 1, units, nullptr, u) == MI_UNET_OK);
    CHECK(u[0].voxels == 1 && u[0].centre == 7 && u[0].gp_at == 0 && u[0].gp_sum == 7 && u[0].gp_n == 1 && u[0].searched == 0);

    // the derived numbers of the row: the centroids, the shift along x only, the integrated intensity, NaN without pair sums
    mi_unet_vspatial_metrics s;
    CHECK(mi_unet_volume_spatial_derive(&t[1], units, 0.5, &s) == MI_UNET_OK);
    CHECK(std::fabs(s.cx_mm - 4.5 * 1.0) < 1e-12 && std::fabs(s.cy_mm - 0.5 * 1.5) < 1e-12 && std::fabs(s.cz_mm - 4.5 * 2.5) < 1e-12);
    CHECK(std::fabs(s.icx_mm - ((double)six / (double)si + 0.5)) < 1e-12 && s.icy_mm == s.cy_mm && std::fabs(s.icz_mm - s.cz_mm) < 1e-12);
    CHECK(std::fabs(s.com_shift_mm - std::fabs(s.icx_mm - s.cx_mm)) < 1e-12 && std::fabs(s.integrated_intensity - (double)si * 1.0 * 1.5 * 2.5) < 1e-6);
    CHECK(std::isfinite(s.morans_i) && s.gearys_c > 0.0 && s.global_peak >= s.local_peak && s.local_peak > 0.0);
    CHECK(mi_unet_volume_spatial_derive(&t[2], units, 0.5, &s) == MI_UNET_OK && std::isnan(s.morans_i) && std::isnan(s.gearys_c) && s.com_shift_mm == 0.0);

    // refused calls
    const int bad_units[3] = { 1, 0, 1 }, far[3] = { 1, 1, 46341 }, fine[3] = { 1, 1, 1 };
    const mi_unet_vspatial_opts neg = { -1, 0 }, over = { (1 << 20) + 1, 0 }, r_neg = { 10, -1 }, r_over = { 10, 46341 }, rows = { 10, 32 },
                                wide = { 10, 200 }, ok_rows = { 10, 31 };
    CHECK(mi_unet_volume_spatial_host(nullptr, inten.data(), D, H, W, 3, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), nullptr, D, H, W, 3, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), 0, H, W, 3, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, 8193, 3, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 0, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 4097, units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, bad_units, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, far, nullptr, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, units, &neg, u) == MI_UNET_EARG && miunet::g_err.find("max_voxels") != std::string::npos);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, units, &over, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, units, &r_neg, u) == MI_UNET_EARG && miunet::g_err.find("peak_r") != std::string::npos);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, units, &r_over, u) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, fine, &rows, u) == MI_UNET_EARG && miunet::g_err.find("rows") != std::string::npos);   // 65 x 65
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, fine, &ok_rows, u) == MI_UNET_OK);                                                   // 63 x 63
    const int flat[3] = { 1, 100, 100 };                                // B(200) under (1, 100, 100): 5 x 5 rows of up to 401 voxels: legal
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, flat, &wide, u) == MI_UNET_OK);
    const int slab[3] = { 1, 2000, 2000 };                              // B(46340) under (1, 2000, 2000): 47 x 47 rows, but 1e8 voxels
    const mi_unet_vspatial_opts huge = { 10, 46340 };
    CHECK(mi_unet_volume_spatial_host(ids.data(), inten.data(), D, H, W, 3, slab, &huge, u) == MI_UNET_EARG && miunet::g_err.find("voxels (at most") != std::string::npos);
    CHECK(mi_unet_volume_spatial_derive(&zero, units, 0.5, &s) == MI_UNET_EARG && mi_unet_volume_spatial_derive(&t[0], units, 0.0, &s) == MI_UNET_EARG);
    CHECK(mi_unet_volume_spatial_derive(&t[0], bad_units, 0.5, &s) == MI_UNET_EARG && mi_unet_volume_spatial_derive(nullptr, units, 0.5, &s) == MI_UNET_EARG);
    std::printf("volume_spatial_host_test ok\n");
    return 0;
}
