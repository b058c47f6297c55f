// The host half of the volume texture (csrc/volume_texture.cpp with MIUNET_NO_DEVICE: mi_unet_volume_texture_host and
// mi_unet_volume_texture_derive) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_texture_host_test.cpp <csrc>/volume_texture.cpp
// Cases: Haralick's 4 x 4 image as a 4 x 1 x 4 volume; 5 x 7 x 9 (odd sizes) with a box, a row that reaches both ends, the last voxel of
// the volume and ids that belong to no component; exact-size buffers (an overrun is the sanitizer's to find); both modes; either table
// NULL; the caps; the derived features; refused calls.  The numbers are checked against facts that hold by construction;
// tests/test_volume_texture_cpu.py compares the same entry points with the reference.
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
    {   // Haralick 1973, fig. 3: with H = 1 only (1, 0, 0) has dz = 0, so G + G^T of the axial table is his horizontal matrix
        const uint16_t img[16] = { 0, 0, 1, 1, 0, 0, 1, 1, 0, 2, 2, 2, 2, 2, 3, 3 };
        const int32_t ids[16] = { 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 };
        const int want[4][4] = { { 4, 2, 1, 0 }, { 2, 4, 0, 0 }, { 1, 0, 6, 1 }, { 0, 0, 1, 2 } };
        for (int mode = 0; mode < 2; ++mode) {
            const mi_unet_vtexture_opts o = { mode, 4, 0, 1 };
            mi_unet_vtexture t;
            uint32_t hist[4], g[16], ga[16];
            CHECK(mi_unet_volume_texture_host(ids, img, 4, 1, 4, 1, &o, &t, hist, g, ga) == MI_UNET_OK);
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j) CHECK((int)(ga[i * 4 + j] + ga[j * 4 + i]) == want[i][j]);
            CHECK(t.voxels == 16 && t.imin == 0 && t.imax == 3 && t.levels_used == 4 && t.pairs_axial == 12 && t.pairs == 12 + 12 + 9 + 9);
            CHECK(hist[0] == 5 && hist[1] == 4 && hist[2] == 5 && hist[3] == 2);
            mi_unet_vtexture_features f;
            CHECK(mi_unet_volume_texture_derive(&t, hist, ga, 4, &f) == MI_UNET_OK);
            CHECK(std::fabs(f.angular_second_moment - 84.0 / 576.0) < 1e-15);          // sum P^2 / 24^2
            CHECK(std::fabs(f.contrast - (2 * 2 * 1 + 2 * 1 * 4 + 2 * 1 * 1) / 24.0) < 1e-15 && f.joint_max == 6.0 / 24.0);
            CHECK(f.mode == 1 && f.median == 2 && f.p10 == 1 && f.p90 == 4);
        }
    }
    const int D = 5, H = 7, W = 9, L = 16;
    const size_t n = (size_t)D * H * W;
    std::vector<int32_t> ids(n, 0);
    std::vector<uint16_t> inten(n);
    for (size_t i = 0; i < n; ++i) inten[i] = (uint16_t)(i * 211 % 65536);
    auto at = [&](int z, int y, int x) -> int32_t & { return ids[((size_t)z * H + y) * W + x]; };
    auto index = [&](int z, int y, int x) { return ((size_t)z * H + y) * W + x; };
    for (int z = 1; z <= 2; ++z)
        for (int y = 1; y <= 3; ++y)
            for (int x = 1; x <= 4; ++x) at(z, y, x) = 1;               // a 2 x 3 x 4 box
    for (int x = 0; x < W; ++x) at(4, 0, x) = 2;                        // a whole row: its neighbours would lie outside the volume
    at(4, 6, 8) = 3;                                                    // the last voxel of the volume
    at(0, 0, 0) = -1; at(0, 0, 1) = 5; at(0, 0, 2) = 4097;              // no component
    inten[index(4, 6, 8)] = 65535;
    // the pairs of a d x h x w box: sum over the offsets of the products of (extent - |offset|)
    auto box_pairs = [](int d, int h, int w, bool axial) {
        int64_t s = 0;
        for (int dz = 0; dz <= (axial ? 0 : 1); ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx)
                    if (dz > 0 || dy > 0 || (dy == 0 && dx > 0)) s += (int64_t)(d - dz) * (h - std::abs(dy)) * (w - std::abs(dx));
        return s;
    };
    std::vector<mi_unet_vtexture> t(4);
    std::vector<uint32_t> hist(4 * L), g(4 * L * L), ga(4 * L * L);
    const mi_unet_vtexture_opts o = { MI_UNET_VTEX_COUNT, L, 0, 1 };
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_OK);
    CHECK(t[0].voxels == 24 && t[1].voxels == 9 && t[2].voxels == 1 && t[3].voxels == 0);
    CHECK(t[0].pairs == box_pairs(2, 3, 4, false) && t[0].pairs_axial == box_pairs(2, 3, 4, true));
    CHECK(t[1].pairs == 8 && t[1].pairs_axial == 8 && t[2].pairs == 0 && t[2].imin == 65535 && t[2].imax == 65535 && t[2].levels_used == 1);
    CHECK(hist[2 * L] == 1);                                            // a constant component is all level 0
    CHECK(t[1].imin == (int)inten[index(4, 0, 0)] && t[1].imax == (int)inten[index(4, 0, 8)]);
    for (int r = 0; r < 4; ++r) {
        int64_t hs = 0, gs = 0, as = 0;
        for (int l = 0; l < L; ++l) hs += hist[r * L + l];
        for (int c = 0; c < L * L; ++c) { gs += g[r * L * L + c]; as += ga[r * L * L + c]; }
        CHECK(hs == t[r].voxels && gs == t[r].pairs && as == t[r].pairs_axial);
    }
    mi_unet_vtexture zero;
    std::memset(&zero, 0, sizeof zero);
    CHECK(std::memcmp(&t[3], &zero, sizeof zero) == 0);                 // an id that no voxel carries
    // the lowest and the highest value of a component fall into the first and the last level
    CHECK(g[1 * L * L + 0 * L + 0] + g[1 * L * L + 0 * L + 1] >= 1 && hist[1 * L + 0] >= 1 && hist[1 * L + L - 1] >= 1);

    // either table NULL: the other one and the histogram are the same bytes, the sum of the missing one is 0
    std::vector<mi_unet_vtexture> u(4);
    std::vector<uint32_t> hist2(4 * L), g2(4 * L * L);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &o, u.data(), hist2.data(), g2.data(), nullptr) == MI_UNET_OK);
    CHECK(g2 == g && hist2 == hist && u[0].pairs == t[0].pairs && u[0].pairs_axial == 0);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &o, u.data(), hist2.data(), nullptr, g2.data()) == MI_UNET_OK);
    CHECK(g2 == ga && hist2 == hist && u[0].pairs == 0 && u[0].pairs_axial == t[0].pairs_axial);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &o, u.data(), hist2.data(), nullptr, nullptr) == MI_UNET_OK);
    CHECK(hist2 == hist && u[0].pairs == 0 && u[0].pairs_axial == 0 && u[0].levels_used == t[0].levels_used);

    // fixed bin size: below lo is level 0, beyond the top bin is level L - 1
    const mi_unet_vtexture_opts wo = { MI_UNET_VTEX_WIDTH, L, 20000, 1000 };
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &wo, u.data(), hist2.data(), g2.data(), nullptr) == MI_UNET_OK);
    CHECK(hist2[2 * L + L - 1] == 1 && u[2].imin == 65535);
    uint32_t below = 0, beyond = 0;
    for (int z = 1; z <= 2; ++z)
        for (int y = 1; y <= 3; ++y)
            for (int x = 1; x <= 4; ++x) {
                below += inten[index(z, y, x)] < 21000;
                beyond += inten[index(z, y, x)] >= 20000 + 15 * 1000;
            }
    CHECK(hist2[0] == below && hist2[L - 1] == beyond && u[0].pairs == t[0].pairs);

    // the caps: m = 4096 at 32 levels and m = 1024 at 64, both 2^22 cells; the default options
    std::vector<mi_unet_vtexture> big(4096);
    std::vector<uint32_t> bh(4096 * 32), bg((size_t)1 << 22);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4096, nullptr, big.data(), bh.data(), bg.data(), nullptr) == MI_UNET_OK);
    CHECK(big[0].pairs == t[0].pairs && big[4].voxels == 1 && big[4095].voxels == 0);                                    // id 5 is a component now
    const mi_unet_vtexture_opts o64 = { MI_UNET_VTEX_COUNT, 64, 0, 1 };
    bh.assign(1024 * 64, 0);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 1024, &o64, big.data(), bh.data(), nullptr, bg.data()) == MI_UNET_OK);
    CHECK(big[0].pairs_axial == t[0].pairs_axial && big[1023].voxels == 0);

    // one voxel that is the whole volume
    const int32_t one = 1;
    const uint16_t v1 = 7;
    uint32_t h1[32], g1[32 * 32];
    CHECK(mi_unet_volume_texture_host(&one, &v1, 1, 1, 1, 1, nullptr, u.data(), h1, g1, nullptr) == MI_UNET_OK);
    CHECK(u[0].voxels == 1 && u[0].imin == 7 && u[0].imax == 7 && u[0].pairs == 0 && h1[0] == 1 && h1[1] == 0);
    mi_unet_vtexture_features f;
    CHECK(mi_unet_volume_texture_derive(&u[0], h1, g1, 32, &f) == MI_UNET_OK);
    CHECK(f.mean == 1.0 && f.variance == 0.0 && f.skewness == 0.0 && f.kurtosis == 0.0 && f.entropy == 0.0 && f.uniformity == 1.0 && f.mode == 1);
    CHECK(std::isnan(f.joint_max) && std::isnan(f.correlation) && std::isnan(f.contrast));
    CHECK(mi_unet_volume_texture_derive(&t[0], hist.data(), g.data(), L, &f) == MI_UNET_OK);
    CHECK(f.joint_max > 0.0 && f.joint_max <= 1.0 && f.joint_entropy >= 0.0 && f.correlation >= -1.0 && f.correlation <= 1.0);
    CHECK(mi_unet_volume_texture_derive(&t[0], hist.data(), nullptr, L, &f) == MI_UNET_OK && std::isnan(f.joint_max) && f.variance > 0.0);

    // refused calls
    mi_unet_vtexture_opts bad = o;
    CHECK(mi_unet_volume_texture_host(nullptr, inten.data(), D, H, W, 4, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), nullptr, D, H, W, 4, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &o, nullptr, hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &o, t.data(), nullptr, g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), 0, H, W, 4, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, 8193, 4, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), 4097, 256, 256, 4, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 0, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4097, &o, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 1025, &o64, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    bad.levels = 1;
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &bad, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    bad.levels = 65;
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &bad, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    bad = o; bad.mode = 2;
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &bad, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    bad = o; bad.width = 0;
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &bad, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG);
    bad = o; bad.lo = 65536;
    CHECK(mi_unet_volume_texture_host(ids.data(), inten.data(), D, H, W, 4, &bad, t.data(), hist.data(), g.data(), ga.data()) == MI_UNET_EARG &&
          miunet::g_err.find("mi_unet_volume_texture_host: lo") == 0);
    CHECK(mi_unet_volume_texture_derive(&zero, hist.data(), nullptr, L, &f) == MI_UNET_EARG && mi_unet_volume_texture_derive(&t[0], hist.data(), nullptr, 65, &f) == MI_UNET_EARG);
    std::printf("volume_texture_host_test ok\n");
    return 0;
}
