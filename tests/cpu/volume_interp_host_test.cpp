// The host half of the volume interpolation (csrc/volume_interp.cpp with MIUNET_NO_DEVICE: mi_unet_volume_interp_host and
// mi_unet_volume_interp_slices) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_interp_host_test.cpp <csrc>/volume_interp.cpp
// Cases: an all-set slice between two empty ones at k = 4, a square that grows between two slices of 9 x 11 (odd sizes) under two
// values with the intensity, one slice, one pixel, one column under a unit that would overflow if it were squared, k = 16 with the
// intensity's extremes, a refused call.  The numbers are checked against facts that hold by construction;
// tests/test_volume_interp_cpu.py compares the same entry points with the reference.
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

static int count(const uint8_t *p, size_t n, uint8_t v)
{
    int c = 0;
    for (size_t i = 0; i < n; ++i) c += p[i] == v;
    return c;
}

int main()
{
    const int iso[2] = { 1, 1 }, one = 1;
    CHECK(mi_unet_volume_interp_slices(1, 1) == 1 && mi_unet_volume_interp_slices(5, 4) == 17 && mi_unet_volume_interp_slices(8192, 16) == 131057);
    CHECK(mi_unet_volume_interp_slices(0, 1) == -1 && mi_unet_volume_interp_slices(8193, 1) == -1 && mi_unet_volume_interp_slices(3, 0) == -1 &&
          mi_unet_volume_interp_slices(3, 17) == -1);
    {   // all set between two empty slices: NONE against NONE, the nearer slice wins and the middle is set
        std::vector<uint8_t> vol(3 * 64, 0), out(9 * 64, 0x55);
        std::memset(vol.data() + 64, 1, 64);
        mi_unet_vinterp_stat st;
        CHECK(mi_unet_volume_interp_host(vol.data(), 3, 8, 8, &one, 1, iso, 4, nullptr, out.data(), nullptr, &st) == MI_UNET_OK);
        const int want[9] = { 0, 0, 64, 64, 64, 64, 64, 0, 0 };
        for (int z = 0; z < 9; ++z) CHECK(count(out.data() + z * 64, 64, 1) == want[z] && count(out.data() + z * 64, 64, 0) == 64 - want[z]);
        CHECK(st.in_voxels == 64 && st.out_voxels == 5 * 64 && st.mixed == 6 * 64 && st.mixed_set == 4 * 64 && st.ties == 2 * 64);
    }
    {   // a 3 x 3 square (value 1) that becomes 7 x 7, a pixel of value 2 beside it, units (7, 7) = (1, 1); k = 2: the middle slice holds
        // the pixels within Chebyshev distance 1 of the small square's border, a 5 x 5 square
        const int D = 2, H = 9, W = 11, k = 2, Dp = 3;
        std::vector<uint8_t> vol((size_t)D * H * W, 0);
        auto at = [&](int z, int y, int x) -> uint8_t & { return vol[((size_t)z * H + y) * W + x]; };
        for (int y = 3; y <= 5; ++y)
            for (int x = 4; x <= 6; ++x) at(0, y, x) = 1;
        for (int y = 1; y <= 7; ++y)
            for (int x = 2; x <= 8; ++x) at(1, y, x) = 1;
        at(0, 0, 0) = 2;
        std::vector<uint16_t> img((size_t)D * H * W), iout((size_t)Dp * H * W, 0x5555);
        for (size_t i = 0; i < img.size(); ++i) img[i] = (uint16_t)(i * 331u);
        const int values[2] = { 1, 2 }, units[2] = { 7, 7 };
        std::vector<uint8_t> out((size_t)2 * Dp * H * W, 0x55);
        mi_unet_vinterp_stat st[2];
        CHECK(mi_unet_volume_interp_host(vol.data(), D, H, W, values, 2, units, k, img.data(), out.data(), iout.data(), st) == MI_UNET_OK);
        const size_t hw = (size_t)H * W;
        CHECK(count(out.data(), hw, 1) == 9 && count(out.data() + 2 * hw, hw, 1) == 49);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) CHECK((out[hw + (size_t)y * W + x] == 1) == (y >= 2 && y <= 6 && x >= 3 && x <= 7));
        CHECK(st[0].in_voxels == 58 && st[0].out_voxels == 9 + 25 + 49 && st[0].mixed == 40 && st[0].mixed_set == 16);
        // value 2: one pixel against an empty slice: e_set = 1 against NONE, unset; the bytes of its plane are 0 or 2
        CHECK(st[1].in_voxels == 1 && st[1].out_voxels == 1 && st[1].mixed == 1 && st[1].mixed_set == 0 && st[1].ties == 0);
        CHECK(out[(size_t)Dp * hw] == 2 && count(out.data() + (size_t)Dp * hw, (size_t)Dp * hw, 0) == (int)(Dp * hw) - 1);
        for (size_t i = 0; i < hw; ++i) {
            CHECK(iout[i] == img[i] && iout[2 * hw + i] == img[hw + i]);
            CHECK(iout[hw + i] == (uint16_t)(((unsigned)img[i] + img[hw + i] + 1) / 2));
        }
    }
    {   // one slice: the identity whatever the factor; one pixel; one column under a unit whose square passes 64 bits if it were taken
        const uint8_t sl[6] = { 3, 0, 3, 3, 3, 0 };
        uint8_t out[6];
        const int three = 3, big[2] = { 2147483647, 1 };
        mi_unet_vinterp_stat st;
        CHECK(mi_unet_volume_interp_host(sl, 1, 2, 3, &three, 1, iso, 16, nullptr, out, nullptr, &st) == MI_UNET_OK);
        CHECK(std::memcmp(sl, out, 6) == 0 && st.in_voxels == 4 && st.out_voxels == 4 && st.mixed == 0);
        CHECK(mi_unet_volume_interp_host(sl, 1, 1, 1, &three, 1, iso, 1, nullptr, out, nullptr, nullptr) == MI_UNET_OK && out[0] == 3);
        uint8_t col[3 * 5];
        CHECK(mi_unet_volume_interp_host(sl, 2, 3, 1, &three, 1, big, 2, nullptr, col, nullptr, &st) == MI_UNET_OK);
        // slice 0 = (set, unset, set), slice 1 = (set, set, unset): the last two pixels are mixed, each 1 against 1, ties, set
        CHECK(col[3] == 3 && col[4] == 3 && col[5] == 3 && st.mixed == 2 && st.ties == 2 && st.mixed_set == 2 && st.out_voxels == 7);
    }
    {   // the intensity's extremes at k = 16: ((16 - j) 0 + j 65535 + 8) / 16 and back
        const uint8_t m[2] = { 0, 0 };
        const uint16_t in[2] = { 0, 65535 };
        uint8_t out[17];
        uint16_t up[17], down[17];
        const uint16_t rev[2] = { 65535, 0 };
        CHECK(mi_unet_volume_interp_host(m, 2, 1, 1, &one, 1, iso, 16, in, out, up, nullptr) == MI_UNET_OK);
        CHECK(mi_unet_volume_interp_host(m, 2, 1, 1, &one, 1, iso, 16, rev, out, down, nullptr) == MI_UNET_OK);
        for (unsigned j = 0; j <= 16; ++j) CHECK(up[j] == (j * 65535u + 8u) / 16u && down[j] == ((16u - j) * 65535u + 8u) / 16u);
        CHECK(up[0] == 0 && up[16] == 65535 && down[0] == 65535 && down[16] == 0);
    }
    // a refused call: the message names the function and nothing is written
    std::vector<uint8_t> vol(2 * 4 * 4, 1), keep(3 * 4 * 4, 0x55);
    mi_unet_vinterp_stat st;
    std::memset(&st, 0x55, sizeof st);
    CHECK(mi_unet_volume_interp_host(vol.data(), 2, 4, 4, &one, 1, iso, 17, nullptr, keep.data(), nullptr, &st) == MI_UNET_EARG);
    CHECK(miunet::g_err.find("mi_unet_volume_interp_host: factor 17") == 0 && count(keep.data(), keep.size(), 0x55) == (int)keep.size());
    CHECK(st.in_voxels == 0x5555555555555555LL);
    const int far[2] = { 46341, 1 };
    CHECK(mi_unet_volume_interp_host(vol.data(), 2, 4, 2, &one, 1, far, 2, nullptr, keep.data(), nullptr, &st) == MI_UNET_EARG);
    CHECK(mi_unet_volume_interp_host(vol.data(), 2, 4, 4, &one, 1, iso, 2, nullptr, vol.data() + 8, nullptr, &st) == MI_UNET_EARG);
    CHECK(miunet::g_err.find("out overlaps masks") != std::string::npos);
    std::printf("volume_interp_host_test ok\n");
    return 0;
}
