// The host half of the volume clean-up (csrc/volume_clean.cpp with MIUNET_NO_DEVICE: mi_unet_volume_clean_host and
// mi_unet_volume_ball) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_clean_host_test.cpp <csrc>/volume_clean.cpp
// Cases: 7 x 9 x 11 (odd sizes) with a closed shell and a speck under two values, the fill, a close and an open by an anisotropic ball
// whose half-widths pass the sides, out aliasing masks, one slice, one voxel, the largest radius, the ball itself, a refused call.
// The numbers are checked against facts that hold by construction; tests/test_volume_clean_cpu.py compares the same entry points
// with the reference.
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
    const int D = 7, H = 9, W = 11;
    const size_t n = (size_t)D * H * W;
    std::vector<uint8_t> vol(n, 0);
    auto at = [&](int z, int y, int x) -> uint8_t & { return vol[((size_t)z * H + y) * W + x]; };
    for (int z = 1; z <= 5; ++z)
        for (int y = 1; y <= 7; ++y)
            for (int x = 1; x <= 9; ++x)
                at(z, y, x) = (z == 1 || z == 5 || y == 1 || y == 7 || x == 1 || x == 9) ? 1 : 0;   // a shell around 3 x 5 x 7 = 105 voxels
    at(3, 4, 5) = 2;                                                    // a speck of the other value inside the cavity
    at(6, 8, 10) = 2;                                                   // and the last voxel of the volume
    const int shell = 5 * 7 * 9 - 105;
    const int values[2] = { 1, 2 }, iso[3] = { 1, 1, 1 };
    {   // the default options: fill only
        std::vector<uint8_t> out(2 * n, 9);
        mi_unet_volume_clean_stat st[2];
        CHECK(mi_unet_volume_clean_host(vol.data(), D, H, W, values, 2, iso, nullptr, out.data(), st) == MI_UNET_OK);
        CHECK(st[0].value == 1 && st[0].reserved == 0 && st[0].in_voxels == shell && st[0].filled == 105 && st[0].closed == 0 && st[0].opened == 0);
        CHECK(st[0].out_voxels == 5 * 7 * 9 && out[(3 * H + 4) * W + 5] == 1 && out[0] == 0);          // the speck is not in S: filled
        CHECK(st[1].value == 2 && st[1].in_voxels == 2 && st[1].filled == 0 && st[1].out_voxels == 2 && out[2 * n - 1] == 2);
    }
    {   // no fill, an open by the plus: the one-voxel walls and the specks go
        const mi_unet_volume_clean_opts o{ 0, 0, 1 };
        std::vector<uint8_t> out(2 * n, 9);
        mi_unet_volume_clean_stat st[2];
        CHECK(mi_unet_volume_clean_host(vol.data(), D, H, W, values, 2, iso, &o, out.data(), st) == MI_UNET_OK);
        CHECK(st[0].filled == 0 && st[0].opened == shell && st[0].out_voxels == 0 && st[1].opened == 2 && st[1].out_voxels == 0);
        for (uint8_t b : out) CHECK(b == 0);
    }
    {   // fill, then a close and an open by a ball whose half-widths pass every side: the close fills the volume (an erosion is
        // constrained only inside it), the open keeps it; out aliases masks
        std::vector<uint8_t> io(vol);
        const int one[1] = { 1 }, units[3] = { 2, 3, 5 };
        const mi_unet_volume_clean_opts o{ 1, 200, 200 };
        mi_unet_volume_clean_stat st;
        CHECK(mi_unet_volume_clean_host(io.data(), D, H, W, one, 1, units, &o, io.data(), &st) == MI_UNET_OK);
        CHECK(st.filled == 105 && st.closed == (int64_t)n - 5 * 7 * 9 && st.opened == 0 && st.out_voxels == (int64_t)n);
        for (uint8_t b : io) CHECK(b == 1);
    }
    {   // one slice: no cavity; a flat disc (r between the in-plane units and uz) closes the ring's hole instead
        const int h = 13, w = 15;                                       // (the ring lies further than the disc from every side)
        std::vector<uint8_t> sl((size_t)h * w, 0), out((size_t)h * w);
        for (int y = 4; y <= 8; ++y)
            for (int x = 5; x <= 9; ++x) sl[(size_t)y * w + x] = (y == 4 || y == 8 || x == 5 || x == 9) ? 3 : 0;       // a ring around 3 x 3
        const int three[1] = { 3 }, units[3] = { 2, 2, 5 };
        mi_unet_volume_clean_stat st;
        CHECK(mi_unet_volume_clean_host(sl.data(), 1, h, w, three, 1, units, nullptr, out.data(), &st) == MI_UNET_OK);
        CHECK(st.in_voxels == 16 && st.filled == 0 && st.out_voxels == 16 && std::memcmp(sl.data(), out.data(), sl.size()) == 0);
        const mi_unet_volume_clean_opts o{ 1, 4, 0 };
        CHECK(mi_unet_volume_clean_host(sl.data(), 1, h, w, three, 1, units, &o, out.data(), &st) == MI_UNET_OK);
        CHECK(st.closed == 9 && st.out_voxels == 25 && out[(size_t)6 * w + 7] == 3);
    }
    {   // one voxel, the largest radius and unit
        const uint8_t v = 7;
        uint8_t out = 0;
        const int seven[1] = { 7 }, units[3] = { 46340, 46340, 46340 };
        const mi_unet_volume_clean_opts o{ 1, 46340, 46340 };
        mi_unet_volume_clean_stat st;
        CHECK(mi_unet_volume_clean_host(&v, 1, 1, 1, seven, 1, units, &o, &out, &st) == MI_UNET_OK && out == 7 && st.out_voxels == 1);
    }
    {   // the ball
        const int units[3] = { 2, 2, 5 };
        int ext[3] = { -1, -1, -1 };
        CHECK(mi_unet_volume_ball(units, 5, ext, nullptr) == MI_UNET_OK && ext[0] == 2 && ext[1] == 2 && ext[2] == 1);
        std::vector<uint8_t> elem((size_t)3 * 5 * 5, 9);
        CHECK(mi_unet_volume_ball(units, 5, ext, elem.data()) == MI_UNET_OK);
        int set = 0;
        for (uint8_t b : elem) set += b;
        CHECK(set == 21 + 2 && elem[2 * 5 + 2] == 1 && elem[25 + 12] == 1 && elem[25] == 0);        // dx^2 + dy^2 <= 6.25 in the slice, and the two poles
        CHECK(mi_unet_volume_ball(units, 46341, ext, elem.data()) == MI_UNET_EARG && ext[0] == 2);
    }
    std::vector<uint8_t> keep(2 * n, 0x55);
    mi_unet_volume_clean_stat st;
    std::memset(&st, 0x55, sizeof st);
    const int twice[2] = { 1, 1 };
    miunet::g_err.clear();
    CHECK(mi_unet_volume_clean_host(vol.data(), D, H, W, twice, 2, iso, nullptr, keep.data(), &st) == MI_UNET_EARG);
    CHECK(keep[0] == 0x55 && keep[2 * n - 1] == 0x55 && reinterpret_cast<const uint8_t *>(&st)[0] == 0x55 && !miunet::g_err.empty());
    std::printf("volume_clean_host_test ok\n");
    return 0;
}
