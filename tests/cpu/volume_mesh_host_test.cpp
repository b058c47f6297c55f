// The host half of the volume mesh (csrc/volume_mesh.cpp with MIUNET_NO_DEVICE: mi_unet_volume_mesh_host,
// mi_unet_volume_mesh_positions and mi_unet_volume_mesh_derive) as a stand-alone program, so that it can run under
// -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_mesh_host_test.cpp <csrc>/volume_mesh.cpp
// Cases: 5 x 7 x 9 (odd sizes) with a box, a voxel that touches it along an edge and the last voxel of the volume under a second value;
// both placements, exact-size arrays (an overrun is the sanitizer's to find), caps at half, the counting call, one voxel that is the whole
// volume, the metrics, refused calls.  The numbers are checked against facts that hold by construction; tests/test_volume_mesh_cpu.py
// compares the same entry points with the reference.
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
    std::vector<uint8_t> vol(n, 0);
    auto at = [&](int z, int y, int x) -> uint8_t & { return vol[((size_t)z * H + y) * W + x]; };
    for (int z = 1; z <= 2; ++z)
        for (int y = 1; y <= 3; ++y)
            for (int x = 1; x <= 4; ++x) at(z, y, x) = 1;               // a 2 x 3 x 4 box: 52 quads, 54 vertices
    at(3, 4, 2) = 1;                                                    // touches the box along one edge: 6 quads, 8 - 2 vertices more
    at(4, 6, 8) = 2;                                                    // the last voxel of the volume
    const int values[2] = { 1, 2 };
    const double mm[3] = { 0.5, 0.75, 2.0 };
    for (int placement = 0; placement < 2; ++placement) {
        mi_unet_mesh_stat st[2];
        CHECK(mi_unet_volume_mesh_host(vol.data(), D, H, W, values, 2, placement, nullptr, 0, nullptr, 0, st) == MI_UNET_OK);
        CHECK(st[0].value == 1 && st[0].placement == placement && st[0].quads == 52 + 6 && st[0].verts == 54 + 6);
        CHECK(st[0].quads_x == 2 * 6 + 2 && st[0].quads_y == 2 * 8 + 2 && st[0].quads_z == 2 * 12 + 2);
        CHECK(st[1].value == 2 && st[1].quads == 6 && st[1].verts == 8 && st[1].quads_x == 2 && st[1].quads_y == 2 && st[1].quads_z == 2);
        const int cv = (int)st[0].verts, cq = (int)st[0].quads;
        std::vector<mi_unet_mesh_vertex> verts(2 * (size_t)cv);
        std::vector<int32_t> quads(2 * (size_t)cq * 4, -7);
        mi_unet_mesh_stat again[2];
        CHECK(mi_unet_volume_mesh_host(vol.data(), D, H, W, values, 2, placement, verts.data(), cv, quads.data(), cq, again) == MI_UNET_OK);
        CHECK(std::memcmp(st, again, sizeof st) == 0);
        for (int i = 0; i < cv; ++i) {
            const mi_unet_mesh_vertex &v = verts[i];
            CHECK(v.n >= 1 && std::abs(v.ox) < v.n && std::abs(v.oy) < v.n && std::abs(v.oz) < v.n);
            CHECK(placement == MI_UNET_MESH_NETS ? v.n >= 3 : (v.n == 1 && !v.ox && !v.oy && !v.oz));
        }
        for (int i = 0; i < 4 * cq; ++i) CHECK(quads[i] >= 0 && quads[i] < cv);
        // the second plane: its eight vertices, its six quads, then zeros
        const mi_unet_mesh_vertex *v2 = verts.data() + cv;
        CHECK(v2[0].x == 8 && v2[0].y == 6 && v2[0].z == 4 && v2[7].x == 9 && v2[7].y == 7 && v2[7].z == 5 && v2[8].n == 0 && v2[cv - 1].n == 0);
        const int32_t *q2 = quads.data() + 4 * (size_t)cq;
        CHECK(q2[0] == 0 && q2[1] == 4 && q2[2] == 6 && q2[3] == 2);     // -x: (0,0,0) (0,0,1) (0,1,1) (0,1,0)
        for (int i = 24; i < 4 * cq; ++i) CHECK(q2[i] == 0);
        // the metrics: under FACES the box surface and the voxel count, in millimetres
        mi_unet_mesh_metrics m;
        CHECK(mi_unet_volume_mesh_derive(verts.data(), cv, quads.data(), cq, mm, &m) == MI_UNET_OK);
        const double vox = mm[0] * mm[1] * mm[2];
        if (placement == MI_UNET_MESH_FACES) {
            const double area = st[0].quads_x * mm[1] * mm[2] + st[0].quads_y * mm[0] * mm[2] + st[0].quads_z * mm[0] * mm[1];
            CHECK(std::fabs(m.area_mm2 - area) < 1e-9 * area && std::fabs(m.volume_mm3 - 25 * vox) < 1e-9 * 25 * vox);
        } else {
            CHECK(m.volume_mm3 > 0 && m.volume_mm3 < 25 * vox && m.area_mm2 > 0);
        }
        std::vector<float> xyz(3 * (size_t)cv, -1.f);
        CHECK(mi_unet_volume_mesh_positions(verts.data(), cv, mm, xyz.data()) == MI_UNET_OK);
        CHECK(xyz[0] == (float)((verts[0].x + verts[0].ox / (2.0 * verts[0].n)) * mm[0]));
        // caps at half: the same prefixes, zero tails, the same counts
        const int hv = cv / 2, hq = cq / 2;
        std::vector<mi_unet_mesh_vertex> pv(2 * (size_t)hv);
        std::vector<int32_t> pq(2 * (size_t)hq * 4, -7);
        CHECK(mi_unet_volume_mesh_host(vol.data(), D, H, W, values, 2, placement, pv.data(), hv, pq.data(), hq, again) == MI_UNET_OK);
        CHECK(std::memcmp(st, again, sizeof st) == 0);
        CHECK(std::memcmp(pv.data(), verts.data(), (size_t)hv * sizeof(mi_unet_mesh_vertex)) == 0);
        CHECK(std::memcmp(pq.data(), quads.data(), (size_t)hq * 4 * sizeof(int32_t)) == 0);
        CHECK(std::memcmp(pv.data() + hv, v2, 8 * sizeof(mi_unet_mesh_vertex)) == 0 && pv[(size_t)hv + 8].n == 0);
    }
    {   // one voxel that is the whole volume
        const uint8_t one = 7;
        const int v7 = 7;
        mi_unet_mesh_vertex verts[8];
        int32_t quads[24];
        mi_unet_mesh_stat st;
        CHECK(mi_unet_volume_mesh_host(&one, 1, 1, 1, &v7, 1, MI_UNET_MESH_NETS, verts, 8, quads, 6, &st) == MI_UNET_OK);
        CHECK(st.quads == 6 && st.verts == 8 && verts[0].n == 3 && verts[0].ox == 2 && verts[7].ox == -2 && verts[7].oz == -2);
    }
    {   // refused calls write nothing and say who refused
        mi_unet_mesh_stat st;
        std::memset(&st, 0x55, sizeof st);
        const mi_unet_mesh_stat before = st;
        int32_t q[4] = { 0, 1, 2, 3 };
        mi_unet_mesh_vertex v[3] = {};
        v[0].n = v[1].n = v[2].n = 1;
        mi_unet_mesh_metrics m = { -1.0, -1.0 };
        CHECK(mi_unet_volume_mesh_host(vol.data(), D, H, W, values, 2, 2, nullptr, 0, nullptr, 0, &st) == MI_UNET_EARG);
        CHECK(miunet::g_err.find("mi_unet_volume_mesh_host") == 0 && std::memcmp(&st, &before, sizeof st) == 0);
        CHECK(mi_unet_volume_mesh_host(vol.data(), D, H, W, values, 2, 0, nullptr, 1, nullptr, 0, &st) == MI_UNET_EARG);
        CHECK(mi_unet_volume_mesh_host(vol.data(), 1024, 1024, 1024, values, 2, 0, nullptr, 0, nullptr, 0, &st) == MI_UNET_EARG);
        CHECK(mi_unet_volume_mesh_derive(v, 3, q, 1, mm, &m) == MI_UNET_EARG && m.area_mm2 == -1.0);       // index 3 of 3
        CHECK(miunet::g_err.find("mi_unet_volume_mesh_derive") == 0);
        v[1].n = 0;
        q[3] = 2;
        CHECK(mi_unet_volume_mesh_derive(v, 3, q, 1, mm, &m) == MI_UNET_EARG && m.area_mm2 == -1.0);       // n == 0
        float xyz[9] = { -1.f };
        CHECK(mi_unet_volume_mesh_positions(v, 3, mm, xyz) == MI_UNET_EARG && xyz[0] == -1.f);
    }
    std::printf("volume_mesh_host_test ok\n");
    return 0;
}
