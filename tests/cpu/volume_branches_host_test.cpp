// The host half of the volume branch graph (csrc/volume_branches.cpp with MIUNET_NO_DEVICE: mi_unet_volume_branches_host,
// mi_unet_volume_branches_derive_branch and mi_unet_volume_branches_derive) as a stand-alone program, so that it can run under
// -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_branches_host_test.cpp <csrc>/volume_branches.cpp
// Cases: a Y of three arms in a 3 x 9 x 11 volume (odd sizes) with a second id beside it, values outside 1 .. m and a radius field; the same
// Y with its short arm pruned; tables that are too small and absent; a ring; a full block, which is one cluster; refused calls.  The
// numbers are checked against facts that hold by construction; tests/test_volume_branches_cpu.py compares the same entry points with
// the reference.
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
    const int units[3] = { 1, 1, 1 };
    const double sp[3] = { 0.5, 0.75, 1.25 };
    {   // id 2: a junction at (y, x) = (4, 5) of the slice z = 1, diagonal arms of four voxels down to (8, 1) and (8, 9), an arm of two
        // voxels up to (2, 5); id 1: one voxel beside the upper end; a value above m and a negative one
        const int D = 3, H = 9, W = 11;
        const size_t n = (size_t)D * H * W;
        auto idx = [&](int z, int y, int x) { return ((size_t)z * H + y) * W + x; };
        std::vector<int32_t> ids(n, 0), r2(n, 0), map(n, -7), out(n, -7);
        ids[idx(1, 4, 5)] = 2;
        for (int k = 1; k <= 4; ++k) ids[idx(1, 4 + k, 5 - k)] = ids[idx(1, 4 + k, 5 + k)] = 2;
        ids[idx(1, 3, 5)] = ids[idx(1, 2, 5)] = 2;
        ids[idx(1, 1, 6)] = 1;
        ids[idx(0, 0, 0)] = 9;
        ids[idx(2, 8, 10)] = -3;
        for (size_t i = 0; i < n; ++i) r2[i] = ids[i] > 0 ? (int32_t)(i % 7) + 1 : 0;
        mi_unet_vnode nodes[8];
        mi_unet_vbranch rows[8];
        mi_unet_vgraph g[3];
        mi_unet_vbranch_info info;
        CHECK(mi_unet_volume_branches_host(ids.data(), r2.data(), D, H, W, 3, units, nullptr, nodes, 8, rows, 8, g, map.data(), out.data(), &info) == MI_UNET_OK);
        CHECK(info.found_nodes == 5 && info.found_branches == 3 && info.rounds == 0 && info.stable == 1);
        // nodes by first voxel: the isolated voxel of id 1, the upper end, the junction, the two lower ends
        CHECK(nodes[0].id == 1 && nodes[0].kind == 0 && nodes[0].first == (int64_t)idx(1, 1, 6) && nodes[0].degree == 0);
        CHECK(nodes[1].kind == 1 && nodes[1].first == (int64_t)idx(1, 2, 5) && nodes[1].degree == 1 && nodes[1].sy == 2 && nodes[1].sx == 5 && nodes[1].sz == 1);
        CHECK(nodes[2].kind == 2 && nodes[2].first == (int64_t)idx(1, 4, 5) && nodes[2].degree == 3 && nodes[2].voxels == 1);
        CHECK(nodes[3].kind == 1 && nodes[4].kind == 1 && nodes[2].r2_min == r2[idx(1, 4, 5)] && nodes[2].r2_max == r2[idx(1, 4, 5)]);
        // branches by key: the upper arm (one voxel), then the two lower arms (three voxels each, four diagonal links)
        CHECK(rows[0].first == (int64_t)idx(1, 3, 5) && rows[0].kind == 0 && rows[0].voxels == 1 && rows[0].node_a == 1 && rows[0].node_b == 2);
        CHECK(rows[0].links[1] == 2 && rows[0].r2_sum == r2[idx(1, 3, 5)] && rows[0].att_lo == (int64_t)idx(1, 2, 5) && rows[0].att_hi == (int64_t)idx(1, 4, 5));
        CHECK(rows[1].voxels == 3 && rows[1].links[2] == 4 && rows[1].node_a == 2 && rows[1].node_b == 3 && rows[2].voxels == 3 && rows[2].node_b == 4);
        CHECK(g[1].nodes == 4 && g[1].ends == 3 && g[1].junction_nodes == 1 && g[1].junction_voxels == 1 && g[1].branches == 3 && g[1].closed == 0);
        CHECK(g[1].links[1] == 2 && g[1].links[2] == 8 && g[0].nodes == 1 && g[0].isolated == 1 && g[2].nodes == 0 && g[2].branches == 0);
        CHECK(map[idx(1, 3, 5)] == 1 && map[idx(1, 4, 5)] == -3 && map[idx(1, 1, 6)] == -1 && map[idx(0, 0, 0)] == 0 && out[idx(0, 0, 0)] == 0 && out[idx(1, 4, 5)] == 2);
        mi_unet_vbranch_metrics bm;
        CHECK(mi_unet_volume_branches_derive_branch(&rows[0], H, W, sp, 0.25, &bm) == MI_UNET_OK);
        CHECK(bm.length_mm == 2 * 0.75 && bm.chord_mm == 2 * 0.75 && bm.tortuosity == 1.0 && bm.radius_rms_mm == std::sqrt((double)rows[0].r2_sum) * 0.25);
        mi_unet_vgraph_metrics gm;
        CHECK(mi_unet_volume_branches_derive(&g[1], rows, 3, info.found_nodes, 2, sp, 0.25, &gm) == MI_UNET_OK && gm.parts == 1 && gm.loops == 0);
        CHECK(gm.length_mm == 2 * 0.75 + 8 * std::sqrt(0.5 * 0.5 + 0.75 * 0.75));
        CHECK(mi_unet_volume_branches_derive(&g[0], rows, 3, info.found_nodes, 1, sp, 0.25, &gm) == MI_UNET_OK && gm.parts == 1 && gm.loops == 0);
        CHECK(mi_unet_volume_branches_derive(&g[1], rows, 2, info.found_nodes, 2, sp, 0.25, &gm) == MI_UNET_EARG);     // a truncated table
        // tables that are too small: the first rows, the counts unchanged, nothing behind the cap touched; absent tables
        mi_unet_vnode few_nodes[3];
        mi_unet_vbranch few_rows[2];
        std::memset(few_nodes, 0x55, sizeof few_nodes);
        std::memset(few_rows, 0x55, sizeof few_rows);
        CHECK(mi_unet_volume_branches_host(ids.data(), r2.data(), D, H, W, 3, units, nullptr, few_nodes, 2, few_rows, 1, g, nullptr, nullptr, &info) == MI_UNET_OK);
        CHECK(info.found_nodes == 5 && info.found_branches == 3 && std::memcmp(few_nodes, nodes, 2 * sizeof nodes[0]) == 0 && std::memcmp(few_rows, rows, sizeof rows[0]) == 0);
        CHECK(reinterpret_cast<const uint8_t *>(&few_nodes[2])[0] == 0x55 && reinterpret_cast<const uint8_t *>(&few_rows[1])[0] == 0x55);
        CHECK(mi_unet_volume_branches_host(ids.data(), nullptr, D, H, W, 3, units, nullptr, nullptr, 0, nullptr, 0, g, nullptr, nullptr, nullptr) == MI_UNET_OK);
        CHECK(g[1].branches == 3);
        // the upper arm is a spur of two voxels: prune 1 leaves it, prune 2 takes it and the junction becomes a branch voxel
        const mi_unet_vbranch_opts p1{ 1, 0 }, p2{ 2, 0 };
        CHECK(mi_unet_volume_branches_host(ids.data(), nullptr, D, H, W, 3, units, &p1, nodes, 8, rows, 8, g, nullptr, nullptr, &info) == MI_UNET_OK);
        CHECK(info.rounds == 0 && info.stable == 1 && info.found_branches == 3 && g[1].pruned_spurs == 0);
        CHECK(mi_unet_volume_branches_host(ids.data(), nullptr, D, H, W, 3, units, &p2, nodes, 8, rows, 8, g, map.data(), out.data(), &info) == MI_UNET_OK);
        CHECK(info.rounds == 1 && info.stable == 1 && info.found_nodes == 3 && info.found_branches == 1 && g[1].pruned_spurs == 1 && g[1].pruned_voxels == 2);
        CHECK(rows[0].voxels == 7 && rows[0].r2_min == 0 && rows[0].r2_sum == 0 && out[idx(1, 3, 5)] == 0 && out[idx(1, 2, 5)] == 0 && map[idx(1, 4, 5)] == 1);
    }
    {   // a ring of twelve voxels: one closed branch, no node; a full block: every voxel a junction voxel, one node
        const int D = 3, H = 9, W = 9;
        std::vector<int32_t> ids((size_t)D * H * W, 0);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (std::abs(y - 4) + std::abs(x - 4) == 3) ids[((size_t)1 * H + y) * W + x] = 1;
        mi_unet_vbranch row;
        mi_unet_vgraph g;
        mi_unet_vbranch_info info;
        CHECK(mi_unet_volume_branches_host(ids.data(), nullptr, D, H, W, 1, units, nullptr, nullptr, 0, &row, 1, &g, nullptr, nullptr, &info) == MI_UNET_OK);
        CHECK(info.found_nodes == 0 && info.found_branches == 1 && row.kind == 1 && row.att_lo == -1 && row.node_b == -1 && row.voxels == 12 && row.links[2] == 12);
        mi_unet_vbranch_metrics bm;
        mi_unet_vgraph_metrics gm;
        CHECK(mi_unet_volume_branches_derive_branch(&row, H, W, sp, 0.25, &bm) == MI_UNET_OK && bm.chord_mm == 0.0 && bm.tortuosity == 0.0);
        CHECK(mi_unet_volume_branches_derive(&g, &row, 1, 0, 1, sp, 0.25, &gm) == MI_UNET_OK && gm.parts == 1 && gm.loops == 1);
        std::vector<int32_t> full(2 * 3 * 4, 1);
        mi_unet_vnode node;
        CHECK(mi_unet_volume_branches_host(full.data(), nullptr, 2, 3, 4, 1, units, nullptr, &node, 1, nullptr, 0, &g, nullptr, nullptr, &info) == MI_UNET_OK);
        CHECK(info.found_nodes == 1 && info.found_branches == 0 && node.kind == 2 && node.voxels == 24 && node.first == 0 && node.sx == 36 && g.junction_voxels == 24);
    }
    std::vector<int32_t> ids(2 * 3 * 4, 1);
    mi_unet_vgraph keep;
    mi_unet_vnode node;
    mi_unet_vbranch row;
    std::memset(&keep, 0x55, sizeof keep);
    mi_unet_vbranch_info info{ 7, 7, 7, 7 };
    const int zero_unit[3] = { 1, 0, 1 }, big_unit[3] = { 1, 1, 15447 };      // (3 * 15447 = 46341)
    const mi_unet_vbranch_opts bad_prune{ -1, 0 }, bad_rounds{ 0, (1 << 20) + 1 };
    auto call = [&](const int32_t *in, int D, int m, const int *un, const mi_unet_vbranch_opts *o, mi_unet_vnode *nd, int cn, mi_unet_vbranch *br, int cb,
                    mi_unet_vgraph *g) { return mi_unet_volume_branches_host(in, nullptr, D, 3, 4, m, un, o, nd, cn, br, cb, g, nullptr, nullptr, &info); };
    CHECK(call(nullptr, 2, 1, units, nullptr, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, nullptr, nullptr, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, units, nullptr, &node, 1, &row, 1, nullptr) == MI_UNET_EARG);
    CHECK(call(ids.data(), 0, 1, units, nullptr, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 0, units, nullptr, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 4097, units, nullptr, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, zero_unit, nullptr, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, big_unit, nullptr, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, units, &bad_prune, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, units, &bad_rounds, &node, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, units, nullptr, nullptr, 1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, units, nullptr, &node, 1, nullptr, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, units, nullptr, &node, -1, &row, 1, &keep) == MI_UNET_EARG);
    CHECK(call(ids.data(), 2, 1, units, nullptr, &node, 1, &row, (1 << 20) + 1, &keep) == MI_UNET_EARG);
    CHECK(reinterpret_cast<const uint8_t *>(&keep)[0] == 0x55 && info.rounds == 7 && miunet::g_err.rfind("mi_unet_volume_branches_host:", 0) == 0);
    std::printf("volume_branches_host_test ok\n");
    return 0;
}
