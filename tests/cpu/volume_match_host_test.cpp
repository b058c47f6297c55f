// The host half of the volume matching (csrc/volume_match.cpp with MIUNET_NO_DEVICE: mi_unet_volume_match_host,
// mi_unet_volume_match_assign and mi_unet_volume_match_derive) as a stand-alone program, so that it can run under
// -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE volume_match_host_test.cpp <csrc>/volume_match.cpp
// Cases: 3 x 5 x 9 (odd sizes) with two pred and three truth components, the last voxel of the volume and ids that belong to no
// component; exact-size buffers (an overrun is the sanitizer's to find); a short, an exact and a long pair list; m = 4096 on both sides;
// the assignment on both sides of a threshold and its scores; refused calls.  The numbers are checked against facts that hold by
// construction; tests/test_volume_match_cpu.py compares the same entry points with the reference.
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

static bool side_is(const mi_unet_vmatch_side &s, int voxels, int covered, int partners, int best, int best_voxels)
{
    return s.voxels == voxels && s.covered == covered && s.partners == partners && s.best == best && s.best_voxels == best_voxels;
}

int main()
{
    const int D = 3, H = 5, W = 9;
    const size_t n = (size_t)D * H * W;
    std::vector<int32_t> pred(n, 0), truth(n, 0);
    auto at = [&](std::vector<int32_t> &v, int z, int y, int x) -> int32_t & { return v[((size_t)z * H + y) * W + x]; };
    for (int x = 0; x < 6; ++x) at(pred, 0, 0, x) = 1;                  // pred 0: 6 voxels in a row
    for (int x = 2; x < 8; ++x) at(truth, 0, 0, x) = 1;                 // truth 0: the same moved by 2: intersection 4, union 8, IoU 1/2
    for (int x = 0; x < 9; ++x) at(pred, 1, 2, x) = 2;                  // pred 1: a whole row, over truth 1 (3 voxels) and truth 2 (3 voxels)
    for (int x = 0; x < 3; ++x) at(truth, 1, 2, x) = 2;
    for (int x = 6; x < 9; ++x) at(truth, 1, 2, x) = 3;
    at(pred, 2, 4, 8) = 3; at(truth, 2, 4, 8) = 4;                      // the last voxel of the volume: pred id 3 and truth id 4
    at(pred, 2, 0, 0) = -1; at(truth, 2, 0, 0) = 0;                     // no component on either side
    at(pred, 2, 0, 1) = 4097; at(truth, 2, 0, 1) = 4097;

    mi_unet_vmatch_side ps[2], ts[3];
    mi_unet_vmatch_pair pairs[3];
    int found = -1;
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 2, 3, 3, ps, ts, pairs, &found) == MI_UNET_OK);
    CHECK(found == 3);
    CHECK(side_is(ps[0], 6, 4, 1, 1, 4) && side_is(ps[1], 9, 6, 2, 2, 3));                  // the tie 3 : 3 goes to the smaller index
    CHECK(side_is(ts[0], 6, 4, 1, 1, 4) && side_is(ts[1], 3, 3, 1, 2, 3) && side_is(ts[2], 3, 3, 1, 2, 3));
    CHECK(pairs[0].p == 0 && pairs[0].t == 0 && pairs[0].voxels == 4 && pairs[1].p == 1 && pairs[1].t == 1 && pairs[1].voxels == 3);
    CHECK(pairs[2].p == 1 && pairs[2].t == 2 && pairs[2].voxels == 3);

    // a short list keeps the first pairs and the exact count; a long one has an all-zero tail
    mi_unet_vmatch_pair two[2], five[5];
    std::memset(five, 0x55, sizeof five);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 2, 3, 2, ps, ts, two, &found) == MI_UNET_OK && found == 3);
    CHECK(std::memcmp(two, pairs, sizeof two) == 0);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 2, 3, 5, ps, ts, five, &found) == MI_UNET_OK && found == 3);
    const mi_unet_vmatch_pair none[2] = { { 0, 0, 0 }, { 0, 0, 0 } };
    CHECK(std::memcmp(five, pairs, sizeof pairs) == 0 && std::memcmp(five + 3, none, sizeof none) == 0);

    // the assignment: at 1/2 the pair at exactly 1/2 is in; at 5/9 nothing is; at 1/65536 pred 1 takes truth 1 (3 / 9 twice: the index)
    int32_t of_p[2], of_t[3];
    mi_unet_vmatch_counts c;
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 3, pairs, 3, 3, 1, 2, of_p, of_t, &c) == MI_UNET_OK);
    CHECK(of_p[0] == 1 && of_p[1] == 0 && of_t[0] == 1 && of_t[1] == 0 && of_t[2] == 0 && c.tp == 1 && c.fp == 1 && c.fn == 2);
    mi_unet_vmatch_scores s;
    CHECK(mi_unet_volume_match_derive(ps, 2, ts, 3, pairs, 3, 3, of_p, &s) == MI_UNET_OK);
    CHECK(s.precision == 0.5 && std::fabs(s.recall - 1.0 / 3.0) < 1e-15 && s.f1 == 2.0 / 5.0 && s.sq == 0.5);
    CHECK(s.rq == 1.0 / 2.5 && s.pq == 0.5 * (1.0 / 2.5) && std::fabs(s.mean_dice - 2.0 / 3.0) < 1e-15);
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 3, pairs, 3, 3, 5, 9, of_p, of_t, &c) == MI_UNET_OK);
    CHECK(of_p[0] == 0 && of_p[1] == 0 && c.tp == 0 && c.fp == 2 && c.fn == 3);
    CHECK(mi_unet_volume_match_derive(ps, 2, ts, 3, pairs, 3, 3, of_p, &s) == MI_UNET_OK);
    CHECK(s.precision == 0.0 && s.recall == 0.0 && s.f1 == 0.0 && std::isnan(s.sq) && s.rq == 0.0 && std::isnan(s.pq) && std::isnan(s.mean_dice));
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 3, pairs, 3, 3, 1, 65536, of_p, of_t, &c) == MI_UNET_OK);
    CHECK(of_p[0] == 1 && of_p[1] == 2 && of_t[0] == 1 && of_t[1] == 2 && of_t[2] == 0 && c.tp == 2 && c.fp == 0 && c.fn == 1);

    // m = 4096 on both sides: the 67 MB table; pred id 3 and truth id 4 are components now
    std::vector<mi_unet_vmatch_side> bp(4096), bt(4096);
    std::vector<mi_unet_vmatch_pair> bq(4);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 4096, 4096, 4, bp.data(), bt.data(), bq.data(), &found) == MI_UNET_OK);
    CHECK(found == 4 && bq[3].p == 2 && bq[3].t == 3 && bq[3].voxels == 1 && side_is(bp[2], 1, 1, 1, 4, 1) && side_is(bt[3], 1, 1, 1, 3, 1));
    CHECK(side_is(bp[4095], 0, 0, 0, 0, 0) && std::memcmp(bp.data(), ps, sizeof ps) == 0);

    // one voxel that is the whole volume
    const int32_t one = 1;
    CHECK(mi_unet_volume_match_host(&one, &one, 1, 1, 1, 1, 1, 1, ps, ts, two, &found) == MI_UNET_OK);
    CHECK(found == 1 && side_is(ps[0], 1, 1, 1, 1, 1) && side_is(ts[0], 1, 1, 1, 1, 1) && two[0].voxels == 1);

    // refused calls
    CHECK(mi_unet_volume_match_host(nullptr, truth.data(), D, H, W, 2, 3, 3, ps, ts, pairs, &found) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 2, 3, 3, ps, ts, pairs, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), 0, H, W, 2, 3, 3, ps, ts, pairs, &found) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), 2048, 1024, 1024, 2, 3, 3, ps, ts, pairs, &found) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), 65536, 65536, 65536, 2, 3, 3, ps, ts, pairs, &found) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 0, 3, 3, ps, ts, pairs, &found) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 2, 4097, 3, ps, ts, pairs, &found) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_host(pred.data(), truth.data(), D, H, W, 2, 3, 0, ps, ts, pairs, &found) == MI_UNET_EARG && miunet::g_err.find("cap") != std::string::npos);
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 3, pairs, 3, 2, 1, 2, of_p, of_t, &c) == MI_UNET_EARG && miunet::g_err.find("truncated") != std::string::npos);
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 3, pairs, 3, 3, 0, 2, of_p, of_t, &c) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 3, pairs, 3, 3, 3, 2, of_p, of_t, &c) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 3, pairs, 3, 3, 1, 65537, of_p, of_t, &c) == MI_UNET_EARG);
    CHECK(mi_unet_volume_match_assign(ps, 2, ts, 2, pairs, 3, 3, 1, 2, of_p, of_t, &c) == MI_UNET_EARG);          // pair (1, 2) is outside two truth entries
    CHECK(mi_unet_volume_match_derive(ps, 2, ts, 3, pairs, 3, 2, of_p, &s) == MI_UNET_EARG);
    of_p[0] = 3;                                                        // (0, 2) is no pair
    CHECK(mi_unet_volume_match_derive(ps, 2, ts, 3, pairs, 3, 3, of_p, &s) == MI_UNET_EARG);
    std::printf("volume_match_host_test ok\n");
    return 0;
}
