// The host half of the scores of a volume (csrc/score_volume.cpp and csrc/score.cpp with MIUNET_NO_DEVICE:
// mi_unet_score_volume_host, mi_unet_score_volume_units, mi_unet_score_volume_derive) as a stand-alone program, so that it can run under
// -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE score_volume_host_test.cpp
//       <csrc>/score_volume.cpp <csrc>/score.cpp          (one command)
// Cases: two boxes in 7 x 33 x 70 (odd sizes) under an anisotropic spacing with the confusion matrix, one slice, one row, one column of
// slices, the empty-set cases, the unit helper, derive, refused calls.  The numbers are checked against facts that hold by construction;
// tests/test_score_volume_cpu.py compares the same entry points with the reference.
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

static void box(std::vector<uint8_t> &v, int H, int W, int z0, int z1, int y0, int y1, int x0, int x1, uint8_t value)
{
    for (int z = z0; z < z1; ++z)
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) v[((size_t)z * H + y) * W + x] = value;
}

int main()
{
    const int D = 7, H = 33, W = 70;
    const size_t dhw = (size_t)D * H * W;
    std::vector<uint8_t> pred(dhw, 0), truth(dhw, 0);
    box(pred, H, W, 1, 5, 5, 25, 10, 50, 1);                    // 4 x 20 x 40
    box(truth, H, W, 2, 6, 7, 27, 13, 53, 1);                   // the same box moved by (dz, dy, dx) = (1, 2, 3)
    pred[0] = 2; truth[dhw - 1] = 2; truth[5] = 200;
    const int values[2] = { 1, 2 }, units[3] = { 2, 3, 10 };
    const mi_unet_score_opts opts{ 0, 3 };
    mi_unet_score s[2];
    std::vector<int64_t> conf(9);
    int64_t skipped = -1;
    CHECK(mi_unet_score_volume_host(pred.data(), truth.data(), D, H, W, values, 2, units, &opts, s, conf.data(), &skipped) == MI_UNET_OK);
    CHECK(s[0].tp == 3 * 18 * 37 && s[0].fp == 4 * 20 * 40 - 3 * 18 * 37 && s[0].fn == s[0].fp);
    const int shell = 4 * 20 * 40 - 2 * 18 * 38;                // the box without its interior
    CHECK(s[0].a_to_t.n == shell && s[0].t_to_a.n == shell);
    // corner to corner: (3 * 2)^2 + (2 * 3)^2 + (1 * 10)^2
    CHECK(s[0].a_to_t.max_d2 == 172 && s[0].t_to_a.max_d2 == 172 && s[0].q_d2_sym == 172 && s[0].a_to_t.q_d2 == 172);
    const int far = (69 * 2) * (69 * 2) + (32 * 3) * (32 * 3) + (6 * 10) * (6 * 10);
    CHECK(s[1].a_to_t.n == 1 && s[1].a_to_t.max_d2 == far && s[1].tp == 0 && s[1].t_to_a.sum_d2 == far);
    CHECK(s[1].a_to_t.sum_d_q16 == (int64_t)std::floor(65536.0 * std::sqrt((double)far)));
    int64_t total = skipped;
    for (int64_t v : conf) total += v;
    CHECK(total == (int64_t)dhw && skipped == 1 && conf[1 * 3 + 1] == s[0].tp);
    mi_unet_score_metrics m, plain;
    CHECK(mi_unet_score_volume_derive(&s[0], 0.1, &m) == MI_UNET_OK && mi_unet_score_derive(&s[0], &plain) == MI_UNET_OK);
    CHECK(m.hd == std::sqrt(172.0) * 0.1 && m.dice == plain.dice && m.assd == plain.assd * 0.1 && m.assd > 0.0);

    // one slice: every voxel of a set is a boundary voxel
    mi_unet_score one;
    CHECK(mi_unet_score_volume_host(pred.data() + (size_t)2 * H * W, truth.data() + (size_t)2 * H * W, 1, H, W, values, 1, units, nullptr, &one, nullptr, nullptr) == MI_UNET_OK);
    CHECK(one.a_to_t.n == 20 * 40 && one.t_to_a.n == 20 * 40 && one.quantile_ppm == 50000 && one.a_to_t.max_d2 == 6 * 6 + 6 * 6);
    // one row of W voxels, one column of D slices: two single voxels
    std::vector<uint8_t> lp(130, 0), lt(130, 0);
    lp[3] = 1; lt[120] = 1;
    CHECK(mi_unet_score_volume_host(lp.data(), lt.data(), 1, 1, 130, values, 1, units, nullptr, &one, nullptr, nullptr) == MI_UNET_OK);
    CHECK(one.a_to_t.max_d2 == (117 * 2) * (117 * 2) && one.t_to_a.n == 1);
    CHECK(mi_unet_score_volume_host(lp.data(), lt.data(), 130, 1, 1, values, 1, units, nullptr, &one, nullptr, nullptr) == MI_UNET_OK);
    CHECK(one.a_to_t.max_d2 == (117 * 10) * (117 * 10) && one.q_d2_sym == one.a_to_t.max_d2);

    std::vector<uint8_t> none(dhw, 0);
    const uint8_t *pairs[3][2] = { { none.data(), truth.data() }, { pred.data(), none.data() }, { none.data(), none.data() } };
    for (int c = 0; c < 3; ++c) {
        mi_unet_score e;
        CHECK(mi_unet_score_volume_host(pairs[c][0], pairs[c][1], D, H, W, values, 1, units, nullptr, &e, nullptr, nullptr) == MI_UNET_OK);
        CHECK(e.a_to_t.max_d2 == -1 && e.t_to_a.q_d2 == -1 && e.q_d2_sym == -1 && e.a_to_t.sum_d2 == 0 && e.t_to_a.sum_d_q16 == 0);
        CHECK(e.tp == 0 && (e.a_to_t.n > 0) == (c == 1) && (e.t_to_a.n > 0) == (c == 0));
        CHECK(mi_unet_score_volume_derive(&e, 0.1, &m) == MI_UNET_OK && std::isnan(m.hd) && std::isnan(m.assd) && m.dice == (c == 2 ? 1.0 : 0.0));
    }

    const double mm[3] = { 0.7, 0.7, 5.0 };
    int u[3] = { -1, -1, -1 };
    double unit = -1.0;
    CHECK(mi_unet_score_volume_units(mm, 64, 512, 512, u, &unit) == MI_UNET_OK && u[0] == 7 && u[1] == 7 && u[2] == 50 && unit == 0.1);
    const double bad[3] = { 0.7, std::nan(""), 5.0 };
    CHECK(mi_unet_score_volume_units(bad, 64, 512, 512, u, &unit) == MI_UNET_EARG && u[2] == 50);
    const double big[3] = { 4.0, 4.0, 4.0 };
    CHECK(mi_unet_score_volume_units(big, 8192, 8192, 8192, u, &unit) == MI_UNET_EARG && unit == 0.1);
    CHECK(mi_unet_score_volume_derive(&s[0], 0.0, &m) == MI_UNET_EARG && mi_unet_score_volume_derive(nullptr, 1.0, &m) == MI_UNET_EARG);

    mi_unet_score keep;
    std::memset(&keep, 0x55, sizeof keep);
    const int twice[2] = { 1, 1 }, limit[3] = { 46341, 1, 1 }, zero[3] = { 1, 0, 1 };
    miunet::g_err.clear();
    CHECK(mi_unet_score_volume_host(pred.data(), truth.data(), D, H, W, twice, 2, units, nullptr, &keep, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_score_volume_host(pred.data(), truth.data(), D, H, W, values, 1, limit, nullptr, &keep, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_score_volume_host(pred.data(), truth.data(), D, H, W, values, 1, zero, nullptr, &keep, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(mi_unet_score_volume_host(pred.data(), truth.data(), D, 8193, W, values, 1, units, nullptr, &keep, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(reinterpret_cast<const uint8_t *>(&keep)[0] == 0x55 && reinterpret_cast<const uint8_t *>(&keep)[87] == 0x55 && !miunet::g_err.empty());
    std::printf("score_volume_host_test ok\n");
    return 0;
}
