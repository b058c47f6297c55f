// The host half of the scores against ground truth (csrc/score.cpp with MIUNET_NO_DEVICE: mi_unet_score_labels_host and
// mi_unet_score_derive) as a stand-alone program, so that it can run under -fsanitize=address,undefined on a CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DMIUNET_NO_DEVICE score_host_test.cpp <csrc>/score.cpp
// Cases: 33 x 70 (odd sizes) with two values and the confusion matrix, the three empty-set cases, a refused call.  The numbers are
// checked against facts that hold by construction; tests/test_score_cpu.py compares the same entry points with the reference.
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
    const int H = 33, W = 70;
    std::vector<uint8_t> pred((size_t)H * W, 0), truth((size_t)H * W, 0);
    for (int y = 5; y < 25; ++y)
        for (int x = 10; x < 50; ++x) pred[(size_t)y * W + x] = 1;
    for (int y = 7; y < 27; ++y)
        for (int x = 13; x < 53; ++x) truth[(size_t)y * W + x] = 1;          // the same box moved by (3, 2)
    pred[0] = 2; truth[(size_t)H * W - 1] = 2; truth[5] = 200;
    const int values[2] = { 1, 2 };
    const mi_unet_score_opts opts{ 0, 3 };
    mi_unet_score s[2];
    std::vector<int64_t> conf(9);
    int64_t skipped = -1;
    CHECK(mi_unet_score_labels_host(pred.data(), truth.data(), 1, H, W, values, 2, &opts, s, conf.data(), &skipped) == MI_UNET_OK);
    CHECK(s[0].tp == 18 * 37 && s[0].fp == 20 * 40 - 18 * 37 && s[0].fn == s[0].fp);
    CHECK(s[0].a_to_t.n == 2 * 20 + 2 * 40 - 4 && s[0].t_to_a.n == s[0].a_to_t.n);
    CHECK(s[0].a_to_t.max_d2 == 13 && s[0].t_to_a.max_d2 == 13 && s[0].q_d2_sym == 13 && s[0].a_to_t.q_d2 == 13);     // corner to corner: 3^2 + 2^2
    CHECK(s[1].a_to_t.n == 1 && s[1].a_to_t.max_d2 == 32 * 32 + 69 * 69 && s[1].tp == 0);
    CHECK(s[1].a_to_t.sum_d_q16 == (int64_t)std::floor(65536.0 * std::sqrt(32.0 * 32 + 69.0 * 69)));
    int64_t total = skipped;
    for (int64_t v : conf) total += v;
    CHECK(total == (int64_t)H * W && skipped == 1 && conf[1 * 3 + 1] == s[0].tp);
    mi_unet_score_metrics m;
    CHECK(mi_unet_score_derive(&s[0], &m) == MI_UNET_OK && m.hd == std::sqrt(13.0) && m.dice > 0.8 && m.dice < 1.0 && m.assd > 0.0);

    std::vector<uint8_t> none((size_t)H * W, 0);
    const uint8_t *pairs[3][2] = { { none.data(), truth.data() }, { pred.data(), none.data() }, { none.data(), none.data() } };
    for (int c = 0; c < 3; ++c) {
        mi_unet_score e;
        CHECK(mi_unet_score_labels_host(pairs[c][0], pairs[c][1], 1, H, W, values, 1, nullptr, &e, nullptr, nullptr) == MI_UNET_OK);
        CHECK(e.a_to_t.max_d2 == -1 && e.t_to_a.q_d2 == -1 && e.q_d2_sym == -1 && e.a_to_t.sum_d2 == 0 && e.t_to_a.sum_d_q16 == 0);
        CHECK(e.tp == 0 && e.quantile_ppm == 50000 && (e.a_to_t.n > 0) == (c == 1) && (e.t_to_a.n > 0) == (c == 0));
        CHECK(mi_unet_score_derive(&e, &m) == MI_UNET_OK && std::isnan(m.hd) && std::isnan(m.assd) && m.dice == (c == 2 ? 1.0 : 0.0));
    }
    mi_unet_score keep;
    std::memset(&keep, 0x55, sizeof keep);
    const int twice[2] = { 1, 1 };
    CHECK(mi_unet_score_labels_host(pred.data(), truth.data(), 1, H, W, twice, 2, nullptr, &keep, nullptr, nullptr) == MI_UNET_EARG);
    CHECK(reinterpret_cast<const uint8_t *>(&keep)[0] == 0x55 && !miunet::g_err.empty());
    std::printf("score_host_test ok\n");
    return 0;
}
