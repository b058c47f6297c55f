// score.cpp -- scores against ground truth (include/mi_unet.h: mi_unet_score_labels): the argument checks, the
// definition as pure host arithmetic (mi_unet_score_labels_host), the derived metrics (mi_unet_score_derive) and the entry point on
// the handle, which owns the stage's workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h;
// tests/cpu/score_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_score_dir) == 32, "mi_unet_score_dir is 32 bytes without padding");
static_assert(sizeof(mi_unet_score) == 88, "mi_unet_score is 88 bytes without padding");

namespace miunet {

namespace {

constexpr mi_unet_score_opts kDefaultScoreOpts{ 50000, 0 };

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_score_args(const char *fn, const uint8_t *pred, const uint8_t *truth, int B, int H, int W, const int *values, int n,
                     const mi_unet_score_opts &o, const mi_unet_score *scores, const int64_t *confusion, const int64_t *skipped)
{
    const std::string f = fn;
    if (!pred || !truth || !values || !scores) return fail(MI_UNET_EARG, f + ": null argument");
    if (B < 1) return fail(MI_UNET_EARG, f + ": B = " + std::to_string(B) + " (at least one image)");
    if (int rc = check_values(f, values, n, MI_UNET_SCORE_MAX_VALUES)) return rc;
    if (o.quantile_ppm < 0 || o.quantile_ppm > 999999)
        return fail(MI_UNET_EARG, f + ": quantile_ppm " + std::to_string(o.quantile_ppm) + " is outside 0 .. 999999");
    if (o.classes < 0 || o.classes > MI_UNET_SCORE_MAX_CLASSES)
        return fail(MI_UNET_EARG, f + ": classes " + std::to_string(o.classes) + " is outside 0 .. " + std::to_string(MI_UNET_SCORE_MAX_CLASSES));
    if (confusion && o.classes == 0) return fail(MI_UNET_EARG, f + ": a confusion matrix needs classes >= 1");
    if (confusion && !skipped) return fail(MI_UNET_EARG, f + ": a confusion matrix needs the skipped counts beside it");
    if (H < 1 || W < 1 || H > 32767 || W > 32767)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(H) + " x " + std::to_string(W) + " is outside 1 .. 32767 per side");
    // step by step: B * n * H * W itself could pass 64 bits (B near 2^31, n = 8, H = W = 32767)
    if ((long long)B * n > MI_UNET_SCORE_MAX_PLANES)
        return fail(MI_UNET_EARG, f + ": B * n = " + std::to_string((long long)B * n) + " planes (at most " + std::to_string(MI_UNET_SCORE_MAX_PLANES) + ")");
    if ((long long)B * n > 0x7FFFFFFFLL / ((long long)H * W)) return fail(MI_UNET_EARG, f + ": B * n * H * W must stay below 2^31");
    return MI_UNET_OK;
}

// floor(2^16 sqrt(d2)): the integer square root of d2 << 32 (the fp64 root, corrected to the exact floor)
uint64_t sqrt_q16(int32_t d2)
{
    const uint64_t v = (uint64_t)(uint32_t)d2 << 32;
    uint64_t r = (uint64_t)std::sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

constexpr int32_t kNoColumn = std::numeric_limits<int32_t>::max();     // g of a column without a boundary pixel

// boundary pixels of { map == v } and, for every pixel, the vertical distance to the nearest one of its column
void boundary_columns(const uint8_t *map, int H, int W, int v, std::vector<uint8_t> &bnd, std::vector<int32_t> &g, int32_t &count)
{
    const size_t hw = (size_t)H * W;
    bnd.assign(hw, 0);
    g.assign(hw, kNoColumn);
    count = 0;
    auto in = [&](int y, int x) { return y >= 0 && y < H && x >= 0 && x < W && map[(size_t)y * W + x] == v; };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            if (in(y, x) && !(in(y - 1, x) && in(y + 1, x) && in(y, x - 1) && in(y, x + 1))) { bnd[(size_t)y * W + x] = 1; ++count; }
    for (int x = 0; x < W; ++x) {
        int32_t d = kNoColumn;
        for (int y = 0; y < H; ++y) {
            d = bnd[(size_t)y * W + x] ? 0 : d == kNoColumn ? kNoColumn : d + 1;
            g[(size_t)y * W + x] = d;
        }
        d = kNoColumn;
        for (int y = H - 1; y >= 0; --y) {
            d = bnd[(size_t)y * W + x] ? 0 : d == kNoColumn ? kNoColumn : d + 1;
            g[(size_t)y * W + x] = std::min(g[(size_t)y * W + x], d);
        }
    }
}

// d2 of every boundary pixel of the source set to the set whose column distances are g, in raster order (g holds a finite entry)
void directed_d2(const std::vector<uint8_t> &src_bnd, const std::vector<int32_t> &g, int H, int W, std::vector<int32_t> &out)
{
    out.clear();
    for (int y = 0; y < H; ++y) {
        const int32_t *const row = g.data() + (size_t)y * W;
        for (int x = 0; x < W; ++x) {
            if (!src_bnd[(size_t)y * W + x]) continue;
            int64_t best = std::numeric_limits<int64_t>::max();
            for (int xx = 0; xx < W; ++xx) {
                if (row[xx] == kNoColumn) continue;
                const int64_t dx = x - xx;
                best = std::min(best, dx * dx + (int64_t)row[xx] * row[xx]);
            }
            out.push_back((int32_t)best);
        }
    }
}

int32_t order_stat(std::vector<int32_t> &v, int quantile_ppm)          // s[n - 1 - floor(n * ppm / 1e6)] of the n values
{
    const uint64_t n = v.size(), k = n * (uint64_t)quantile_ppm / 1000000ull;
    std::nth_element(v.begin(), v.begin() + (n - 1 - k), v.end());
    return v[n - 1 - k];
}

mi_unet_score_dir direction(std::vector<int32_t> &d2, int32_t n, bool have, int quantile_ppm)
{
    mi_unet_score_dir r{ n, -1, -1, 0, 0, 0 };
    if (!have) return r;
    r.max_d2 = 0;
    for (int32_t d : d2) {
        r.max_d2 = std::max(r.max_d2, d);
        r.sum_d2 += d;
        r.sum_d_q16 += (int64_t)sqrt_q16(d);
    }
    r.q_d2 = order_stat(d2, quantile_ppm);
    return r;
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_score_labels_host(const uint8_t *pred, const uint8_t *truth, int B, int H, int W, const int *values, int n,
                              const mi_unet_score_opts *opts, mi_unet_score *scores, int64_t *confusion, int64_t *skipped)
{
    const mi_unet_score_opts o = opts ? *opts : kDefaultScoreOpts;
    if (int rc = check_score_args("mi_unet_score_labels_host", pred, truth, B, H, W, values, n, o, scores, confusion, skipped)) return rc;
    const size_t hw = (size_t)H * W;
    std::vector<uint8_t> bnd_a, bnd_t;
    std::vector<int32_t> g_a, g_t, d_a, d_t;
    for (int b = 0; b < B; ++b) {
        const uint8_t *const p = pred + b * hw, *const t = truth + b * hw;
        for (int k = 0; k < n; ++k) {
            const int v = values[k];
            mi_unet_score s{};
            for (size_t i = 0; i < hw; ++i) {
                const bool a = p[i] == v, tt = t[i] == v;
                s.tp += a && tt; s.fp += a && !tt; s.fn += tt && !a;
            }
            s.value = v;
            s.quantile_ppm = o.quantile_ppm;
            int32_t n_a = 0, n_t = 0;
            boundary_columns(p, H, W, v, bnd_a, g_a, n_a);
            boundary_columns(t, H, W, v, bnd_t, g_t, n_t);
            const bool have = n_a > 0 && n_t > 0;
            d_a.clear(); d_t.clear();
            if (have) {
                directed_d2(bnd_a, g_t, H, W, d_a);
                directed_d2(bnd_t, g_a, H, W, d_t);
            }
            s.a_to_t = direction(d_a, n_a, have, o.quantile_ppm);
            s.t_to_a = direction(d_t, n_t, have, o.quantile_ppm);
            s.q_d2_sym = -1;
            if (have) {
                d_a.insert(d_a.end(), d_t.begin(), d_t.end());
                s.q_d2_sym = order_stat(d_a, o.quantile_ppm);
            }
            scores[(size_t)b * n + k] = s;
        }
        if (confusion) {
            const int c = o.classes;
            int64_t *const m = confusion + (size_t)b * c * c;
            std::fill(m, m + (size_t)c * c, 0);
            int64_t skip = 0;
            for (size_t i = 0; i < hw; ++i) {
                if (p[i] < c && t[i] < c) ++m[(size_t)t[i] * c + p[i]];
                else ++skip;
            }
            skipped[b] = skip;
        }
    }
    return MI_UNET_OK;
}

int mi_unet_score_derive(const mi_unet_score *s, mi_unet_score_metrics *out)
{
    if (!s || !out) return fail(MI_UNET_EARG, "mi_unet_score_derive: null argument");
    const double tp = s->tp, fp = s->fp, fn = s->fn;
    auto ratio = [](double num, double den) { return den == 0.0 ? 1.0 : num / den; };
    out->dice = ratio(2.0 * tp, 2.0 * tp + fp + fn);
    out->iou = ratio(tp, tp + fp + fn);
    out->precision = ratio(tp, tp + fp);
    out->recall = ratio(tp, tp + fn);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out->hd = out->hd_q = out->assd = out->rmsd = nan;
    const mi_unet_score_dir &a = s->a_to_t, &t = s->t_to_a;
    if (a.max_d2 >= 0 && t.max_d2 >= 0 && s->q_d2_sym >= 0 && a.n > 0 && t.n > 0) {
        const double cnt = (double)a.n + (double)t.n;
        out->hd = std::sqrt((double)std::max(a.max_d2, t.max_d2));
        out->hd_q = std::sqrt((double)s->q_d2_sym);
        out->assd = (double)(a.sum_d_q16 + t.sum_d_q16) / 65536.0 / cnt;
        out->rmsd = std::sqrt((double)(a.sum_d2 + t.sum_d2) / cnt);
    }
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_score_labels(mi_unet_t *h, const uint8_t *pred, const uint8_t *truth, int B, int H, int W, const int *values, int n,
                         const mi_unet_score_opts *opts, mi_unet_score *scores, int64_t *confusion, int64_t *skipped)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_score_opts o = opts ? *opts : kDefaultScoreOpts;
    if (int rc = check_score_args("mi_unet_score_labels", pred, truth, B, H, W, values, n, o, scores, confusion, skipped)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int classes = confusion ? o.classes : 0;
    const size_t map_bytes = (size_t)B * H * W, P = (size_t)B * n;
    // device: both maps, the scores, the kernels' workspace; pinned: both maps, the scores, the matrix with its skipped counts
    const size_t at_truth = up256(map_bytes), at_scores = at_truth + up256(map_bytes), at_ws = at_scores + up256(P * sizeof(mi_unet_score));
    const size_t conf_bytes = (size_t)B * ((size_t)classes * classes + 1) * sizeof(int64_t);
    const size_t dev_need = at_ws + score_workspace_bytes(B, H, W, n, classes), host_need = at_ws + conf_bytes;
    hipStream_t s = h->stream;
    if (int rc = h->ws_score.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_score.d, *const p = h->ws_score.p;
    host_copy(h, p, pred, map_bytes);
    host_copy(h, p + at_truth, truth, map_bytes);
    HIP_TRY(hipMemcpyAsync(d, p, map_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + at_truth, p + at_truth, map_bytes, hipMemcpyHostToDevice, s));
    ScoreValues vals;
    vals.n = n;
    for (int k = 0; k < n; ++k) vals.v[k] = values[k];
    const unsigned long long *d_conf = nullptr;
    const hipError_t e = launch_score(d, d + at_truth, B, H, W, vals, o.quantile_ppm, classes, d + at_ws,
                                      reinterpret_cast<mi_unet_score *>(d + at_scores), &d_conf, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("score launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p + at_scores, d + at_scores, P * sizeof(mi_unet_score), hipMemcpyDeviceToHost, s));
    if (classes) HIP_TRY(hipMemcpyAsync(p + at_ws, d_conf, conf_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                           // the call's only host synchronisation
    memcpy(scores, p + at_scores, P * sizeof(mi_unet_score));
    if (classes) {
        const size_t m = (size_t)B * classes * classes * sizeof(int64_t);
        memcpy(confusion, p + at_ws, m);
        memcpy(skipped, p + at_ws + m, (size_t)B * sizeof(int64_t));
    }
    return MI_UNET_OK;
}
#endif

}  // extern "C"
