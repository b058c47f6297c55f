// volume_match.cpp -- the components of a prediction against the components of a truth (include/mi_unet.h: mi_unet_volume_match;
// DESIGN.md 7.14): the argument checks, the definition as sequential host arithmetic (mi_unet_volume_match_host), the one-to-one
// assignment at an IoU threshold (mi_unet_volume_match_assign), the scores of an assignment (mi_unet_volume_match_derive) and the entry
// point on the handle, which owns the stage's workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h;
// tests/cpu/volume_match_host_test.cpp).
#include <algorithm>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vmatch_side) == 20, "mi_unet_vmatch_side is five int32 without padding");
static_assert(sizeof(mi_unet_vmatch_pair) == 12, "mi_unet_vmatch_pair is three int32 without padding");

namespace miunet {

namespace {

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_match_args(const char *fn, const int32_t *pred, const int32_t *truth, int D, int H, int W, int mp, int mt, int cap,
                     const mi_unet_vmatch_side *ps, const mi_unet_vmatch_side *ts, const mi_unet_vmatch_pair *pairs, const int *found)
{
    const std::string f = fn;
    if (!pred || !truth || !ps || !ts || !pairs || !found) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_min1(f, D, H, W)) return rc;
    // (each factor is below 2^31, so the products are tested one at a time)
    if ((int64_t)D * H >= ((int64_t)1 << 31) || (int64_t)D * H * W >= ((int64_t)1 << 31))
        return fail(MI_UNET_EARG, f + ": D * H * W must stay below 2^31");
    if (mp < 1 || mp > MI_UNET_VOLUME_MAX_TABLE || mt < 1 || mt > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(mp) + " and " + std::to_string(mt) + " components (1 .. " +
                                      std::to_string(MI_UNET_VOLUME_MAX_TABLE) + " a side)");
    if (cap < 1) return fail(MI_UNET_EARG, f + ": cap " + std::to_string(cap) + " (at least 1)");
    return MI_UNET_OK;
}

// the checks assign and derive share
int check_tables(const std::string &f, const mi_unet_vmatch_side *ps, int mp, const mi_unet_vmatch_side *ts, int mt,
                 const mi_unet_vmatch_pair *pairs, int found, int cap)
{
    if (!ps || !ts || !pairs) return fail(MI_UNET_EARG, f + ": null argument");
    if (mp < 1 || mp > MI_UNET_VOLUME_MAX_TABLE || mt < 1 || mt > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(mp) + " and " + std::to_string(mt) + " components (1 .. " +
                                      std::to_string(MI_UNET_VOLUME_MAX_TABLE) + " a side)");
    if (cap < 1) return fail(MI_UNET_EARG, f + ": cap " + std::to_string(cap) + " (at least 1)");
    if (found < 0) return fail(MI_UNET_EARG, f + ": found " + std::to_string(found) + " (at least 0)");
    if (found > cap)
        return fail(MI_UNET_EARG, f + ": the pair list is truncated (found " + std::to_string(found) + " > cap " + std::to_string(cap) + ")");
    for (int i = 0; i < found; ++i)
        if (pairs[i].p < 0 || pairs[i].p >= mp || pairs[i].t < 0 || pairs[i].t >= mt)
            return fail(MI_UNET_EARG, f + ": pair " + std::to_string(i) + " names a component outside the tables");
    return MI_UNET_OK;
}

inline int cls(int32_t id, int m) { return id >= 1 && id <= m ? id : 0; }

// i / u of a pair as two integers; u = vp + vt - i < 2^32
struct Cand { int64_t i, u; int32_t p, t; };

inline Cand cand_of(const mi_unet_vmatch_pair &q, const mi_unet_vmatch_side *ps, const mi_unet_vmatch_side *ts)
{
    return Cand{ q.voxels, (int64_t)ps[q.p].voxels + ts[q.t].voxels - q.voxels, q.p, q.t };
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_match_host(const int32_t *pred_ids, const int32_t *truth_ids, int D, int H, int W, int mp, int mt, int cap,
                              mi_unet_vmatch_side *pred_side, mi_unet_vmatch_side *truth_side, mi_unet_vmatch_pair *pairs, int *found)
{
    if (int rc = check_match_args("mi_unet_volume_match_host", pred_ids, truth_ids, D, H, W, mp, mt, cap, pred_side, truth_side, pairs, found))
        return rc;
    const size_t dhw = (size_t)D * H * W, cols = (size_t)mt + 1;
    std::vector<int32_t> N(((size_t)mp + 1) * cols, 0);
    for (size_t i = 0; i < dhw; ++i) {
        const size_t key = (size_t)cls(pred_ids[i], mp) * cols + (size_t)cls(truth_ids[i], mt);
        if (key) ++N[key];
    }
    auto side = [&](int n_other, auto cell) {                  // cell(b) = the count against class b of the other side
        mi_unet_vmatch_side s{ 0, 0, 0, 0, 0 };
        for (int b = 0; b <= n_other; ++b) {
            const int32_t v = cell(b);
            s.voxels += v;
            if (b >= 1 && v > 0) {
                s.covered += v;
                ++s.partners;
                if (v > s.best_voxels) { s.best_voxels = v; s.best = b; }      // (ascending b: a tie keeps the smaller index)
            }
        }
        return s;
    };
    for (int r = 0; r < mp; ++r) pred_side[r] = side(mt, [&](int b) { return N[(size_t)(r + 1) * cols + b]; });
    for (int c = 0; c < mt; ++c) truth_side[c] = side(mp, [&](int a) { return N[(size_t)a * cols + (c + 1)]; });
    int64_t n = 0;
    for (int a = 1; a <= mp; ++a)
        for (int b = 1; b <= mt; ++b) {
            const int32_t v = N[(size_t)a * cols + b];
            if (v <= 0) continue;
            if (n < cap) pairs[n] = mi_unet_vmatch_pair{ a - 1, b - 1, v };
            ++n;                                                // (n <= D * H * W < 2^31)
        }
    if (n < cap) std::memset(pairs + n, 0, (size_t)(cap - n) * sizeof(mi_unet_vmatch_pair));
    *found = (int)n;
    return MI_UNET_OK;
}

int mi_unet_volume_match_assign(const mi_unet_vmatch_side *pred_side, int mp, const mi_unet_vmatch_side *truth_side, int mt,
                                const mi_unet_vmatch_pair *pairs, int found, int cap, int iou_num, int iou_den, int32_t *match_of_pred,
                                int32_t *match_of_truth, mi_unet_vmatch_counts *counts)
{
    const std::string f = "mi_unet_volume_match_assign";
    if (!match_of_pred || !match_of_truth || !counts) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_tables(f, pred_side, mp, truth_side, mt, pairs, found, cap)) return rc;
    if (iou_num < 1 || iou_den > 65536 || iou_num > iou_den)
        return fail(MI_UNET_EARG, f + ": threshold " + std::to_string(iou_num) + " / " + std::to_string(iou_den) + " (1 <= num <= den <= 65536)");
    std::vector<Cand> cands;
    for (int k = 0; k < found; ++k) {
        const Cand c = cand_of(pairs[k], pred_side, truth_side);
        if (c.i > 0 && c.u > 0 && c.i * iou_den >= (int64_t)iou_num * c.u) cands.push_back(c);    // (i < 2^31, u < 2^32, den <= 2^16)
    }
    std::sort(cands.begin(), cands.end(), [](const Cand &x, const Cand &y) {
        const int64_t l = x.i * y.u, r = y.i * x.u;             // x.i / x.u > y.i / y.u; both products below 2^63
        if (l != r) return l > r;
        if (x.p != y.p) return x.p < y.p;
        return x.t < y.t;
    });
    std::vector<int32_t> of_p((size_t)mp, 0), of_t((size_t)mt, 0);
    int tp = 0;
    for (const Cand &c : cands) {
        if (of_p[c.p] || of_t[c.t]) continue;
        of_p[c.p] = c.t + 1;
        of_t[c.t] = c.p + 1;
        ++tp;
    }
    int present_p = 0, present_t = 0;
    for (int r = 0; r < mp; ++r) present_p += pred_side[r].voxels > 0;
    for (int c = 0; c < mt; ++c) present_t += truth_side[c].voxels > 0;
    std::memcpy(match_of_pred, of_p.data(), of_p.size() * sizeof(int32_t));
    std::memcpy(match_of_truth, of_t.data(), of_t.size() * sizeof(int32_t));
    *counts = mi_unet_vmatch_counts{ tp, present_p - tp, present_t - tp };
    return MI_UNET_OK;
}

int mi_unet_volume_match_derive(const mi_unet_vmatch_side *pred_side, int mp, const mi_unet_vmatch_side *truth_side, int mt,
                                const mi_unet_vmatch_pair *pairs, int found, int cap, const int32_t *match_of_pred, mi_unet_vmatch_scores *out)
{
    const std::string f = "mi_unet_volume_match_derive";
    if (!match_of_pred || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_tables(f, pred_side, mp, truth_side, mt, pairs, found, cap)) return rc;
    int tp = 0, present_p = 0, present_t = 0;
    double sum_iou = 0.0, sum_dice = 0.0;
    for (int r = 0; r < mp; ++r) {
        present_p += pred_side[r].voxels > 0;
        const int32_t t1 = match_of_pred[r];
        if (t1 == 0) continue;
        if (t1 < 0 || t1 > mt) return fail(MI_UNET_EARG, f + ": match_of_pred[" + std::to_string(r) + "] = " + std::to_string(t1));
        // the pair list is ordered by (p, t)
        const mi_unet_vmatch_pair want{ r, t1 - 1, 0 };
        const mi_unet_vmatch_pair *q = std::lower_bound(pairs, pairs + found, want, [](const mi_unet_vmatch_pair &x, const mi_unet_vmatch_pair &y) {
            return x.p != y.p ? x.p < y.p : x.t < y.t;
        });
        if (q == pairs + found || q->p != want.p || q->t != want.t || q->voxels < 1)
            return fail(MI_UNET_EARG, f + ": match (" + std::to_string(r) + ", " + std::to_string(t1 - 1) + ") is not in the pair list");
        const Cand c = cand_of(*q, pred_side, truth_side);
        sum_iou += (double)c.i / (double)c.u;
        sum_dice += 2.0 * (double)c.i / (double)(c.u + c.i);
        ++tp;
    }
    for (int c = 0; c < mt; ++c) present_t += truth_side[c].voxels > 0;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double T = tp, FP = present_p - tp, FN = present_t - tp;
    mi_unet_vmatch_scores o;
    o.precision = T + FP > 0.0 ? T / (T + FP) : nan;
    o.recall = T + FN > 0.0 ? T / (T + FN) : nan;
    o.f1 = 2.0 * T + FP + FN > 0.0 ? 2.0 * T / (2.0 * T + FP + FN) : nan;
    o.sq = tp ? sum_iou / T : nan;
    o.rq = T + FP / 2.0 + FN / 2.0 > 0.0 ? T / (T + FP / 2.0 + FN / 2.0) : nan;
    o.pq = o.sq * o.rq;
    o.mean_dice = tp ? sum_dice / T : nan;
    *out = o;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
// Pairs that travel back with the tables in the one copy before the call's synchronisation.  A real series has tens of pairs; a list
// that holds more is fetched in a second copy, once `found` says how long it is.
constexpr size_t kEagerPairs = 65536;

int mi_unet_volume_match(mi_unet_t *h, const int32_t *pred_ids, const int32_t *truth_ids, int D, int H, int W, int mp, int mt, int cap,
                         mi_unet_vmatch_side *pred_side, mi_unet_vmatch_side *truth_side, mi_unet_vmatch_pair *pairs, int *found)
{
    if (int rc = check_handle(h, false)) return rc;
    if (int rc = check_match_args("mi_unet_volume_match", pred_ids, truth_ids, D, H, W, mp, mt, cap, pred_side, truth_side, pairs, found))
        return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, MP = (size_t)mp, MT = (size_t)mt, cells = (MP + 1) * (MT + 1);
    // a pair holds at least one voxel and one cell, so this many positions can be filled at all
    const size_t keep = std::min({ (size_t)cap, dhw, MP * MT });
    // results, the same layout on the device and in pinned memory: pred side, truth side, found, pairs; then on the device the row
    // counts, the row offsets, the columns' accumulators, the table and both stacks; in pinned memory both stacks
    const size_t at_ts = up256(MP * sizeof(mi_unet_vmatch_side)), at_found = at_ts + up256(MT * sizeof(mi_unet_vmatch_side));
    const size_t at_pairs = at_found + 256, at_rest = at_pairs + up256(keep * sizeof(mi_unet_vmatch_pair));
    const size_t at_rows = at_rest, at_first = at_rows + up256(MP * sizeof(int32_t)), at_acc = at_first + up256(MP * sizeof(int32_t));
    const size_t at_table = at_acc + up256(MT * VMT_COL_ACC_BYTES);
    const size_t at_pred = at_table + up256(cells * sizeof(int32_t)), at_truth = at_pred + up256(dhw * sizeof(int32_t));
    const size_t dev_need = at_truth + up256(dhw * sizeof(int32_t));
    const size_t hat_pred = at_rest, hat_truth = hat_pred + up256(dhw * sizeof(int32_t)), host_need = hat_truth + up256(dhw * sizeof(int32_t));
    hipStream_t s = h->stream;
    if (int rc = h->ws_vmt.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vmt.d, *const p = h->ws_vmt.p;
    host_copy(h, p + hat_pred, pred_ids, dhw * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(d + at_pred, p + hat_pred, dhw * sizeof(int32_t), hipMemcpyHostToDevice, s));
    host_copy(h, p + hat_truth, truth_ids, dhw * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(d + at_truth, p + hat_truth, dhw * sizeof(int32_t), hipMemcpyHostToDevice, s));
    VolumeMatchArgs a;
    a.D = D; a.H = H; a.W = W; a.mp = mp; a.mt = mt;
    int32_t *const d_table = reinterpret_cast<int32_t *>(d + at_table);
    mi_unet_vmatch_pair *const d_pairs = reinterpret_cast<mi_unet_vmatch_pair *>(d + at_pairs);
    hipError_t e = launch_volume_match_count(reinterpret_cast<const int32_t *>(d + at_pred), reinterpret_cast<const int32_t *>(d + at_truth), a,
                                             d_table, s);
    if (e == hipSuccess)
        e = launch_volume_match_tables(d_table, a, reinterpret_cast<mi_unet_vmatch_side *>(d), reinterpret_cast<mi_unet_vmatch_side *>(d + at_ts),
                                       reinterpret_cast<int32_t *>(d + at_rows), reinterpret_cast<int32_t *>(d + at_first),
                                       reinterpret_cast<int32_t *>(d + at_found), d + at_acc, d_pairs, (int)keep, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume match launch: ") + hipGetErrorString(e));
    const size_t eager = std::min(keep, kEagerPairs);
    HIP_TRY(hipMemcpyAsync(p, d, at_pairs + eager * sizeof(mi_unet_vmatch_pair), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int n_found = *reinterpret_cast<const int32_t *>(p + at_found);
    const size_t n = std::min((size_t)std::max(n_found, 0), keep);
    if (n > eager) {
        HIP_TRY(hipMemcpyAsync(p + at_pairs + eager * sizeof(mi_unet_vmatch_pair), d_pairs + eager, (n - eager) * sizeof(mi_unet_vmatch_pair),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    std::memcpy(pred_side, p, MP * sizeof(mi_unet_vmatch_side));
    std::memcpy(truth_side, p + at_ts, MT * sizeof(mi_unet_vmatch_side));
    std::memcpy(pairs, p + at_pairs, n * sizeof(mi_unet_vmatch_pair));
    if (n < (size_t)cap) std::memset(pairs + n, 0, ((size_t)cap - n) * sizeof(mi_unet_vmatch_pair));
    *found = n_found;
    return MI_UNET_OK;
}
#endif

}  // extern "C"
