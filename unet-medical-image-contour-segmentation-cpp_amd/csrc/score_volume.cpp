// score_volume.cpp -- scores of a stack as one volume (include/mi_unet.h: mi_unet_score_volume): the argument checks,
// the definition as sequential host arithmetic (mi_unet_score_volume_host), the unit helper, the derived metrics in mm and the entry
// point on the handle, which shares mi_unet_score_labels' workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled
// (stage_common.h), together with score.cpp (tests/cpu/score_volume_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "stage_common.h"

namespace miunet {

namespace {

constexpr mi_unet_score_opts kDefaultOpts{ 50000, 0 };
constexpr int kMaxSide = MI_UNET_SCORE_VOLUME_MAX_SIDE;
constexpr int64_t kD2Limit = (int64_t)1 << 31;          // every d2 stays below it (d2_fits)
constexpr int64_t kNone = std::numeric_limits<int64_t>::max();

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_args(const char *fn, const uint8_t *pred, const uint8_t *truth, int D, int H, int W, const int *values, int n, const int *units,
               const mi_unet_score_opts &o, const mi_unet_score *scores, const int64_t *confusion, const int64_t *skipped)
{
    const std::string f = fn;
    if (!pred || !truth || !values || !units || !scores) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_max(f, D, H, W, kMaxSide)) return rc;
    if (int rc = check_values(f, values, n, MI_UNET_SCORE_MAX_VALUES)) return rc;
    if (o.quantile_ppm < 0 || o.quantile_ppm > 999999)
        return fail(MI_UNET_EARG, f + ": quantile_ppm " + std::to_string(o.quantile_ppm) + " is outside 0 .. 999999");
    if (o.classes < 0 || o.classes > MI_UNET_SCORE_MAX_CLASSES)
        return fail(MI_UNET_EARG, f + ": classes " + std::to_string(o.classes) + " is outside 0 .. " + std::to_string(MI_UNET_SCORE_MAX_CLASSES));
    if (confusion && o.classes == 0) return fail(MI_UNET_EARG, f + ": a confusion matrix needs classes >= 1");
    if (confusion && !skipped) return fail(MI_UNET_EARG, f + ": a confusion matrix needs the skipped count beside it");
    if ((int64_t)n * D * H * W >= kD2Limit) return fail(MI_UNET_EARG, f + ": n * D * H * W must stay below 2^31");      // (< 2^42: no overflow)
    if (int rc = check_units_min1(f, units)) return rc;
    if (!d2_fits(D, H, W, units)) return fail(MI_UNET_EARG, f + ": the squared diagonal of the volume in spacing units must stay below 2^31");
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

// One set of one plane: its boundary voxels and, per voxel, the squared distance along z (in units) to the nearest boundary voxel of
// its (y, x) column, kNone for a column without one.
struct SetField {
    std::vector<uint8_t> bnd;
    std::vector<int64_t> gz2;
    int32_t count = 0;
};

void boundary_columns(const uint8_t *map, int D, int H, int W, int v, int64_t uz, SetField &s)
{
    const size_t hw = (size_t)H * W, dhw = hw * D;
    s.bnd.assign(dhw, 0);
    s.gz2.assign(dhw, kNone);
    s.count = 0;
    auto in = [&](int z, int y, int x) { return z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W && map[(size_t)z * hw + (size_t)y * W + x] == v; };
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (in(z, y, x) && !(in(z - 1, y, x) && in(z + 1, y, x) && in(z, y - 1, x) && in(z, y + 1, x) && in(z, y, x - 1) && in(z, y, x + 1))) {
                    s.bnd[(size_t)z * hw + (size_t)y * W + x] = 1;
                    ++s.count;
                }
    for (size_t c = 0; c < hw; ++c) {
        int64_t d = -1;                                         // index distance to the last boundary voxel seen, -1: none yet
        for (int z = 0; z < D; ++z) {
            d = s.bnd[(size_t)z * hw + c] ? 0 : d < 0 ? -1 : d + 1;
            if (d >= 0) s.gz2[(size_t)z * hw + c] = d * uz * d * uz;
        }
        d = -1;
        for (int z = D - 1; z >= 0; --z) {
            d = s.bnd[(size_t)z * hw + c] ? 0 : d < 0 ? -1 : d + 1;
            if (d >= 0) s.gz2[(size_t)z * hw + c] = std::min(s.gz2[(size_t)z * hw + c], d * uz * d * uz);
        }
    }
}

// d2 of every boundary voxel of src to the boundary of dst (not empty), in raster order: per row (z, y) that holds source voxels, the
// row of f = min over y' of gz2(z, y', x) + ((y - y') uy)^2, then per source voxel the minimum over x' of ((x - x') ux)^2 + f(x')
void directed_d2(const SetField &src, const SetField &dst, int D, int H, int W, int64_t ux, int64_t uy, std::vector<int32_t> &out)
{
    const size_t hw = (size_t)H * W;
    std::vector<int64_t> f((size_t)W);
    out.clear();
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y) {
            const uint8_t *const b = src.bnd.data() + (size_t)z * hw + (size_t)y * W;
            if (!std::any_of(b, b + W, [](uint8_t v) { return v != 0; })) continue;
            for (int x = 0; x < W; ++x) {
                int64_t best = kNone;
                for (int yy = 0; yy < H; ++yy) {
                    const int64_t g = dst.gz2[(size_t)z * hw + (size_t)yy * W + x];
                    if (g != kNone) best = std::min(best, g + (int64_t)(y - yy) * uy * (y - yy) * uy);
                }
                f[x] = best;
            }
            for (int x = 0; x < W; ++x) {
                if (!b[x]) continue;
                int64_t best = kNone;
                for (int xx = 0; xx < W; ++xx)
                    if (f[xx] != kNone) best = std::min(best, f[xx] + (int64_t)(x - xx) * ux * (x - xx) * ux);
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

int mi_unet_score_volume_host(const uint8_t *pred, const uint8_t *truth, int D, int H, int W, const int *values, int n,
                              const int spacing_units[3], const mi_unet_score_opts *opts, mi_unet_score *scores, int64_t *confusion,
                              int64_t *skipped)
{
    const mi_unet_score_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_args("mi_unet_score_volume_host", pred, truth, D, H, W, values, n, spacing_units, o, scores, confusion, skipped)) return rc;
    const size_t dhw = (size_t)D * H * W;
    const int64_t ux = spacing_units[0], uy = spacing_units[1], uz = spacing_units[2];
    SetField fa, ft;
    std::vector<int32_t> d_a, d_t;
    for (int k = 0; k < n; ++k) {
        const int v = values[k];
        mi_unet_score s{};
        for (size_t i = 0; i < dhw; ++i) {
            const bool a = pred[i] == v, t = truth[i] == v;
            s.tp += a && t; s.fp += a && !t; s.fn += t && !a;
        }
        s.value = v;
        s.quantile_ppm = o.quantile_ppm;
        boundary_columns(pred, D, H, W, v, uz, fa);
        boundary_columns(truth, D, H, W, v, uz, ft);
        const bool have = fa.count > 0 && ft.count > 0;
        d_a.clear(); d_t.clear();
        if (have) {
            directed_d2(fa, ft, D, H, W, ux, uy, d_a);
            directed_d2(ft, fa, D, H, W, ux, uy, d_t);
        }
        s.a_to_t = direction(d_a, fa.count, have, o.quantile_ppm);
        s.t_to_a = direction(d_t, ft.count, have, o.quantile_ppm);
        s.q_d2_sym = -1;
        if (have) {
            d_a.insert(d_a.end(), d_t.begin(), d_t.end());
            s.q_d2_sym = order_stat(d_a, o.quantile_ppm);
        }
        scores[k] = s;
    }
    if (confusion) {
        const int c = o.classes;
        std::fill(confusion, confusion + (size_t)c * c, 0);
        int64_t skip = 0;
        for (size_t i = 0; i < dhw; ++i) {
            if (pred[i] < c && truth[i] < c) ++confusion[(size_t)truth[i] * c + pred[i]];
            else ++skip;
        }
        skipped[0] = skip;
    }
    return MI_UNET_OK;
}

int mi_unet_score_volume_units(const double spacing_mm[3], int D, int H, int W, int units[3], double *unit_mm)
{
    if (!spacing_mm || !units || !unit_mm) return fail(MI_UNET_EARG, "mi_unet_score_volume_units: null argument");
    if (!sides_within(D, H, W, kMaxSide)) return fail(MI_UNET_EARG, "mi_unet_score_volume_units: D, H, W must be in 1 .. " + std::to_string(kMaxSide));
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing_mm[a]) || !(spacing_mm[a] > 0.0))
            return fail(MI_UNET_EARG, "mi_unet_score_volume_units: the spacing must be finite and positive");
    static const double kUnit[5] = { 1.0, 0.1, 0.01, 0.001, 0.0001 };
    for (int k = 4; k >= 0; --k) {
        int64_t u[3];
        bool ok = true;
        for (int a = 0; a < 3; ++a) {
            const double q = spacing_mm[a] / kUnit[k];
            if (!(q < 2147483647.0)) { ok = false; break; }     // (llround of it must fit an int)
            u[a] = std::llround(q);
            ok = ok && u[a] >= 1;
        }
        if (!ok || !d2_fits(D, H, W, u)) continue;
        for (int a = 0; a < 3; ++a) units[a] = (int)u[a];
        *unit_mm = kUnit[k];
        return MI_UNET_OK;
    }
    return fail(MI_UNET_EARG, "mi_unet_score_volume_units: no unit of 1 .. 0.0001 mm keeps the volume's squared diagonal below 2^31 with every unit >= 1");
}

int mi_unet_score_volume_derive(const mi_unet_score *s, double unit_mm, mi_unet_score_metrics *out)
{
    if (!s || !out) return fail(MI_UNET_EARG, "mi_unet_score_volume_derive: null argument");
    if (!std::isfinite(unit_mm) || !(unit_mm > 0.0)) return fail(MI_UNET_EARG, "mi_unet_score_volume_derive: unit_mm must be finite and positive");
    mi_unet_score_metrics m{};
    if (int rc = mi_unet_score_derive(s, &m)) return rc;
    m.hd *= unit_mm; m.hd_q *= unit_mm; m.assd *= unit_mm; m.rmsd *= unit_mm;
    *out = m;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_score_volume(mi_unet_t *h, const uint8_t *pred, const uint8_t *truth, int D, int H, int W, const int *values, int n,
                         const int spacing_units[3], const mi_unet_score_opts *opts, mi_unet_score *scores, int64_t *confusion, int64_t *skipped)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_score_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_args("mi_unet_score_volume", pred, truth, D, H, W, values, n, spacing_units, o, scores, confusion, skipped)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int classes = confusion ? o.classes : 0;
    const size_t map_bytes = (size_t)D * H * W;
    // device: both volumes, the scores, the kernels' workspace; pinned: both volumes, the scores, the matrix with its skipped count
    const size_t at_truth = up256(map_bytes), at_scores = at_truth + up256(map_bytes), at_ws = at_scores + up256((size_t)n * sizeof(mi_unet_score));
    const size_t conf_bytes = ((size_t)classes * classes + 1) * sizeof(int64_t);
    const size_t dev_need = at_ws + score_volume_workspace_bytes(D, H, W, n, classes), host_need = at_ws + conf_bytes;
    hipStream_t s = h->stream;
    if (int rc = h->ws_score.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_score.d, *const p = h->ws_score.p;
    host_copy(h, p, pred, map_bytes);
    host_copy(h, p + at_truth, truth, map_bytes);
    HIP_TRY(hipMemcpyAsync(d, p, map_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + at_truth, p + at_truth, map_bytes, hipMemcpyHostToDevice, s));
    ScoreVolumeArgs a;
    a.D = D; a.H = H; a.W = W; a.ux = spacing_units[0]; a.uy = spacing_units[1]; a.uz = spacing_units[2];
    a.quantile_ppm = o.quantile_ppm; a.classes = classes;
    a.vals.n = n;
    for (int k = 0; k < n; ++k) a.vals.v[k] = values[k];
    const unsigned long long *d_conf = nullptr;
    const hipError_t e = launch_score_volume(d, d + at_truth, a, d + at_ws, reinterpret_cast<mi_unet_score *>(d + at_scores), &d_conf, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("score volume launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p + at_scores, d + at_scores, (size_t)n * sizeof(mi_unet_score), hipMemcpyDeviceToHost, s));
    if (classes) HIP_TRY(hipMemcpyAsync(p + at_ws, d_conf, conf_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                           // the call's only host synchronisation
    memcpy(scores, p + at_scores, (size_t)n * sizeof(mi_unet_score));
    if (classes) {
        const size_t m = (size_t)classes * classes * sizeof(int64_t);
        memcpy(confusion, p + at_ws, m);
        memcpy(skipped, p + at_ws + m, sizeof(int64_t));
    }
    return MI_UNET_OK;
}
#endif

}  // extern "C"
