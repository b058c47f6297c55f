// volume_spatial.cpp -- per component of a labelled stack where its intensity sits: the intensity-weighted sums, the intensity peaks
// and the inverse-distance pair sums behind Moran's I and Geary's C (include/mi_unet.h: mi_unet_volume_spatial): the
// argument checks, the rows of the ball, the definition as sequential host arithmetic (mi_unet_volume_spatial_host), the function that
// turns an entry into millimetres and the two statistics (mi_unet_volume_spatial_derive) and the entry point on the handle, which owns
// the stage's workspace and splits the pair sums into launches of bounded work.  With MIUNET_NO_DEVICE only the host arithmetic is
// compiled (stage_common.h; tests/cpu/volume_spatial_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vspatial) == 168, "mi_unet_vspatial is 168 bytes without padding");
static_assert(sizeof(mi_unet_vspatial_opts) == 8, "mi_unet_vspatial_opts is two ints");
static_assert(sizeof(mi_unet_vspatial_metrics) == 12 * sizeof(double), "mi_unet_vspatial_metrics is 12 doubles");

namespace miunet {

namespace {

constexpr mi_unet_vspatial_opts kDefaultOpts{ 131072, 0 };
constexpr int kMaxSide = MI_UNET_SCORE_VOLUME_MAX_SIDE;
constexpr int kMaxR = MI_UNET_VOLUME_CLEAN_MAX_R;

struct BallRow { int dy, dz, hx, pad; };    // a row of B(r): its offsets and its x half-width

// the rows of B(r) in the order (dz, dy) ascending: hx = floor(sqrt(r^2 - (dy uy)^2 - (dz uz)^2) / ux), the largest dx of
// mi_unet_volume_ball's definition -> the ball's voxels
int64_t ball_rows(const int *units, int r, std::vector<BallRow> &rows)
{
    const int64_t r2 = (int64_t)r * r;
    const int ey = r / units[1], ez = r / units[2];
    int64_t voxels = 0;
    for (int dz = -ez; dz <= ez; ++dz)
        for (int dy = -ey; dy <= ey; ++dy) {
            const int64_t ty = (int64_t)dy * units[1], tz = (int64_t)dz * units[2], rem = r2 - ty * ty - tz * tz;
            if (rem < 0) continue;
            int64_t root = (int64_t)std::sqrt((double)rem);
            while (root * root > rem) --root;
            while ((root + 1) * (root + 1) <= rem) ++root;
            const int hx = (int)(root / units[0]);
            rows.push_back(BallRow{ dy, dz, hx, 0 });
            voxels += 2 * (int64_t)hx + 1;
        }
    return voxels;
}

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_spatial_args(const char *fn, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const int *units,
                       const mi_unet_vspatial_opts &o, const mi_unet_vspatial *table)
{
    const std::string f = fn;
    if (!ids || !intensity || !units || !table) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_max(f, D, H, W, kMaxSide)) return rc;
    if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return fail(MI_UNET_EARG, f + ": D * H * W must stay below 2^31");    // (< 2^39: no overflow)
    if (m < 1 || m > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components (1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE) + ")");
    if (int rc = check_units_min1(f, units)) return rc;
    if (!d2_fits(D, H, W, units)) return fail(MI_UNET_EARG, f + ": the squared diagonal of the volume in spacing units must stay below 2^31");
    if (o.max_voxels < 0 || o.max_voxels > MI_UNET_VSPATIAL_MAX_VOXELS_LIMIT)
        return fail(MI_UNET_EARG, f + ": max_voxels " + std::to_string(o.max_voxels) + " is outside 0 .. " +
                                      std::to_string(MI_UNET_VSPATIAL_MAX_VOXELS_LIMIT));
    if (o.peak_r < 0 || o.peak_r > kMaxR) return fail(MI_UNET_EARG, f + ": peak_r " + std::to_string(o.peak_r) + " is outside 0 .. " + std::to_string(kMaxR));
    const int64_t nrows = (2 * (int64_t)(o.peak_r / units[1]) + 1) * (2 * (int64_t)(o.peak_r / units[2]) + 1);
    if (nrows > MI_UNET_VSPATIAL_MAX_BALL_ROWS)
        return fail(MI_UNET_EARG, f + ": the ball of peak_r " + std::to_string(o.peak_r) + " has " + std::to_string(nrows) + " rows (at most " +
                                      std::to_string(MI_UNET_VSPATIAL_MAX_BALL_ROWS) + ")");
    std::vector<BallRow> rows;
    const int64_t voxels = ball_rows(units, o.peak_r, rows);
    if (voxels > MI_UNET_VSPATIAL_MAX_BALL_VOXELS)
        return fail(MI_UNET_EARG, f + ": the ball of peak_r " + std::to_string(o.peak_r) + " has " + std::to_string(voxels) + " voxels (at most " +
                                      std::to_string(MI_UNET_VSPATIAL_MAX_BALL_VOXELS) + ")");
    return MI_UNET_OK;
}

inline bool searched(int32_t voxels, int max_voxels) { return voxels >= 2 && voxels <= max_voxels; }

// what the host derives from a component's sums before anything else runs: the centre, and who is searched
inline void set_centre_and_pairs(mi_unet_vspatial &t, int max_voxels)
{
    if (!t.voxels) return;
    const int64_t A = t.voxels;
    t.centre = (int32_t)((2 * t.si + A) / (2 * A));
    t.searched = searched(t.voxels, max_voxels);
    t.pairs = t.searched ? A * (A - 1) / 2 : 0;
}

struct Point { int32_t x, y, z, v; };       // pre-scaled coordinates and the voxel's intensity less the component's centre

#ifndef MIUNET_NO_DEVICE
// The pairs one launch of the pair sums may hold.  k_vsp_pairs runs at 2e11 pairs / s on an MI355X (DESIGN.md 7.20 has the measured
// rate), so a launch of 2^28 pairs takes about 1.3 ms, hundreds of times the cost of launching it: a component at the default cap of
// 2^17 voxels (8.6e9 pairs) becomes 32 launches, one at the limit of 2^20 (5.5e11 pairs) 2048, and none of them can occupy the device
// for long.  The ranking compares A^2 indices per component, a few integer operations each, under the same bound times 16.
constexpr int64_t kPairsPerLaunch = (int64_t)1 << 28;
constexpr int64_t kComparesPerLaunch = (int64_t)1 << 32;
constexpr int kTilesPerItem = 32;                               // b-tiles a workgroup takes: 2 M pairs

// the work list [i0, ...) in launches of bounded work: a launch ends once the next item would pass the bound
template <class Launch>
hipError_t bounded_launches(const std::vector<int64_t> &work, int64_t bound, Launch launch)
{
    hipError_t e = hipSuccess;
    for (size_t i0 = 0; e == hipSuccess && i0 < work.size();) {
        size_t i1 = i0;
        for (int64_t sum = 0; i1 < work.size() && (i1 == i0 || sum + work[i1] <= bound); ++i1) sum += work[i1];
        e = launch(i0, (int)(i1 - i0));
        i0 = i1;
    }
    return e;
}
#endif

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_spatial_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const int spacing_units[3],
                                const mi_unet_vspatial_opts *opts, mi_unet_vspatial *table)
{
    const mi_unet_vspatial_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_spatial_args("mi_unet_volume_spatial_host", ids, intensity, D, H, W, m, spacing_units, o, table)) return rc;
    std::vector<mi_unet_vspatial> t((size_t)m);
    std::memset(t.data(), 0, t.size() * sizeof(mi_unet_vspatial));
    auto member = [&](int32_t id) { return id >= 1 && id <= m; };
    const int32_t *p = ids;
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x, ++p) {
                if (!member(*p)) continue;
                mi_unet_vspatial &c = t[*p - 1];
                const int32_t iv = intensity[p - ids];
                c.imin = c.voxels ? std::min(c.imin, iv) : iv;
                c.imax = c.voxels ? std::max(c.imax, iv) : iv;
                ++c.voxels;
                c.sx += x; c.sy += y; c.sz += z;
                c.si += iv; c.sii += (int64_t)iv * iv;
                c.six += (int64_t)iv * x; c.siy += (int64_t)iv * y; c.siz += (int64_t)iv * z;
            }
    for (int r = 0; r < m; ++r) set_centre_and_pairs(t[r], o.max_voxels);
    // the peaks: the row prefix sums, then every voxel of a component in index order; a later voxel wins only with a larger mean
    std::vector<BallRow> rows;
    ball_rows(spacing_units, o.peak_r, rows);
    const size_t stride = (size_t)W + 1;
    std::vector<uint32_t> prefix((size_t)D * H * stride);
    for (size_t row = 0; row < (size_t)D * H; ++row) {
        uint32_t run = 0;
        prefix[row * stride] = 0;
        for (int x = 0; x < W; ++x) prefix[row * stride + x + 1] = run += intensity[row * W + x];
    }
    p = ids;
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x, ++p) {
                if (!member(*p)) continue;
                mi_unet_vspatial &c = t[*p - 1];
                uint64_t s = 0, n = 0;
                for (const BallRow &b : rows) {
                    const int yy = y + b.dy, zz = z + b.dz;
                    if (yy < 0 || yy >= H || zz < 0 || zz >= D) continue;
                    const int lo = std::max(x - b.hx, 0), hi = std::min(x + b.hx, W - 1);
                    const uint32_t *const q = prefix.data() + ((size_t)zz * H + yy) * stride;
                    s += q[hi + 1] - q[lo];
                    n += (uint64_t)(hi - lo + 1);
                }
                const int32_t at = (int32_t)(p - ids);
                if (!c.gp_n || s * (uint64_t)c.gp_n > (uint64_t)c.gp_sum * n) { c.gp_sum = (int64_t)s; c.gp_n = (int64_t)n; c.gp_at = at; }
                if (intensity[at] == c.imax && (!c.lp_n || s * (uint64_t)c.lp_n > (uint64_t)c.lp_sum * n)) {
                    c.lp_sum = (int64_t)s; c.lp_n = (int64_t)n; c.lp_at = at;
                }
            }
    // the points of the searched components, a segment each, in index order; then the pairs i < j, i ascending, then j
    std::vector<size_t> first((size_t)m + 1, 0);
    for (int r = 0; r < m; ++r) first[r + 1] = first[r] + (t[r].searched ? (size_t)t[r].voxels : 0);
    std::vector<Point> pts(first[m]);
    std::vector<size_t> at(first.begin(), first.end() - 1);
    p = ids;
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x, ++p)
                if (member(*p) && t[*p - 1].searched)
                    pts[at[*p - 1]++] = Point{ x * spacing_units[0], y * spacing_units[1], z * spacing_units[2],
                                               (int32_t)intensity[p - ids] - t[*p - 1].centre };
    for (int r = 0; r < m; ++r) {
        if (!t[r].searched) continue;
        const Point *const e = pts.data() + first[r];
        const int n = t[r].voxels;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j) {
                const int32_t dx = e[i].x - e[j].x, dy = e[i].y - e[j].y, dz = e[i].z - e[j].z;
                const double w = 1.0 / std::sqrt((double)(dx * dx + dy * dy + dz * dz));
                const int64_t yi = e[i].v, yj = e[j].v;
                s0 += w;
                s1 += w * (double)(yi + yj);
                s2 += w * (double)(yi * yj);
                s3 += w * (double)((yi - yj) * (yi - yj));
            }
        t[r].s0 = s0; t[r].s1 = s1; t[r].s2 = s2; t[r].s3 = s3;
    }
    std::memcpy(table, t.data(), t.size() * sizeof(mi_unet_vspatial));
    return MI_UNET_OK;
}

int mi_unet_volume_spatial_derive(const mi_unet_vspatial *c, const int spacing_units[3], double unit_mm, mi_unet_vspatial_metrics *out)
{
    const std::string f = "mi_unet_volume_spatial_derive";
    if (!c || !spacing_units || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (c->voxels < 1) return fail(MI_UNET_EARG, f + ": voxels " + std::to_string(c->voxels) + " (a component has at least one voxel)");
    if (int rc = check_units_min1(f, spacing_units)) return rc;
    if (!std::isfinite(unit_mm) || !(unit_mm > 0.0)) return fail(MI_UNET_EARG, f + ": unit_mm must be finite and > 0");
    const double s[3] = { spacing_units[0] * unit_mm, spacing_units[1] * unit_mm, spacing_units[2] * unit_mm };
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double Ad = (double)c->voxels;
    mi_unet_vspatial_metrics o;
    o.cx_mm = ((double)c->sx / Ad + 0.5) * s[0];
    o.cy_mm = ((double)c->sy / Ad + 0.5) * s[1];
    o.cz_mm = ((double)c->sz / Ad + 0.5) * s[2];
    const double sid = (double)c->si;
    o.icx_mm = c->si ? ((double)c->six / sid + 0.5) * s[0] : nan;
    o.icy_mm = c->si ? ((double)c->siy / sid + 0.5) * s[1] : nan;
    o.icz_mm = c->si ? ((double)c->siz / sid + 0.5) * s[2] : nan;
    const double ddx = o.icx_mm - o.cx_mm, ddy = o.icy_mm - o.cy_mm, ddz = o.icz_mm - o.cz_mm;
    o.com_shift_mm = std::sqrt(ddx * ddx + ddy * ddy + ddz * ddz);
    o.integrated_intensity = sid * (s[0] * s[1] * s[2]);
    o.local_peak = c->lp_n ? (double)c->lp_sum / (double)c->lp_n : nan;
    o.global_peak = c->gp_n ? (double)c->gp_sum / (double)c->gp_n : nan;
    // V = sum (v - mean)^2 from an exact 128-bit numerator, converted once: A * sii < 2^83, si^2 < 2^94
    const __int128 A = c->voxels;
    const double V = (double)(A * c->sii - (__int128)c->si * c->si) / Ad;
    const double delta = (double)(c->si - (int64_t)c->centre * c->voxels) / Ad;                // (the numerator is exact: |.| <= A / 2)
    if (!c->searched || V == 0.0) {
        o.morans_i = o.gearys_c = nan;
    } else {
        o.morans_i = Ad / (2.0 * c->s0) * (2.0 * (c->s2 - delta * c->s1 + delta * delta * c->s0)) / V;
        o.gearys_c = (Ad - 1.0) / (2.0 * (2.0 * c->s0)) * (2.0 * c->s3) / V;
    }
    *out = o;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_spatial(mi_unet_t *h, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const int spacing_units[3],
                           const mi_unet_vspatial_opts *opts, mi_unet_vspatial *table)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vspatial_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_spatial_args("mi_unet_volume_spatial", ids, intensity, D, H, W, m, spacing_units, o, table)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, M = (size_t)m;
    std::vector<BallRow> rows;
    ball_rows(spacing_units, o.peak_r, rows);
    // device and pinned alike: ids, intensity, table, seg, peaks, rows | device only: cursor, prefix
    Layout lay;
    lay.take(dhw * sizeof(int32_t));                            // (the ids come first, at 0)
    const size_t at_int = lay.take(dhw * sizeof(uint16_t));
    const size_t at_table = lay.take(M * sizeof(mi_unet_vspatial)), at_seg = lay.take(M * sizeof(int4));
    const size_t at_peaks = lay.take(M * 6 * sizeof(long long)), at_rows = lay.take(rows.size() * sizeof(BallRow));
    const size_t host_need = lay.end;
    const size_t at_cursor = lay.take(M * sizeof(int)), at_prefix = lay.take((size_t)D * H * ((size_t)W + 1) * sizeof(uint32_t));
    hipStream_t s = h->stream;
    if (int rc = h->ws_vsp.reserve(lay.end, host_need, s)) return rc;
    uint8_t *const d = h->ws_vsp.d, *const p = h->ws_vsp.p;
    host_copy(h, p, ids, dhw * sizeof(int32_t));
    host_copy(h, p + at_int, intensity, dhw * sizeof(uint16_t));
    std::memcpy(p + at_rows, rows.data(), rows.size() * sizeof(BallRow));
    HIP_TRY(hipMemcpyAsync(d, p, dhw * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + at_int, p + at_int, dhw * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d + at_rows, p + at_rows, rows.size() * sizeof(BallRow), hipMemcpyHostToDevice, s));
    VolumeSpatialArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m; a.ux = spacing_units[0]; a.uy = spacing_units[1]; a.uz = spacing_units[2];
    const int32_t *const d_ids = reinterpret_cast<const int32_t *>(d);
    const uint16_t *const d_int = reinterpret_cast<const uint16_t *>(d + at_int);
    mi_unet_vspatial *const d_table = reinterpret_cast<mi_unet_vspatial *>(d + at_table);
    uint32_t *const d_prefix = reinterpret_cast<uint32_t *>(d + at_prefix);
    hipError_t e = launch_volume_spatial_sums(d_ids, d_int, a, d_table, s);
    if (e == hipSuccess) e = launch_volume_spatial_prefix(d_int, a, d_prefix, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume spatial launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p + at_table, d_table, M * sizeof(mi_unet_vspatial), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                           // the voxels size the segments and the work lists, si gives the centre
    mi_unet_vspatial *const t = reinterpret_cast<mi_unet_vspatial *>(p + at_table);
    int4 *const seg = reinterpret_cast<int4 *>(p + at_seg);
    size_t cands = 0, points = 0;
    std::vector<VspItem> items, rank_items;                     // the pair sums' upper triangle; the ranking's whole square
    std::vector<int64_t> item_pairs, rank_compares;
    for (int r = 0; r < m; ++r) {
        t[r].imin = t[r].voxels ? 65535 - t[r].imin : 0;
        set_centre_and_pairs(t[r], o.max_voxels);
        const int n = t[r].voxels;
        seg[r] = make_int4((int)cands, n, t[r].searched ? (int)points : -1, t[r].centre);      // (cands, points <= D * H * W < 2^31)
        cands += (size_t)n;
        if (!t[r].searched) continue;
        points += (size_t)n;
        const int tiles = (n + VSP_TILE - 1) / VSP_TILE;
        for (int ta = 0; ta < tiles; ++ta) {
            const int64_t na = std::min(VSP_TILE, n - ta * VSP_TILE);
            for (int tb = 0; tb < tiles; tb += kTilesPerItem) {
                const int nt = std::min(kTilesPerItem, tiles - tb);
                rank_items.push_back(VspItem{ r, ta, tb, nt });
                rank_compares.push_back(na * (std::min<int64_t>(n, (int64_t)(tb + nt) * VSP_TILE) - (int64_t)tb * VSP_TILE));
            }
            for (int tb = ta; tb < tiles; tb += kTilesPerItem) {
                const int nt = std::min(kTilesPerItem, tiles - tb);
                items.push_back(VspItem{ r, ta, tb, nt });
                item_pairs.push_back(na * (std::min<int64_t>(n, (int64_t)(tb + nt) * VSP_TILE) - (int64_t)tb * VSP_TILE));
            }
        }
    }
    if (cands) {
        // device: candidates, rank, points, both work lists, slots; pinned: both work lists, slots
        Layout big, pin;
        const size_t at_cand = big.take(cands * sizeof(VspCand)), at_rank = big.take(cands * sizeof(int));
        const size_t at_points = big.take(points * sizeof(int4));
        const size_t item_bytes = items.size() * sizeof(VspItem), rank_bytes = rank_items.size() * sizeof(VspItem);
        const size_t slot_bytes = items.size() * 4 * sizeof(double);
        const size_t at_items = big.take(item_bytes), at_ritems = big.take(rank_bytes), at_slots = big.take(slot_bytes);
        const size_t pin_items = pin.take(item_bytes), pin_ritems = pin.take(rank_bytes), pin_slots = pin.take(slot_bytes);
        if (int rc = h->ws_vsp_pts.reserve(big.end, pin.end, s)) return rc;                   // (nothing of the stage is in flight here)
        uint8_t *const dp = h->ws_vsp_pts.d, *const pp = h->ws_vsp_pts.p;
        const int4 *const d_seg = reinterpret_cast<const int4 *>(d + at_seg);
        VspCand *const d_cand = reinterpret_cast<VspCand *>(dp + at_cand);
        int *const d_rank = reinterpret_cast<int *>(dp + at_rank);
        int4 *const d_points = reinterpret_cast<int4 *>(dp + at_points);
        const VspItem *const d_items = reinterpret_cast<const VspItem *>(dp + at_items);
        const VspItem *const d_ritems = reinterpret_cast<const VspItem *>(dp + at_ritems);
        double *const d_slots = reinterpret_cast<double *>(dp + at_slots);
        long long *const d_peaks = reinterpret_cast<long long *>(d + at_peaks);
        HIP_TRY(hipMemcpyAsync(d + at_seg, p + at_seg, M * sizeof(int4), hipMemcpyHostToDevice, s));
        e = launch_volume_spatial_fill(d_ids, d_int, d_prefix, a, d_table, d_seg, reinterpret_cast<const int4 *>(d + at_rows), (int)rows.size(),
                                       reinterpret_cast<int *>(d + at_cursor), d_rank, cands, d_cand, s);
        if (e == hipSuccess) e = launch_volume_spatial_peaks(d_cand, d_seg, m, d_peaks, s);
        if (e == hipSuccess && points) {
            std::memcpy(pp + pin_items, items.data(), item_bytes);
            std::memcpy(pp + pin_ritems, rank_items.data(), rank_bytes);
            HIP_TRY(hipMemcpyAsync(dp + at_items, pp + pin_items, item_bytes, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(dp + at_ritems, pp + pin_ritems, rank_bytes, hipMemcpyHostToDevice, s));
            e = bounded_launches(rank_compares, kComparesPerLaunch,
                                 [&](size_t i0, int n) { return launch_volume_spatial_rank(d_cand, d_seg, d_ritems + i0, n, d_rank, s); });
            if (e == hipSuccess) e = launch_volume_spatial_place(d_cand, d_rank, d_int, a, d_seg, cands, d_points, s);
            if (e == hipSuccess)
                e = bounded_launches(item_pairs, kPairsPerLaunch, [&](size_t i0, int n) {
                    return launch_volume_spatial_pairs(d_points, d_seg, d_items + i0, n, d_slots + 4 * i0, s);
                });
        }
        if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume spatial launch: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(p + at_peaks, d_peaks, M * 6 * sizeof(long long), hipMemcpyDeviceToHost, s));
        if (points) HIP_TRY(hipMemcpyAsync(pp + pin_slots, d_slots, slot_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const long long *const peaks = reinterpret_cast<const long long *>(p + at_peaks);
        for (int r = 0; r < m; ++r) {
            if (!t[r].voxels) continue;
            const long long *const k = peaks + 6 * (size_t)r;
            t[r].gp_sum = k[0]; t[r].gp_n = k[1]; t[r].gp_at = (int32_t)k[2];
            t[r].lp_sum = k[3]; t[r].lp_n = k[4]; t[r].lp_at = (int32_t)k[5];
        }
        // a component's sums: its items' slots in the order of the work list
        const double *const slots = reinterpret_cast<const double *>(pp + pin_slots);
        for (size_t i = 0; i < items.size(); ++i) {
            mi_unet_vspatial &c = t[items[i].comp];
            c.s0 += slots[4 * i + 0]; c.s1 += slots[4 * i + 1]; c.s2 += slots[4 * i + 2]; c.s3 += slots[4 * i + 3];
        }
    }
    std::memcpy(table, t, M * sizeof(mi_unet_vspatial));
    return MI_UNET_OK;
}
#endif

}  // extern "C"
