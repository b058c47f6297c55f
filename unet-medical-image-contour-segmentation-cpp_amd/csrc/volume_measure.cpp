// volume_measure.cpp -- per component of a labelled stack its moments, its intensity and its longest diameters (include/mi_unet.h:
// mi_unet_volume_measure): the argument checks, the definition as sequential host arithmetic
// (mi_unet_volume_measure_host), the function that turns an entry into millimetres (mi_unet_volume_measure_derive) and the entry point on
// the handle, which owns the stage's workspace and splits the pair search into launches of bounded work.  With
// MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h; tests/cpu/volume_measure_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vmeasure) == 128, "mi_unet_vmeasure is 128 bytes without padding");
static_assert(sizeof(mi_unet_vmeasure_opts) == 4, "mi_unet_vmeasure_opts is one int");
static_assert(sizeof(mi_unet_vmeasure_shape) == 19 * sizeof(double), "mi_unet_vmeasure_shape is 19 doubles");

namespace miunet {

namespace {

constexpr mi_unet_vmeasure_opts kDefaultOpts{ 262144 };
constexpr int kMaxSide = MI_UNET_SCORE_VOLUME_MAX_SIDE;

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_measure_args(const char *fn, const int32_t *ids, int D, int H, int W, int m, const int *units, const mi_unet_vmeasure_opts &o,
                       const mi_unet_vmeasure *table)
{
    const std::string f = fn;
    if (!ids || !units || !table) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_max(f, D, H, W, kMaxSide)) return rc;
    if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return fail(MI_UNET_EARG, f + ": D * H * W must stay below 2^31");    // (< 2^39: no overflow)
    if (m < 1 || m > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components (1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE) + ")");
    if (int rc = check_units_min1(f, units)) return rc;
    if (!d2_fits(D, H, W, units)) return fail(MI_UNET_EARG, f + ": the squared diagonal of the volume in spacing units must stay below 2^31");
    if (o.max_ends < 0 || o.max_ends > MI_UNET_VMEASURE_MAX_ENDS_LIMIT)
        return fail(MI_UNET_EARG, f + ": max_ends " + std::to_string(o.max_ends) + " is outside 0 .. " + std::to_string(MI_UNET_VMEASURE_MAX_ENDS_LIMIT));
    return MI_UNET_OK;
}

inline bool searched(const mi_unet_vmeasure &t, int max_ends) { return t.ends >= 1 && t.ends <= max_ends; }

inline void set_diameters(mi_unet_vmeasure &t, int32_t v) { t.d2 = t.dp = t.dq = t.a_d2 = t.a_p = t.a_q = v; }

struct End { int32_t x, y, z, idx; };       // pre-scaled coordinates and the voxel's index

// the definition of the pair search over one component's run ends in index order: the first strictly larger d2 of an ascending scan is
// the pair with the smallest p, then the smallest q
void search(const End *e, int n, mi_unet_vmeasure &t)
{
    int32_t best = -1, best_a = -1;
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            const int32_t dx = e[i].x - e[j].x, dy = e[i].y - e[j].y, dz = e[i].z - e[j].z;
            const int32_t d2 = dx * dx + dy * dy + dz * dz;
            if (d2 > best) { best = d2; t.d2 = d2; t.dp = e[i].idx; t.dq = e[j].idx; }
            if (dz == 0 && d2 > best_a) { best_a = d2; t.a_d2 = d2; t.a_p = e[i].idx; t.a_q = e[j].idx; }
        }
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_measure_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const int spacing_units[3],
                                const mi_unet_vmeasure_opts *opts, mi_unet_vmeasure *table)
{
    const mi_unet_vmeasure_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_measure_args("mi_unet_volume_measure_host", ids, D, H, W, m, spacing_units, o, table)) return rc;
    std::vector<mi_unet_vmeasure> t((size_t)m);
    std::memset(t.data(), 0, t.size() * sizeof(mi_unet_vmeasure));
    auto member = [&](int32_t id) { return id >= 1 && id <= m; };
    auto is_end = [&](const int32_t *p, int x) { return (x == 0 || p[-1] != *p) || (x == W - 1 || p[1] != *p); };
    const int32_t *p = ids;
    const uint16_t *v = intensity;
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x, ++p) {
                if (!member(*p)) continue;
                mi_unet_vmeasure &c = t[*p - 1];
                if (intensity) {
                    const int32_t iv = v[p - ids];
                    c.imin = c.voxels ? std::min(c.imin, iv) : iv;
                    c.imax = c.voxels ? std::max(c.imax, iv) : iv;
                    c.si += iv;
                    c.sii += (int64_t)iv * iv;
                }
                ++c.voxels;
                c.ends += is_end(p, x);
                c.sx += x; c.sy += y; c.sz += z;
                c.sxx += (int64_t)x * x; c.syy += (int64_t)y * y; c.szz += (int64_t)z * z;
                c.sxy += (int64_t)x * y; c.sxz += (int64_t)x * z; c.syz += (int64_t)y * z;
            }
    // the run ends of the searched components, a segment each, in index order
    std::vector<size_t> first((size_t)m + 1, 0);
    for (int r = 0; r < m; ++r) first[r + 1] = first[r] + (searched(t[r], o.max_ends) ? (size_t)t[r].ends : 0);
    std::vector<End> ends(first[m]);
    std::vector<size_t> at(first.begin(), first.end() - 1);
    p = ids;
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x, ++p)
                if (member(*p) && searched(t[*p - 1], o.max_ends) && is_end(p, x))
                    ends[at[*p - 1]++] = End{ x * spacing_units[0], y * spacing_units[1], z * spacing_units[2], (int32_t)(p - ids) };
    for (int r = 0; r < m; ++r) {
        if (searched(t[r], o.max_ends)) search(ends.data() + first[r], t[r].ends, t[r]);
        else if (t[r].voxels) set_diameters(t[r], -1);
    }
    std::memcpy(table, t.data(), t.size() * sizeof(mi_unet_vmeasure));
    return MI_UNET_OK;
}

int mi_unet_volume_measure_derive(const mi_unet_vmeasure *c, const int spacing_units[3], double unit_mm, mi_unet_vmeasure_shape *out)
{
    const std::string f = "mi_unet_volume_measure_derive";
    if (!c || !spacing_units || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (c->voxels < 1) return fail(MI_UNET_EARG, f + ": voxels " + std::to_string(c->voxels) + " (a component has at least one voxel)");
    if (int rc = check_units_min1(f, spacing_units)) return rc;
    if (!std::isfinite(unit_mm) || !(unit_mm > 0.0)) return fail(MI_UNET_EARG, f + ": unit_mm must be finite and > 0");
    const double s[3] = { spacing_units[0] * unit_mm, spacing_units[1] * unit_mm, spacing_units[2] * unit_mm };
    const __int128 A = c->voxels;
    const double Ad = (double)c->voxels, A2 = Ad * Ad;
    // exact 128-bit numerators, converted once: A * sxx < 2^88, sx^2 < 2^88
    auto central = [&](int64_t sab, int64_t sa, int64_t sb) { return (double)(A * sab - (__int128)sa * sb) / A2; };
    const int64_t first[3] = { c->sx, c->sy, c->sz };
    const int64_t second[3][3] = { { c->sxx, c->sxy, c->sxz }, { c->sxy, c->syy, c->syz }, { c->sxz, c->syz, c->szz } };
    double M[3][3], V[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };      // M = V^T C V stays symmetric; the columns of V are the vectors
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) M[a][b] = central(second[a][b], first[a], first[b]) * s[a] * s[b] + (a == b ? s[a] * s[a] / 12.0 : 0.0);
    // cyclic Jacobi: 16 sweeps over (0, 1), (0, 2), (1, 2); a 3 x 3 symmetric matrix is diagonal to rounding after five or six
    for (int sweep = 0; sweep < 16; ++sweep)
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
            if (M[p][q] == 0.0) continue;
            const double theta = (M[q][q] - M[p][p]) / (2.0 * M[p][q]);
            const double tn = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
            const double cs = 1.0 / std::sqrt(tn * tn + 1.0), sn = tn * cs;
            for (int k = 0; k < 3; ++k) {                       // columns p, q of M, then rows p, q
                const double kp = M[k][p], kq = M[k][q];
                M[k][p] = cs * kp - sn * kq;
                M[k][q] = sn * kp + cs * kq;
            }
            for (int k = 0; k < 3; ++k) {
                const double pk = M[p][k], qk = M[q][k];
                M[p][k] = cs * pk - sn * qk;
                M[q][k] = sn * pk + cs * qk;
            }
            M[p][q] = M[q][p] = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double kp = V[k][p], kq = V[k][q];
                V[k][p] = cs * kp - sn * kq;
                V[k][q] = sn * kp + cs * kq;
            }
        }
    int order[3] = { 0, 1, 2 };
    std::stable_sort(order, order + 3, [&](int a, int b) { return M[a][a] > M[b][b]; });
    mi_unet_vmeasure_shape o;
    o.cx_mm = ((double)c->sx / Ad + 0.5) * s[0];
    o.cy_mm = ((double)c->sy / Ad + 0.5) * s[1];
    o.cz_mm = ((double)c->sz / Ad + 0.5) * s[2];
    for (int i = 0; i < 3; ++i) {
        const int col = order[i];
        o.axis_mm[i] = 2.0 * std::sqrt(5.0 * std::max(M[col][col], 0.0));
        double v[3] = { V[0][col], V[1][col], V[2][col] };
        const double norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        int big = 0;
        for (int k = 1; k < 3; ++k)
            if (std::fabs(v[k]) > std::fabs(v[big])) big = k;
        const double sign = v[big] < 0.0 ? -1.0 : 1.0;
        for (int k = 0; k < 3; ++k) o.axis_dir[i][k] = sign * v[k] / norm;
    }
    o.mean = (double)c->si / Ad;
    o.std = std::sqrt(std::max(central(c->sii, c->si, c->si), 0.0));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    o.diameter_mm = c->d2 < 0 ? nan : std::sqrt((double)c->d2) * unit_mm;
    o.axial_diameter_mm = c->a_d2 < 0 ? nan : std::sqrt((double)c->a_d2) * unit_mm;
    *out = o;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
// The pairs one launch of the search may hold.  k_vms_pairs runs at 1e12 pairs / s and more on an MI355X (DESIGN.md 7.13 has the measured
// rate), so a launch of 2^30 pairs takes about a millisecond, a hundred times the cost of launching it: a component at the default cap of
// 2^18 run ends (3.4e10 pairs) becomes 32 launches, one at the limit of 2^20 (5.5e11 pairs) 512, and none of them can occupy the device
// for long.
constexpr int64_t kPairsPerLaunch = (int64_t)1 << 30;

int mi_unet_volume_measure(mi_unet_t *h, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const int spacing_units[3],
                           const mi_unet_vmeasure_opts *opts, mi_unet_vmeasure *table)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vmeasure_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_measure_args("mi_unet_volume_measure", ids, D, H, W, m, spacing_units, o, table)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, M = (size_t)m;
    // device: ids, intensity, table, seg, diam | cursor, keys; pinned: the same up to diam
    const size_t at_int = up256(dhw * sizeof(int32_t)), at_table = at_int + up256(intensity ? dhw * sizeof(uint16_t) : 0);
    const size_t at_seg = at_table + up256(M * sizeof(mi_unet_vmeasure)), at_diam = at_seg + up256(M * sizeof(int2));
    const size_t at_cursor = at_diam + up256(M * 6 * sizeof(int32_t)), at_keys = at_cursor + up256(M * sizeof(int));
    const size_t dev_need = at_keys + up256(M * 2 * sizeof(unsigned long long)), host_need = at_cursor;
    hipStream_t s = h->stream;
    if (int rc = h->ws_vms.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vms.d, *const p = h->ws_vms.p;
    host_copy(h, p, ids, dhw * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(d, p, dhw * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (intensity) {
        host_copy(h, p + at_int, intensity, dhw * sizeof(uint16_t));
        HIP_TRY(hipMemcpyAsync(d + at_int, p + at_int, dhw * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    }
    VolumeMeasureArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m; a.ux = spacing_units[0]; a.uy = spacing_units[1]; a.uz = spacing_units[2];
    const int32_t *const d_ids = reinterpret_cast<const int32_t *>(d);
    mi_unet_vmeasure *const d_table = reinterpret_cast<mi_unet_vmeasure *>(d + at_table);
    hipError_t e = launch_volume_measure_sums(d_ids, intensity ? reinterpret_cast<const uint16_t *>(d + at_int) : nullptr, a, d_table, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume measure launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p + at_table, d_table, M * sizeof(mi_unet_vmeasure), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                           // the run ends size the segments and the work list
    mi_unet_vmeasure *const t = reinterpret_cast<mi_unet_vmeasure *>(p + at_table);
    int2 *const seg = reinterpret_cast<int2 *>(p + at_seg);
    size_t points = 0;
    std::vector<VmsItem> items;
    std::vector<int64_t> item_pairs;
    constexpr int kTilesPerItem = 32;                           // b-tiles a workgroup takes: 2 M pairs, some tens of microseconds
    for (int r = 0; r < m; ++r) {
        t[r].imin = intensity && t[r].voxels ? 65535 - t[r].imin : 0;
        seg[r] = make_int2(0, 0);
        if (!searched(t[r], o.max_ends)) {
            if (t[r].voxels) set_diameters(t[r], -1);
            continue;
        }
        seg[r] = make_int2((int)points, t[r].ends);             // (points <= D * H * W < 2^31)
        points += (size_t)t[r].ends;
        const int tiles = (t[r].ends + VMS_TILE - 1) / VMS_TILE;
        for (int ta = 0; ta < tiles; ++ta) {
            const int64_t na = std::min(VMS_TILE, t[r].ends - ta * VMS_TILE);
            for (int tb = ta; tb < tiles; tb += kTilesPerItem) {
                const int nt = std::min(kTilesPerItem, tiles - tb);
                items.push_back(VmsItem{ r, ta, tb, nt });
                item_pairs.push_back(na * (std::min<int64_t>(t[r].ends, (int64_t)(tb + nt) * VMS_TILE) - (int64_t)tb * VMS_TILE));
            }
        }
    }
    if (points) {
        const size_t at_items = up256(points * sizeof(int4)), item_bytes = items.size() * sizeof(VmsItem);
        if (int rc = h->ws_vms_pts.reserve(at_items + up256(item_bytes), up256(item_bytes), s)) return rc;     // (nothing of the stage is in flight here)
        uint8_t *const dp = h->ws_vms_pts.d, *const pp = h->ws_vms_pts.p;
        std::memcpy(pp, items.data(), item_bytes);
        const int2 *const d_seg = reinterpret_cast<const int2 *>(d + at_seg);
        int4 *const d_points = reinterpret_cast<int4 *>(dp);
        const VmsItem *const d_items = reinterpret_cast<const VmsItem *>(dp + at_items);
        unsigned long long *const d_keys = reinterpret_cast<unsigned long long *>(d + at_keys);
        int32_t *const d_diam = reinterpret_cast<int32_t *>(d + at_diam);
        HIP_TRY(hipMemcpyAsync(d + at_seg, p + at_seg, M * sizeof(int2), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(dp + at_items, pp, item_bytes, hipMemcpyHostToDevice, s));
        e = launch_volume_measure_fill(d_ids, a, d_seg, reinterpret_cast<int *>(d + at_cursor), d_keys, d_points, s);
        // the work list in launches of bounded work: a launch ends once the next item would pass the bound
        for (size_t i0 = 0; e == hipSuccess && i0 < items.size();) {
            size_t i1 = i0;
            for (int64_t pairs = 0; i1 < items.size() && (i1 == i0 || pairs + item_pairs[i1] <= kPairsPerLaunch); ++i1) pairs += item_pairs[i1];
            e = launch_volume_measure_pairs(d_points, d_seg, d_items + i0, (int)(i1 - i0), d_keys, s);
            i0 = i1;
        }
        if (e == hipSuccess) e = launch_volume_measure_ends(d_points, d_seg, d_keys, a, d_diam, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume measure launch: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(p + at_diam, d_diam, M * 6 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const int32_t *const diam = reinterpret_cast<const int32_t *>(p + at_diam);
        for (int r = 0; r < m; ++r)
            if (seg[r].y > 0) std::memcpy(&t[r].d2, diam + 6 * (size_t)r, 6 * sizeof(int32_t));
    }
    std::memcpy(table, t, M * sizeof(mi_unet_vmeasure));
    return MI_UNET_OK;
}
#endif

}  // extern "C"
