// volume_nbhood.cpp -- per component of a labelled stack its neighbourhood-difference, dependence and distance-zone tables
// (include/mi_unet.h: mi_unet_volume_nbhood): the argument checks, the definition as sequential host arithmetic
// (mi_unet_volume_nbhood_host), the function that turns the counts of one component into features and the entry point on the handle,
// which owns the stage's workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h;
// tests/cpu/volume_nbhood_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "texture_common.h"

static_assert(sizeof(mi_unet_vnbhood) == 44, "mi_unet_vnbhood is eleven int32 without padding");
static_assert(sizeof(mi_unet_vnbhood_opts) == 24, "mi_unet_vnbhood_opts is six ints");
static_assert(sizeof(mi_unet_vnbhood_out) == 8 * sizeof(void *), "mi_unet_vnbhood_out is eight pointers");
static_assert(sizeof(mi_unet_vnbhood_features) == 304, "mi_unet_vnbhood_features is 38 doubles");

namespace miunet {

namespace {

constexpr mi_unet_vnbhood_opts kDefaultOpts{ MI_UNET_VTEX_COUNT, 32, 0, 1, 0, 32 };
constexpr mi_unet_vnbhood_out kNoTables{ nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
constexpr int kCols = 27, kColsAxial = 9;

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_nbhood_args(const char *fn, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vnbhood_opts &o,
                      const mi_unet_vnbhood *table, const mi_unet_vnbhood_out &out)
{
    const std::string f = fn;
    if (!ids || !intensity || !table) return fail(MI_UNET_EARG, f + ": null argument");
    if ((out.ngt_count == nullptr) != (out.ngt_diff == nullptr)) return fail(MI_UNET_EARG, f + ": ngt_count and ngt_diff are both given or both null");
    if ((out.ngt_count_axial == nullptr) != (out.ngt_diff_axial == nullptr))
        return fail(MI_UNET_EARG, f + ": ngt_count_axial and ngt_diff_axial are both given or both null");
    if (int rc = check_texture_volume(f, D, H, W, m, common_opts(o))) return rc;
    if (o.alpha < 0 || o.alpha > o.levels - 1)
        return fail(MI_UNET_EARG, f + ": alpha " + std::to_string(o.alpha) + " (0 .. " + std::to_string(o.levels - 1) + ")");
    if (o.max_dist < 1 || o.max_dist > MI_UNET_VNBHOOD_MAX_DIST)
        return fail(MI_UNET_EARG, f + ": max_dist " + std::to_string(o.max_dist) + " (1 .. " + std::to_string(MI_UNET_VNBHOOD_MAX_DIST) + ")");
    if ((int64_t)m * o.levels * std::max({ o.levels, 32, o.max_dist }) > (int64_t)MI_UNET_VTEX_MAX_CELLS)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components at " + std::to_string(o.levels) + " levels and max_dist " +
                                      std::to_string(o.max_dist) + " pass 2^22 cells per table");
    return check_texture_bins(f, common_opts(o));
}

// the five NGTDM features from one component's count and diff rows of `cols` columns
void ngtdm_features(const uint32_t *count, const uint64_t *diff, int L, int cols, mi_unet_vnbhood_features *o)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> p((size_t)L + 1, 0.0), s((size_t)L + 1, 0.0);
    std::vector<int64_t> ni((size_t)L + 1, 0);
    int64_t N = 0;
    if (count)
        for (int l = 0; l < L; ++l)
            for (int c = 1; c < cols; ++c) {
                ni[(size_t)l + 1] += count[(size_t)l * cols + c];
                s[(size_t)l + 1] += (double)diff[(size_t)l * cols + c] / (double)c;
            }
    for (int i = 1; i <= L; ++i) N += ni[(size_t)i];
    if (N == 0) {
        o->coarseness = o->contrast = o->busyness = o->complexity = o->strength = nan;
        return;
    }
    const double n = (double)N;
    int G = 0;
    double ps = 0.0, ss = 0.0;
    for (int i = 1; i <= L; ++i) {
        if (!ni[(size_t)i]) continue;
        ++G;
        p[(size_t)i] = (double)ni[(size_t)i] / n;
        ps += p[(size_t)i] * s[(size_t)i];
        ss += s[(size_t)i];
    }
    double con = 0.0, busy = 0.0, cpx = 0.0, str = 0.0;
    for (int i = 1; i <= L; ++i) {
        if (!ni[(size_t)i]) continue;
        for (int j = 1; j <= L; ++j) {
            if (!ni[(size_t)j]) continue;
            const double pi = p[(size_t)i], pj = p[(size_t)j], d = (double)(i - j), d2 = d * d;
            con += pi * pj * d2;
            busy += std::fabs((double)i * pi - (double)j * pj);
            cpx += std::fabs(d) * (pi * s[(size_t)i] + pj * s[(size_t)j]) / (pi + pj);
            str += (pi + pj) * d2;
        }
    }
    o->coarseness = ps == 0.0 ? 1e6 : 1.0 / ps;
    o->contrast = G == 1 ? 0.0 : con / ((double)G * (double)(G - 1)) * ss / n;
    o->busyness = busy == 0.0 ? 0.0 : ps / busy;
    o->complexity = cpx / n;
    o->strength = ss == 0.0 ? 0.0 : str / ss;
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_nbhood_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vnbhood_opts *opts,
                               mi_unet_vnbhood *table, const mi_unet_vnbhood_out *out)
{
    const mi_unet_vnbhood_opts o = opts ? *opts : kDefaultOpts;
    const mi_unet_vnbhood_out w = out ? *out : kNoTables;
    if (int rc = check_nbhood_args("mi_unet_volume_nbhood_host", ids, intensity, D, H, W, m, o, table, w)) return rc;
    const int L = o.levels, Dm = o.max_dist;
    const size_t dhw = (size_t)D * H * W, rows = (size_t)m * L;
    std::vector<mi_unet_vnbhood> t((size_t)m);
    std::memset(t.data(), 0, t.size() * sizeof(mi_unet_vnbhood));
    const std::vector<int32_t> key = texture_keys(ids, intensity, dhw, common_opts(o), t);
    if (w.ngt_count) std::memset(w.ngt_count, 0, rows * kCols * sizeof(uint32_t));
    if (w.ngt_diff) std::memset(w.ngt_diff, 0, rows * kCols * sizeof(uint64_t));
    if (w.dep) std::memset(w.dep, 0, rows * kCols * sizeof(uint32_t));
    if (w.ngt_count_axial) std::memset(w.ngt_count_axial, 0, rows * kColsAxial * sizeof(uint32_t));
    if (w.ngt_diff_axial) std::memset(w.ngt_diff_axial, 0, rows * kColsAxial * sizeof(uint64_t));
    if (w.dep_axial) std::memset(w.dep_axial, 0, rows * kColsAxial * sizeof(uint32_t));
    if (w.dzm) std::memset(w.dzm, 0, rows * Dm * sizeof(uint32_t));
    if (w.dzm_axial) std::memset(w.dzm_axial, 0, rows * Dm * sizeof(uint32_t));
    auto inside = [&](int x, int y, int z) { return x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D; };
    if (w.ngt_count || w.dep || w.ngt_count_axial || w.dep_axial) {
        size_t i = 0;
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x, ++i) {
                    const int32_t k = key[i];
                    if (!k) continue;
                    const int id = k >> 8, l = k & 255;
                    int c8 = 0, s8 = 0, k8 = 0, c26 = 0, s26 = 0, k26 = 0;
                    for (int dz = -1; dz <= 1; ++dz)
                        for (int dy = -1; dy <= 1; ++dy)
                            for (int dx = -1; dx <= 1; ++dx) {
                                if ((!dx && !dy && !dz) || !inside(x + dx, y + dy, z + dz)) continue;
                                const int32_t q = key[(size_t)((ptrdiff_t)i + ((ptrdiff_t)dz * H + dy) * W + dx)];
                                if ((q >> 8) != id) continue;
                                const int ql = q & 255, near = std::abs(ql - l) <= o.alpha;
                                ++c26; s26 += ql; k26 += near;
                                if (!dz) { ++c8; s8 += ql; k8 += near; }
                            }
                    mi_unet_vnbhood &c = t[id - 1];
                    const size_t row = (size_t)(id - 1) * L + l;
                    if (w.ngt_count) {
                        ++w.ngt_count[row * kCols + c26];
                        w.ngt_diff[row * kCols + c26] += (uint64_t)std::abs(c26 * l - s26);
                        c.valid += c26 > 0;
                    }
                    if (w.dep) {
                        ++w.dep[row * kCols + k26];
                        c.dependence_max = std::max(c.dependence_max, k26 + 1);
                    }
                    if (w.ngt_count_axial) {
                        ++w.ngt_count_axial[row * kColsAxial + c8];
                        w.ngt_diff_axial[row * kColsAxial + c8] += (uint64_t)std::abs(c8 * l - s8);
                        c.valid_axial += c8 > 0;
                    }
                    if (w.dep_axial) ++w.dep_axial[row * kColsAxial + k8];
                }
    }
    if (w.dzm || w.dzm_axial) {
        // the distance, one axis after the other: along a line forward and backward, carry = same component ? value before + 1 : 1
        std::vector<uint16_t> da(dhw, 0xFFFF), df;
        auto sweep = [&](std::vector<uint16_t> &v, size_t first, size_t step, int n) {
            for (int pass = 0; pass < 2; ++pass) {
                int prev_id = -1, prev_val = 0;
                for (int j = 0; j < n; ++j) {
                    const size_t i = first + (size_t)(pass ? n - 1 - j : j) * step;
                    const int id = key[i] >> 8;
                    const int val = std::min<int>(v[i], id == prev_id ? prev_val + 1 : 1);
                    v[i] = (uint16_t)val;
                    prev_id = id; prev_val = val;
                }
            }
        };
        for (size_t row = 0; row < (size_t)D * H; ++row) sweep(da, row * W, 1, W);
        for (int z = 0; z < D; ++z)
            for (int x = 0; x < W; ++x) sweep(da, (size_t)z * H * W + x, (size_t)W, H);
        if (w.dzm) {
            df = da;
            for (size_t c = 0; c < (size_t)H * W; ++c) sweep(df, c, (size_t)H * W, D);
        }
        for (size_t i = 0; i < dhw; ++i) {
            if (!key[i]) continue;
            mi_unet_vnbhood &c = t[(key[i] >> 8) - 1];
            if (w.dzm) c.deepest = std::max<int32_t>(c.deepest, df[i]);
            if (w.dzm_axial) c.deepest_axial = std::max<int32_t>(c.deepest_axial, da[i]);
        }
        for_each_zone(key, D, H, W, [&](int32_t, int32_t k, const std::vector<int32_t> &members) {
            int near_f = 0xFFFF, near_a = 0xFFFF;
            for (const int32_t p : members) {
                if (w.dzm) near_f = std::min<int>(near_f, df[(size_t)p]);
                near_a = std::min<int>(near_a, da[(size_t)p]);
            }
            mi_unet_vnbhood &c = t[(k >> 8) - 1];
            const size_t row = ((size_t)((k >> 8) - 1) * L + (k & 255)) * Dm;
            ++c.zones;
            if (w.dzm) {
                ++w.dzm[row + (size_t)(std::min(near_f, Dm) - 1)];
                c.clamped += near_f > Dm;
            }
            if (w.dzm_axial) {
                ++w.dzm_axial[row + (size_t)(std::min(near_a, Dm) - 1)];
                c.clamped_axial += near_a > Dm;
            }
        });
    }
    std::memcpy(table, t.data(), t.size() * sizeof(mi_unet_vnbhood));
    return MI_UNET_OK;
}

int mi_unet_volume_nbhood_derive(const mi_unet_vnbhood *c, const mi_unet_vnbhood_out *rows, int L, int Dm, int axial, mi_unet_vnbhood_features *out)
{
    const std::string f = "mi_unet_volume_nbhood_derive";
    if (!c || !rows || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_texture_component(f, c->voxels, L)) return rc;
    if (Dm < 1 || Dm > MI_UNET_VNBHOOD_MAX_DIST)
        return fail(MI_UNET_EARG, f + ": max_dist " + std::to_string(Dm) + " (1 .. " + std::to_string(MI_UNET_VNBHOOD_MAX_DIST) + ")");
    const uint32_t *const count = axial ? rows->ngt_count_axial : rows->ngt_count, *const dep = axial ? rows->dep_axial : rows->dep;
    const uint64_t *const diff = axial ? rows->ngt_diff_axial : rows->ngt_diff;
    const uint32_t *const dzm = axial ? rows->dzm_axial : rows->dzm;
    if ((count == nullptr) != (diff == nullptr)) return fail(MI_UNET_EARG, f + ": a count row and its diff row are both given or both null");
    const int cols = axial ? kColsAxial : kCols;
    mi_unet_vnbhood_features o;
    ngtdm_features(count, diff, L, cols, &o);
    matrix_features(cells_of(dep, L, cols), L, (double)c->voxels, &o.ngldm, &o.dependence_energy);
    matrix_features(cells_of(dzm, L, Dm), L, (double)c->voxels, &o.gldzm, nullptr);
    *out = o;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_nbhood(mi_unet_t *h, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vnbhood_opts *opts,
                          mi_unet_vnbhood *table, const mi_unet_vnbhood_out *out)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vnbhood_opts o = opts ? *opts : kDefaultOpts;
    const mi_unet_vnbhood_out w = out ? *out : kNoTables;
    if (int rc = check_nbhood_args("mi_unet_volume_nbhood", ids, intensity, D, H, W, m, o, table, w)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, M = (size_t)m, rows = M * o.levels;
    const int want = (w.ngt_count ? VNB_WANT_NGT : 0) | (w.dep ? VNB_WANT_DEP : 0) | (w.ngt_count_axial ? VNB_WANT_NGT_AXIAL : 0) |
                     (w.dep_axial ? VNB_WANT_DEP_AXIAL : 0) | (w.dzm ? VNB_WANT_DZM : 0) | (w.dzm_axial ? VNB_WANT_DZM_AXIAL : 0);
    const bool zones = want & (VNB_WANT_DZM | VNB_WANT_DZM_AXIAL);
    // device and pinned alike: the table, then the tables that were asked for, one behind the other: one copy brings them all back
    const size_t n_count = w.ngt_count ? rows * kCols * sizeof(uint32_t) : 0, n_diff = w.ngt_count ? rows * kCols * sizeof(uint64_t) : 0;
    const size_t n_dep = w.dep ? rows * kCols * sizeof(uint32_t) : 0;
    const size_t n_count_a = w.ngt_count_axial ? rows * kColsAxial * sizeof(uint32_t) : 0, n_diff_a = w.ngt_count_axial ? rows * kColsAxial * sizeof(uint64_t) : 0;
    const size_t n_dep_a = w.dep_axial ? rows * kColsAxial * sizeof(uint32_t) : 0;
    const size_t n_dzm = w.dzm ? rows * o.max_dist * sizeof(uint32_t) : 0, n_dzm_a = w.dzm_axial ? rows * o.max_dist * sizeof(uint32_t) : 0;
    Layout lay;
    const size_t at_table = lay.take(M * sizeof(mi_unet_vnbhood)), at_count = lay.take(n_count), at_diff = lay.take(n_diff), at_dep = lay.take(n_dep);
    const size_t at_count_a = lay.take(n_count_a), at_diff_a = lay.take(n_diff_a), at_dep_a = lay.take(n_dep_a);
    const size_t at_dzm = lay.take(n_dzm), at_dzm_a = lay.take(n_dzm_a), results = lay.end;
    // device only: keys (ids in place), intensity, range, the zone stage's accumulators and ours, the forest with its sizes and scan,
    // one record and `found` that the zone list wants, the zones' minima, both distance stacks
    const size_t at_keys = lay.take(dhw * sizeof(int32_t)), at_int = lay.take(dhw * sizeof(uint16_t));
    const size_t host_need = lay.end;                           // the stacks are staged behind the results, where the device keeps what only it needs
    const size_t at_range = lay.take(M * sizeof(int2)), at_zacc = lay.take(M * sizeof(VznAcc)), at_acc = lay.take(M * sizeof(VnbAcc)), at_one = lay.take(512);
    const size_t stack = zones ? dhw * sizeof(int32_t) : 0, half = zones ? dhw * sizeof(uint16_t) : 0;
    const size_t at_parent = lay.take(stack), at_size = lay.take(stack), at_scan = lay.take(zones ? vzn_scan_ints(dhw) * sizeof(int32_t) : 0);
    const size_t at_zmin_a = lay.take(w.dzm_axial ? stack : 0), at_da = lay.take(half), at_df = lay.take(w.dzm ? half : 0);
    hipStream_t s = h->stream;
    if (int rc = h->ws_vnb.reserve(lay.end, host_need, s)) return rc;
    uint8_t *const d = h->ws_vnb.d, *const p = h->ws_vnb.p;
    if (int rc = upload_stacks(h, h->ws_vnb, at_keys, ids, at_int, intensity, dhw)) return rc;
    const VolumeTextureArgs ta = texture_args(D, H, W, m, common_opts(o));
    VolumeZonesArgs za;
    za.D = D; za.H = H; za.W = W; za.m = m; za.L = o.levels; za.R = 1;
    VolumeNbhoodArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m; a.L = o.levels; a.alpha = o.alpha; a.Dm = o.max_dist;
    VnbTables t;
    t.count = reinterpret_cast<uint32_t *>(d + at_count); t.diff = reinterpret_cast<unsigned long long *>(d + at_diff);
    t.dep = reinterpret_cast<uint32_t *>(d + at_dep);
    t.count_axial = reinterpret_cast<uint32_t *>(d + at_count_a); t.diff_axial = reinterpret_cast<unsigned long long *>(d + at_diff_a);
    t.dep_axial = reinterpret_cast<uint32_t *>(d + at_dep_a);
    t.dzm = reinterpret_cast<uint32_t *>(d + at_dzm); t.dzm_axial = reinterpret_cast<uint32_t *>(d + at_dzm_a);
    int32_t *const d_keys = reinterpret_cast<int32_t *>(d + at_keys);
    int2 *const d_range = reinterpret_cast<int2 *>(d + at_range);
    VznAcc *const d_zacc = reinterpret_cast<VznAcc *>(d + at_zacc);
    VnbAcc *const d_acc = reinterpret_cast<VnbAcc *>(d + at_acc);
    int32_t *const d_parent = reinterpret_cast<int32_t *>(d + at_parent), *const d_size = reinterpret_cast<int32_t *>(d + at_size);
    uint16_t *const d_da = reinterpret_cast<uint16_t *>(d + at_da), *const d_df = w.dzm ? reinterpret_cast<uint16_t *>(d + at_df) : nullptr;
    hipError_t e = launch_volume_texture_keys(d_keys, reinterpret_cast<const uint16_t *>(d + at_int), ta, d_range, s);
    // (with nothing wanted the run launcher clears the zone stage's accumulators and counts the voxels; it touches neither table)
    if (e == hipSuccess) e = launch_volume_zones_runs(d_keys, za, 0, d_zacc, t.count, t.count, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, M * sizeof(VnbAcc), s);
    bool lds_table = kVnbLdsTable;
    if (const char *v = std::getenv("MIUNET_VNB_EXP")) {       // (experiments) 1: every count straight to memory, 2: the leader's counts in LDS
        const int form = std::atoi(v);
        lds_table = form == 2 || (form != 1 && kVnbLdsTable);
    }
    if (e == hipSuccess) e = launch_volume_nbhood_gather(d_keys, a, want, lds_table, t, s);
    if (e == hipSuccess && zones) {
        e = launch_volume_nbhood_dist(d_keys, a, d_da, d_df, s);
        // the list itself is not wanted: one record, and the forest stays behind in `parent`; the sizes are done with after it, so the
        // zones' minima of d take their place
        if (e == hipSuccess)
            e = launch_volume_zones_list(d_keys, za, d_parent, d_size, reinterpret_cast<int32_t *>(d + at_scan), d_zacc,
                                         reinterpret_cast<mi_unet_vzone *>(d + at_one), 1, reinterpret_cast<int32_t *>(d + at_one + 256), s);
        if (e == hipSuccess)
            e = launch_volume_nbhood_zones(d_keys, a, want, d_parent, d_da, d_df, d_size, reinterpret_cast<int32_t *>(d + at_zmin_a), d_acc, t, s);
    }
    if (e == hipSuccess) e = launch_volume_nbhood_finish(d_range, a, want, d_zacc, d_acc, t, reinterpret_cast<mi_unet_vnbhood *>(d + at_table), s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume nbhood launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p, d, results, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(table, p + at_table, M * sizeof(mi_unet_vnbhood));
    if (w.ngt_count) std::memcpy(w.ngt_count, p + at_count, n_count);
    if (w.ngt_diff) std::memcpy(w.ngt_diff, p + at_diff, n_diff);
    if (w.dep) std::memcpy(w.dep, p + at_dep, n_dep);
    if (w.ngt_count_axial) std::memcpy(w.ngt_count_axial, p + at_count_a, n_count_a);
    if (w.ngt_diff_axial) std::memcpy(w.ngt_diff_axial, p + at_diff_a, n_diff_a);
    if (w.dep_axial) std::memcpy(w.dep_axial, p + at_dep_a, n_dep_a);
    if (w.dzm) std::memcpy(w.dzm, p + at_dzm, n_dzm);
    if (w.dzm_axial) std::memcpy(w.dzm_axial, p + at_dzm_a, n_dzm_a);
    return MI_UNET_OK;
}
#endif

}  // extern "C"
