// volume_zones.cpp -- per component of a labelled stack its grey-level run-length and size-zone matrices (include/mi_unet.h:
// mi_unet_volume_zones): the argument checks, the definition as sequential host arithmetic (mi_unet_volume_zones_host),
// the two functions that turn the counts of one component into features and the entry point on the handle, which owns the stage's
// workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h; tests/cpu/volume_zones_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vzones) == 56, "mi_unet_vzones is 56 bytes without padding");
static_assert(sizeof(mi_unet_vzones_opts) == 20, "mi_unet_vzones_opts is five ints");
static_assert(sizeof(mi_unet_vzone) == 16, "mi_unet_vzone is four int32");
static_assert(sizeof(mi_unet_vzone_features) == 128, "mi_unet_vzone_features is 16 doubles");

namespace miunet {

namespace {

constexpr mi_unet_vzones_opts kDefaultOpts{ MI_UNET_VTEX_COUNT, 32, 0, 1, 32 };
constexpr int kMaxSide = MI_UNET_SCORE_VOLUME_MAX_SIDE;

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_zones_args(const char *fn, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vzones_opts &o,
                     const mi_unet_vzones *table, const mi_unet_vzone *zones, int cap, const int *found)
{
    const std::string f = fn;
    if (!ids || !intensity || !table) return fail(MI_UNET_EARG, f + ": null argument");
    if ((zones == nullptr) != (found == nullptr)) return fail(MI_UNET_EARG, f + ": zones and found are both given or both null");
    if (int rc = check_sides_max(f, D, H, W, kMaxSide)) return rc;
    if ((int64_t)D * H * W > (int64_t)MI_UNET_VTEX_MAX_VOXELS) return fail(MI_UNET_EARG, f + ": D * H * W must not pass 2^28");   // (< 2^39: no overflow)
    if (m < 1 || m > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components (1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE) + ")");
    if (o.mode != MI_UNET_VTEX_COUNT && o.mode != MI_UNET_VTEX_WIDTH) return fail(MI_UNET_EARG, f + ": mode " + std::to_string(o.mode) + " does not exist");
    if (o.levels < 2 || o.levels > MI_UNET_VTEX_MAX_LEVELS)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(o.levels) + " levels (2 .. " + std::to_string(MI_UNET_VTEX_MAX_LEVELS) + ")");
    if (o.max_run < 2 || o.max_run > MI_UNET_VZONES_MAX_RUN)
        return fail(MI_UNET_EARG, f + ": max_run " + std::to_string(o.max_run) + " (2 .. " + std::to_string(MI_UNET_VZONES_MAX_RUN) + ")");
    if ((int64_t)m * o.levels * o.max_run > (int64_t)MI_UNET_VTEX_MAX_CELLS)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components at " + std::to_string(o.levels) + " levels and max_run " +
                                      std::to_string(o.max_run) + " pass 2^22 cells per table");
    if (o.width < 1 || o.width > 65536) return fail(MI_UNET_EARG, f + ": width " + std::to_string(o.width) + " is outside 1 .. 65536");
    if (o.lo < 0 || o.lo > 65535) return fail(MI_UNET_EARG, f + ": lo " + std::to_string(o.lo) + " is outside 0 .. 65535");
    if (zones && (cap < 1 || cap > MI_UNET_VZONES_MAX_CAP))
        return fail(MI_UNET_EARG, f + ": cap " + std::to_string(cap) + " (1 .. " + std::to_string(MI_UNET_VZONES_MAX_CAP) + ")");
    return MI_UNET_OK;
}

// the 13 offsets as (dx, dy, dz), the 4 with dz = 0 first
constexpr int kOffsets[13][3] = { { 1, 0, 0 }, { -1, 1, 0 }, { 0, 1, 0 }, { 1, 1, 0 }, { -1, -1, 1 }, { 0, -1, 1 }, { 1, -1, 1 }, { -1, 0, 1 },
                                  { 0, 0, 1 }, { 1, 0, 1 }, { -1, 1, 1 }, { 0, 1, 1 }, { 1, 1, 1 } };

struct Cell {
    int64_t i, j, c;            // level + 1, run length or zone size, count
};

// the 16 features over the non-zero cells of one matrix, sorted by (i, j); `space` = voxels * directions
void features(const std::vector<Cell> &cells, int L, double space, mi_unet_vzone_features *out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    mi_unet_vzone_features o;
    int64_t N = 0, si = 0, sj = 0;
    std::vector<int64_t> ni((size_t)L + 1, 0);
    std::vector<std::pair<int64_t, int64_t>> nj;                // (j, n_j), j ascending
    for (const Cell &c : cells) {
        N += c.c;
        ni[(size_t)c.i] += c.c;
        si += c.i * c.c;
        sj += c.j * c.c;
        nj.emplace_back(c.j, c.c);
    }
    if (N == 0) {
        double *const v = reinterpret_cast<double *>(&o);
        for (int k = 0; k < 16; ++k) v[k] = nan;
        *out = o;
        return;
    }
    std::sort(nj.begin(), nj.end());
    size_t u = 0;
    for (size_t k = 0; k < nj.size(); ++k) {
        if (u && nj[u - 1].first == nj[k].first) nj[u - 1].second += nj[k].second;
        else nj[u++] = nj[k];
    }
    nj.resize(u);
    const double n = (double)N, mu_i = (double)si / n, mu_j = (double)sj / n;
    double se = 0.0, le = 0.0, lg = 0.0, hg = 0.0, gn = 0.0, sn = 0.0;
    for (const auto &e : nj) {
        const double j = (double)e.first, c = (double)e.second;
        se += c / (j * j);
        le += c * (j * j);
        sn += c * c;
    }
    for (int i = 1; i <= L; ++i) {
        if (!ni[(size_t)i]) continue;
        const double c = (double)ni[(size_t)i], ii = (double)i * (double)i;
        lg += c / ii;
        hg += c * ii;
        gn += c * c;
    }
    double sl = 0.0, sh = 0.0, ll = 0.0, lh = 0.0, gv = 0.0, sv = 0.0, ent = 0.0;
    for (const Cell &cell : cells) {
        const double c = (double)cell.c, ii = (double)cell.i * (double)cell.i, jj = (double)cell.j * (double)cell.j, p = c / n;
        const double di = (double)cell.i - mu_i, dj = (double)cell.j - mu_j;
        sl += c / (ii * jj);
        sh += c * ii / jj;
        ll += c * jj / ii;
        lh += c * ii * jj;
        gv += di * di * p;
        sv += dj * dj * p;
        ent -= p * std::log2(p);
    }
    o.short_emphasis = se / n; o.long_emphasis = le / n; o.low_grey_emphasis = lg / n; o.high_grey_emphasis = hg / n;
    o.short_low = sl / n; o.short_high = sh / n; o.long_low = ll / n; o.long_high = lh / n;
    o.grey_nonuniformity = gn / n; o.grey_nonuniformity_norm = gn / n / n;
    o.size_nonuniformity = sn / n; o.size_nonuniformity_norm = sn / n / n;
    o.percentage = n / space;
    o.grey_variance = gv; o.size_variance = sv; o.entropy = ent;
    *out = o;
}

int check_feature_args(const std::string &f, const mi_unet_vzones *c, const void *data, const void *out, int L)
{
    if (!c || !data || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (c->voxels < 1) return fail(MI_UNET_EARG, f + ": voxels " + std::to_string(c->voxels) + " (a component has at least one voxel)");
    if (L < 2 || L > MI_UNET_VTEX_MAX_LEVELS) return fail(MI_UNET_EARG, f + ": " + std::to_string(L) + " levels (2 .. " + std::to_string(MI_UNET_VTEX_MAX_LEVELS) + ")");
    return MI_UNET_OK;
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_zones_host(const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vzones_opts *opts,
                              mi_unet_vzones *table, uint32_t *rlm, uint32_t *rlm_axial, mi_unet_vzone *zones, int cap, int *found)
{
    const mi_unet_vzones_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_zones_args("mi_unet_volume_zones_host", ids, intensity, D, H, W, m, o, table, zones, cap, found)) return rc;
    const int L = o.levels, R = o.max_run;
    const size_t dhw = (size_t)D * H * W, cells = (size_t)m * L * R;
    std::vector<mi_unet_vzones> t((size_t)m);
    std::memset(t.data(), 0, t.size() * sizeof(mi_unet_vzones));
    auto member = [&](int32_t id) { return id >= 1 && id <= m; };
    for (size_t i = 0; i < dhw; ++i) {
        if (!member(ids[i])) continue;
        mi_unet_vzones &c = t[ids[i] - 1];
        const int32_t v = intensity[i];
        c.imin = c.voxels ? std::min(c.imin, v) : v;
        c.imax = c.voxels ? std::max(c.imax, v) : v;
        ++c.voxels;
    }
    std::vector<int32_t> key(dhw, 0);
    for (size_t i = 0; i < dhw; ++i) {
        if (!member(ids[i])) continue;
        const mi_unet_vzones &c = t[ids[i] - 1];
        const int32_t v = intensity[i];
        int32_t l;
        if (o.mode == MI_UNET_VTEX_COUNT) l = ((v - c.imin) * L) / (c.imax - c.imin + 1);
        else l = v < o.lo ? 0 : std::min(L - 1, (v - o.lo) / o.width);
        key[i] = (ids[i] << 8) | l;
    }
    if (rlm) std::memset(rlm, 0, cells * sizeof(uint32_t));
    if (rlm_axial) std::memset(rlm_axial, 0, cells * sizeof(uint32_t));
    auto inside = [&](int x, int y, int z) { return x >= 0 && x < W && y >= 0 && y < H && z >= 0 && z < D; };
    if (rlm || rlm_axial) {
        const int n_off = rlm ? 13 : 4;
        size_t i = 0;
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x, ++i) {
                    const int32_t k = key[i];
                    if (!k) continue;
                    mi_unet_vzones &c = t[(k >> 8) - 1];
                    const size_t row = ((size_t)((k >> 8) - 1) * L + (k & 255)) * R;
                    for (int d = 0; d < n_off; ++d) {
                        const int dx = kOffsets[d][0], dy = kOffsets[d][1], dz = kOffsets[d][2];
                        const ptrdiff_t step = ((ptrdiff_t)dz * H + dy) * W + dx;
                        if (inside(x - dx, y - dy, z - dz) && key[(size_t)((ptrdiff_t)i - step)] == k) continue;     // not the run's first voxel
                        int n = 1;
                        for (int qx = x + dx, qy = y + dy, qz = z + dz; inside(qx, qy, qz) && key[(size_t)((ptrdiff_t)i + n * step)] == k;
                             qx += dx, qy += dy, qz += dz)
                            ++n;
                        const size_t cell = row + (size_t)(std::min(n, R) - 1);
                        if (rlm) {
                            ++rlm[cell];
                            ++c.runs;
                            c.clamped += n > R;
                            c.longest_run = std::max(c.longest_run, n);
                        }
                        if (rlm_axial && dz == 0) {
                            ++rlm_axial[cell];
                            ++c.runs_axial;
                            c.clamped_axial += n > R;
                        }
                    }
                }
    }
    if (zones) {
        // raster order: the first voxel of a zone that has not been seen opens it; the zone is flooded from there
        std::vector<uint8_t> seen(dhw, 0);
        std::vector<int32_t> todo;
        int64_t n_zones = 0;
        for (size_t i = 0; i < dhw; ++i) {
            const int32_t k = key[i];
            if (!k || seen[i]) continue;
            int32_t size = 0;
            seen[i] = 1;
            todo.assign(1, (int32_t)i);
            while (!todo.empty()) {
                const int32_t p = todo.back();
                todo.pop_back();
                ++size;
                const int px = p % W, py = (p / W) % H, pz = p / (W * H);
                for (int dz = -1; dz <= 1; ++dz)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            if (!inside(px + dx, py + dy, pz + dz)) continue;
                            const int32_t q = p + (dz * H + dy) * W + dx;
                            if (key[(size_t)q] != k || seen[(size_t)q]) continue;
                            seen[(size_t)q] = 1;
                            todo.push_back(q);
                        }
            }
            mi_unet_vzones &c = t[(k >> 8) - 1];
            ++c.zones;
            c.largest_zone = std::max(c.largest_zone, size);
            if (n_zones < cap) zones[n_zones] = mi_unet_vzone{ (int32_t)i, (k >> 8) - 1, k & 255, size };
            ++n_zones;                                          // (at most D * H * W <= 2^28)
        }
        if (n_zones < cap) std::memset(zones + n_zones, 0, (size_t)(cap - n_zones) * sizeof(mi_unet_vzone));
        *found = (int)n_zones;
    }
    std::memcpy(table, t.data(), t.size() * sizeof(mi_unet_vzones));
    return MI_UNET_OK;
}

int mi_unet_volume_zones_run_features(const mi_unet_vzones *c, const uint32_t *rlm_row, int L, int R, int directions, mi_unet_vzone_features *out)
{
    const std::string f = "mi_unet_volume_zones_run_features";
    if (int rc = check_feature_args(f, c, rlm_row, out, L)) return rc;
    if (R < 2 || R > MI_UNET_VZONES_MAX_RUN)
        return fail(MI_UNET_EARG, f + ": max_run " + std::to_string(R) + " (2 .. " + std::to_string(MI_UNET_VZONES_MAX_RUN) + ")");
    if (directions != 13 && directions != 4) return fail(MI_UNET_EARG, f + ": " + std::to_string(directions) + " directions (13 or 4)");
    std::vector<Cell> cells;
    for (int l = 0; l < L; ++l)
        for (int j = 0; j < R; ++j)
            if (const uint32_t v = rlm_row[(size_t)l * R + j]) cells.push_back(Cell{ l + 1, j + 1, (int64_t)v });
    features(cells, L, (double)c->voxels * (double)directions, out);
    return MI_UNET_OK;
}

int mi_unet_volume_zones_zone_features(const mi_unet_vzones *c, const mi_unet_vzone *zones, int nz, int r, int L, mi_unet_vzone_features *out)
{
    const std::string f = "mi_unet_volume_zones_zone_features";
    if (nz < 0) return fail(MI_UNET_EARG, f + ": " + std::to_string(nz) + " records");
    if (int rc = check_feature_args(f, c, nz ? static_cast<const void *>(zones) : static_cast<const void *>(c), out, L)) return rc;
    std::vector<std::pair<int32_t, int32_t>> mine;              // (level, size) of the records of r
    for (int k = 0; k < nz; ++k) {
        if (zones[k].component != r) continue;
        if (zones[k].level < 0 || zones[k].level >= L)
            return fail(MI_UNET_EARG, f + ": record " + std::to_string(k) + " has level " + std::to_string(zones[k].level) + " (0 .. " + std::to_string(L - 1) + ")");
        if (zones[k].size < 1) return fail(MI_UNET_EARG, f + ": record " + std::to_string(k) + " has size " + std::to_string(zones[k].size));
        mine.emplace_back(zones[k].level, zones[k].size);
    }
    std::sort(mine.begin(), mine.end());
    std::vector<Cell> cells;
    for (const auto &e : mine) {
        if (!cells.empty() && cells.back().i == e.first + 1 && cells.back().j == e.second) ++cells.back().c;
        else cells.push_back(Cell{ e.first + 1, e.second, 1 });
    }
    features(cells, L, (double)c->voxels, out);
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_zones(mi_unet_t *h, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vzones_opts *opts,
                         mi_unet_vzones *table, uint32_t *rlm, uint32_t *rlm_axial, mi_unet_vzone *zones, int cap, int *found)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vzones_opts o = opts ? *opts : kDefaultOpts;
    if (int rc = check_zones_args("mi_unet_volume_zones", ids, intensity, D, H, W, m, o, table, zones, cap, found)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, M = (size_t)m;
    const size_t table_bytes = M * sizeof(mi_unet_vzones), cells_bytes = M * o.levels * o.max_run * sizeof(uint32_t);
    const size_t keep = zones ? std::min((size_t)cap, dhw) : 0;              // (a volume has at most a zone per voxel)
    const size_t scan_ints = zones ? vzn_scan_ints(dhw) : 0;
    // device and pinned alike: table, found, inter (then rlm), axial, zones | device only: keys (ids in place), intensity, range, acc,
    // parent, size, scan
    const size_t at_found = up256(table_bytes), at_inter = at_found + 256, at_axial = at_inter + up256(cells_bytes);
    const size_t at_zones = at_axial + up256(cells_bytes), at_keys = at_zones + up256(keep * sizeof(mi_unet_vzone));
    const size_t at_int = at_keys + up256(dhw * sizeof(int32_t)), at_range = at_int + up256(dhw * sizeof(uint16_t));
    const size_t at_acc = at_range + up256(M * sizeof(int2)), at_parent = at_acc + up256(M * sizeof(VznAcc));
    const size_t at_size = at_parent + (zones ? up256(dhw * sizeof(int32_t)) : 0), at_scan = at_size + (zones ? up256(dhw * sizeof(int32_t)) : 0);
    // launch_volume_texture_keys takes m L^2 <= 2^22 at once; a call beyond that (L above R) goes through it in parts of `part_m`
    // components, which need the ids kept, a stack for the part and one for the joined keys
    const int part_m = (int)std::min<int64_t>(m, (int64_t)MI_UNET_VTEX_MAX_CELLS / ((int64_t)o.levels * o.levels));
    const bool parts = part_m < m;
    const size_t at_part = at_scan + up256(scan_ints * sizeof(int32_t)), at_joined = at_part + (parts ? up256(dhw * sizeof(int32_t)) : 0);
    const size_t dev_need = at_joined + (parts ? up256(dhw * sizeof(int32_t)) : 0);
    // the stacks are staged behind the results, where the device keeps what only it needs
    const size_t host_need = at_int + up256(dhw * sizeof(uint16_t));
    hipStream_t s = h->stream;
    if (int rc = h->ws_vzn.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vzn.d, *const p = h->ws_vzn.p;
    host_copy(h, p + at_keys, ids, dhw * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(d + at_keys, p + at_keys, dhw * sizeof(int32_t), hipMemcpyHostToDevice, s));
    host_copy(h, p + at_int, intensity, dhw * sizeof(uint16_t));
    HIP_TRY(hipMemcpyAsync(d + at_int, p + at_int, dhw * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    VolumeTextureArgs ta;
    ta.D = D; ta.H = H; ta.W = W; ta.m = m; ta.mode = o.mode; ta.L = o.levels; ta.lo = o.lo; ta.width = o.width;
    VolumeZonesArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m; a.L = o.levels; a.R = o.max_run;
    // the 13-offset table is the sum of its two parts, so it needs both
    const int want = rlm ? (VZN_WANT_AXIAL | VZN_WANT_INTER) : rlm_axial ? VZN_WANT_AXIAL : 0;
    int32_t *const d_ids = reinterpret_cast<int32_t *>(d + at_keys), *const d_part = reinterpret_cast<int32_t *>(d + at_part);
    int32_t *const d_keys = parts ? reinterpret_cast<int32_t *>(d + at_joined) : d_ids;      // (one part: the ids become the keys in place)
    int2 *const d_range = reinterpret_cast<int2 *>(d + at_range);
    VznAcc *const d_acc = reinterpret_cast<VznAcc *>(d + at_acc);
    mi_unet_vzones *const d_table = reinterpret_cast<mi_unet_vzones *>(d);
    int32_t *const d_found = reinterpret_cast<int32_t *>(d + at_found);
    uint32_t *const d_inter = reinterpret_cast<uint32_t *>(d + at_inter), *const d_axial = reinterpret_cast<uint32_t *>(d + at_axial);
    mi_unet_vzone *const d_zones = reinterpret_cast<mi_unet_vzone *>(d + at_zones);
    hipError_t e = hipSuccess;
    if (!parts) {
        e = launch_volume_texture_keys(d_keys, reinterpret_cast<const uint16_t *>(d + at_int), ta, d_range, s);
    } else {
        HIP_TRY(hipMemsetAsync(d_keys, 0, dhw * sizeof(int32_t), s));
        for (int first = 0; first < m && e == hipSuccess; first += part_m) {
            ta.m = std::min(part_m, m - first);
            e = launch_volume_zones_part(d_ids, a, first, ta.m, d_part, s);
            if (e == hipSuccess) e = launch_volume_texture_keys(d_part, reinterpret_cast<const uint16_t *>(d + at_int), ta, d_range + first, s);
            if (e == hipSuccess) e = launch_volume_zones_join(d_part, a, first, d_keys, s);
        }
    }
    if (e == hipSuccess) e = launch_volume_zones_runs(d_keys, a, want, d_acc, d_inter, d_axial, s);
    if (e == hipSuccess && zones)
        e = launch_volume_zones_list(d_keys, a, reinterpret_cast<int32_t *>(d + at_parent), reinterpret_cast<int32_t *>(d + at_size),
                                     reinterpret_cast<int32_t *>(d + at_scan), d_acc, d_zones, (int)keep, d_found, s);
    if (e == hipSuccess) e = launch_volume_zones_finish(d_range, a, want, d_acc, d_inter, d_axial, d_table, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume zones launch: ") + hipGetErrorString(e));
    // the results in one copy up to the tables that were asked for; of the list the first records, the rest once `found` is known
    const size_t eager = std::min(keep, kVznEagerZones);
    const size_t head = rlm_axial ? at_zones : rlm ? at_axial : at_inter;
    HIP_TRY(hipMemcpyAsync(p, d, head, hipMemcpyDeviceToHost, s));
    if (eager) HIP_TRY(hipMemcpyAsync(p + at_zones, d_zones, eager * sizeof(mi_unet_vzone), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const int n_found = zones ? *reinterpret_cast<const int32_t *>(p + at_found) : 0;
    const size_t n = std::min((size_t)std::max(n_found, 0), keep);
    if (n > eager) {
        HIP_TRY(hipMemcpyAsync(p + at_zones + eager * sizeof(mi_unet_vzone), d_zones + eager, (n - eager) * sizeof(mi_unet_vzone),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    mi_unet_vzones *const t = reinterpret_cast<mi_unet_vzones *>(p);
    if (!rlm_axial)
        for (int r = 0; r < m; ++r) t[r].runs_axial = t[r].clamped_axial = 0;      // (a part of rlm, not asked for as a table)
    std::memcpy(table, t, table_bytes);
    if (rlm) std::memcpy(rlm, p + at_inter, cells_bytes);
    if (rlm_axial) std::memcpy(rlm_axial, p + at_axial, cells_bytes);
    if (zones) {
        std::memcpy(zones, p + at_zones, n * sizeof(mi_unet_vzone));
        if (n < (size_t)cap) std::memset(zones + n, 0, ((size_t)cap - n) * sizeof(mi_unet_vzone));
        *found = n_found;
    }
    return MI_UNET_OK;
}
#endif

}  // extern "C"
