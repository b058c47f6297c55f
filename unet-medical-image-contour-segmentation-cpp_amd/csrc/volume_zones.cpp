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

#include "texture_common.h"

static_assert(sizeof(mi_unet_vzones) == 56, "mi_unet_vzones is 56 bytes without padding");
static_assert(sizeof(mi_unet_vzones_opts) == 20, "mi_unet_vzones_opts is five ints");
static_assert(sizeof(mi_unet_vzone) == 16, "mi_unet_vzone is four int32");
static_assert(sizeof(mi_unet_vzone_features) == 128, "mi_unet_vzone_features is 16 doubles");

namespace miunet {

namespace {

constexpr mi_unet_vzones_opts kDefaultOpts{ MI_UNET_VTEX_COUNT, 32, 0, 1, 32 };

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_zones_args(const char *fn, const int32_t *ids, const uint16_t *intensity, int D, int H, int W, int m, const mi_unet_vzones_opts &o,
                     const mi_unet_vzones *table, const mi_unet_vzone *zones, int cap, const int *found)
{
    const std::string f = fn;
    if (!ids || !intensity || !table) return fail(MI_UNET_EARG, f + ": null argument");
    if ((zones == nullptr) != (found == nullptr)) return fail(MI_UNET_EARG, f + ": zones and found are both given or both null");
    if (int rc = check_texture_volume(f, D, H, W, m, common_opts(o))) return rc;
    if (o.max_run < 2 || o.max_run > MI_UNET_VZONES_MAX_RUN)
        return fail(MI_UNET_EARG, f + ": max_run " + std::to_string(o.max_run) + " (2 .. " + std::to_string(MI_UNET_VZONES_MAX_RUN) + ")");
    if ((int64_t)m * o.levels * o.max_run > (int64_t)MI_UNET_VTEX_MAX_CELLS)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components at " + std::to_string(o.levels) + " levels and max_run " +
                                      std::to_string(o.max_run) + " pass 2^22 cells per table");
    if (int rc = check_texture_bins(f, common_opts(o))) return rc;
    if (zones && (cap < 1 || cap > MI_UNET_VZONES_MAX_CAP))
        return fail(MI_UNET_EARG, f + ": cap " + std::to_string(cap) + " (1 .. " + std::to_string(MI_UNET_VZONES_MAX_CAP) + ")");
    return MI_UNET_OK;
}

// the 13 offsets as (dx, dy, dz), the 4 with dz = 0 first
constexpr int kOffsets[13][3] = { { 1, 0, 0 }, { -1, 1, 0 }, { 0, 1, 0 }, { 1, 1, 0 }, { -1, -1, 1 }, { 0, -1, 1 }, { 1, -1, 1 }, { -1, 0, 1 },
                                  { 0, 0, 1 }, { 1, 0, 1 }, { -1, 1, 1 }, { 0, 1, 1 }, { 1, 1, 1 } };

int check_feature_args(const std::string &f, const mi_unet_vzones *c, const void *data, const void *out, int L)
{
    if (!c || !data || !out) return fail(MI_UNET_EARG, f + ": null argument");
    return check_texture_component(f, c->voxels, L);
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
    const std::vector<int32_t> key = texture_keys(ids, intensity, dhw, common_opts(o), t);
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
        int64_t n_zones = 0;
        for_each_zone(key, D, H, W, [&](int32_t first, int32_t k, const std::vector<int32_t> &members) {
            const int32_t size = (int32_t)members.size();
            mi_unet_vzones &c = t[(k >> 8) - 1];
            ++c.zones;
            c.largest_zone = std::max(c.largest_zone, size);
            if (n_zones < cap) zones[n_zones] = mi_unet_vzone{ first, (k >> 8) - 1, k & 255, size };
            ++n_zones;                                          // (at most D * H * W <= 2^28)
        });
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
    matrix_features(cells_of(rlm_row, L, R), L, (double)c->voxels * (double)directions, out, nullptr);
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
    matrix_features(cells, L, (double)c->voxels, out, nullptr);
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
    Layout lay;
    const size_t at_table = lay.take(table_bytes), at_found = lay.take(256), at_inter = lay.take(cells_bytes), at_axial = lay.take(cells_bytes);
    const size_t at_zones = lay.take(keep * sizeof(mi_unet_vzone)), at_keys = lay.take(dhw * sizeof(int32_t)), at_int = lay.take(dhw * sizeof(uint16_t));
    const size_t host_need = lay.end;                           // the stacks are staged behind the results, where the device keeps what only it needs
    const size_t at_range = lay.take(M * sizeof(int2)), at_acc = lay.take(M * sizeof(VznAcc));
    const size_t at_parent = lay.take(zones ? dhw * sizeof(int32_t) : 0), at_size = lay.take(zones ? dhw * sizeof(int32_t) : 0);
    const size_t at_scan = lay.take(scan_ints * sizeof(int32_t));
    // launch_volume_texture_keys takes m L^2 <= 2^22 at once; a call beyond that (L above R) goes through it in parts of `part_m`
    // components, which need the ids kept, a stack for the part and one for the joined keys
    const int part_m = (int)std::min<int64_t>(m, (int64_t)MI_UNET_VTEX_MAX_CELLS / ((int64_t)o.levels * o.levels));
    const bool parts = part_m < m;
    const size_t at_part = lay.take(parts ? dhw * sizeof(int32_t) : 0), at_joined = lay.take(parts ? dhw * sizeof(int32_t) : 0);
    hipStream_t s = h->stream;
    if (int rc = h->ws_vzn.reserve(lay.end, host_need, s)) return rc;
    uint8_t *const d = h->ws_vzn.d, *const p = h->ws_vzn.p;
    if (int rc = upload_stacks(h, h->ws_vzn, at_keys, ids, at_int, intensity, dhw)) return rc;
    VolumeTextureArgs ta = texture_args(D, H, W, m, common_opts(o));
    VolumeZonesArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m; a.L = o.levels; a.R = o.max_run;
    // the 13-offset table is the sum of its two parts, so it needs both
    const int want = rlm ? (VZN_WANT_AXIAL | VZN_WANT_INTER) : rlm_axial ? VZN_WANT_AXIAL : 0;
    int32_t *const d_ids = reinterpret_cast<int32_t *>(d + at_keys), *const d_part = reinterpret_cast<int32_t *>(d + at_part);
    int32_t *const d_keys = parts ? reinterpret_cast<int32_t *>(d + at_joined) : d_ids;      // (one part: the ids become the keys in place)
    int2 *const d_range = reinterpret_cast<int2 *>(d + at_range);
    VznAcc *const d_acc = reinterpret_cast<VznAcc *>(d + at_acc);
    mi_unet_vzones *const d_table = reinterpret_cast<mi_unet_vzones *>(d + at_table);
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
    mi_unet_vzones *const t = reinterpret_cast<mi_unet_vzones *>(p + at_table);
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
