// volume.cpp -- a stack of masks labelled as one volume (include/mi_unet.h: mi_unet_volume_components): the argument
// checks, the definition as pure host arithmetic (mi_unet_volume_components_host), the derived metrics (mi_unet_volume_derive) and the
// entry point on the handle, which owns the stage's workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled
// (stage_common.h; tests/cpu/volume_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vcomp) == 88, "mi_unet_vcomp is 88 bytes without padding");

namespace miunet {

namespace {

constexpr mi_unet_volume_opts kDefaultVolumeOpts{ 26, 0, 0 };

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_volume_args(const char *fn, const uint8_t *masks, int D, int H, int W, const int *values, int n, const mi_unet_volume_opts &o,
                      const mi_unet_vcomp *table, int cap, const int32_t *found, const int32_t *kept)
{
    const std::string f = fn;
    if (!masks || !values || !table || !found || !kept) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_min1(f, D, H, W)) return rc;
    if (int rc = check_values(f, values, n, MI_UNET_VOLUME_MAX_VALUES)) return rc;
    if (cap < 1 || cap > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": cap " + std::to_string(cap) + " is outside 1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE));
    if (o.connectivity != 6 && o.connectivity != 18 && o.connectivity != 26)
        return fail(MI_UNET_EARG, f + ": connectivity " + std::to_string(o.connectivity) + " is none of 6, 18, 26");
    if (o.min_voxels < 0) return fail(MI_UNET_EARG, f + ": min_voxels " + std::to_string(o.min_voxels) + " is negative");
    if (o.keep_largest < 0) return fail(MI_UNET_EARG, f + ": keep_largest " + std::to_string(o.keep_largest) + " is negative");
    if (!product_below_2_31(n, D, H, W)) return fail(MI_UNET_EARG, f + ": n * D * H * W must stay below 2^31");
    return MI_UNET_OK;
}

int find(std::vector<int32_t> &parent, int i)
{
    while (parent[i] != i) {
        parent[i] = parent[parent[i]];
        i = parent[i];
    }
    return i;
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_components_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const mi_unet_volume_opts *opts,
                                   uint8_t *out, int32_t *ids, mi_unet_vcomp *table, int cap, int32_t *found, int32_t *kept)
{
    const mi_unet_volume_opts o = opts ? *opts : kDefaultVolumeOpts;
    if (int rc = check_volume_args("mi_unet_volume_components_host", masks, D, H, W, values, n, o, table, cap, found, kept)) return rc;
    const size_t hw = (size_t)H * W, dhw = (size_t)D * hw;
    const int max_axes = o.connectivity == 6 ? 1 : o.connectivity == 18 ? 2 : 3;
    // `out` may be `masks`: every plane reads its set from a copy taken before anything is written
    const std::vector<uint8_t> vol(masks, masks + dhw);
    std::vector<int32_t> parent(dhw), comp(dhw);
    std::vector<mi_unet_vcomp> comps;
    std::vector<int32_t> order, rank_of;
    for (int k = 0; k < n; ++k) {
        const int v = values[k];
        auto in = [&](int z, int y, int x) {
            return z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W && vol[(size_t)z * hw + (size_t)y * W + x] == v;
        };
        // union-find over the 13 neighbours that lie before a voxel in raster order; the smaller root wins, so a root is its
        // component's raster-first voxel
        for (size_t i = 0; i < dhw; ++i) parent[i] = vol[i] == v ? (int32_t)i : -1;
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    if (!in(z, y, x)) continue;
                    const int i = (int)((size_t)z * hw + (size_t)y * W + x);
                    for (int dz = -1; dz <= 0; ++dz)
                        for (int dy = -1; dy <= (dz < 0 ? 1 : 0); ++dy)
                            for (int dx = -1; dx <= ((dz < 0 || dy < 0) ? 1 : -1); ++dx) {
                                if ((dz != 0) + (dy != 0) + (dx != 0) > max_axes || !in(z + dz, y + dy, x + dx)) continue;
                                int a = find(parent, i), b = find(parent, i + dz * (int)hw + dy * W + dx);
                                if (a == b) continue;
                                if (a < b) std::swap(a, b);
                                parent[a] = b;
                            }
                }
        comps.clear();
        for (size_t i = 0; i < dhw; ++i) {                       // raster order: a root comes before every other voxel of its component
            if (parent[i] < 0) { comp[i] = -1; continue; }
            const int r = find(parent, (int)i);
            if (r == (int)i) {
                comp[i] = (int32_t)comps.size();
                comps.push_back(mi_unet_vcomp{ 0, (int32_t)i, W, H, D, -1, -1, -1, 0, v, 0, 0, 0, 0, 0, 0 });
            } else {
                comp[i] = comp[r];
            }
            mi_unet_vcomp &c = comps[comp[i]];
            const int z = (int)(i / hw), y = (int)(i % hw) / W, x = (int)(i % hw) % W;
            ++c.voxels;
            c.x0 = std::min(c.x0, x); c.y0 = std::min(c.y0, y); c.z0 = std::min(c.z0, z);
            c.x1 = std::max(c.x1, x); c.y1 = std::max(c.y1, y); c.z1 = std::max(c.z1, z);
            c.faces_x += !in(z, y, x - 1) + !in(z, y, x + 1);
            c.faces_y += !in(z, y - 1, x) + !in(z, y + 1, x);
            c.faces_z += !in(z - 1, y, x) + !in(z + 1, y, x);
            c.sx += x; c.sy += y; c.sz += z;
        }
        const int nc = (int)comps.size();
        order.resize(nc);
        for (int c = 0; c < nc; ++c) order[c] = c;
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            return comps[a].voxels != comps[b].voxels ? comps[a].voxels > comps[b].voxels : comps[a].first < comps[b].first;
        });
        rank_of.resize(nc);
        int nkept = 0;
        for (int r = 0; r < nc; ++r) {
            mi_unet_vcomp &c = comps[order[r]];
            rank_of[order[r]] = r;
            c.kept = c.voxels >= o.min_voxels && (o.keep_largest == 0 || r < o.keep_largest);
            nkept += c.kept;
        }
        found[k] = nc;
        kept[k] = nkept;
        mi_unet_vcomp *const t = table + (size_t)k * cap;
        for (int r = 0; r < cap; ++r) {
            if (r < nc) t[r] = comps[order[r]];
            else std::memset(&t[r], 0, sizeof t[r]);
        }
        for (size_t i = 0; i < dhw; ++i) {
            const bool keep = comp[i] >= 0 && comps[comp[i]].kept;
            if (out) out[(size_t)k * dhw + i] = keep ? (uint8_t)v : 0;
            if (ids) ids[(size_t)k * dhw + i] = !keep ? 0 : rank_of[comp[i]] < cap ? 1 + rank_of[comp[i]] : -1;
        }
    }
    return MI_UNET_OK;
}

int mi_unet_volume_derive(const mi_unet_vcomp *c, const double spacing_xyz[3], mi_unet_vcomp_metrics *out)
{
    if (!c || !spacing_xyz || !out) return fail(MI_UNET_EARG, "mi_unet_volume_derive: null argument");
    if (c->voxels < 1) return fail(MI_UNET_EARG, "mi_unet_volume_derive: a component has at least one voxel");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing_xyz[a]) || !(spacing_xyz[a] > 0.0))
            return fail(MI_UNET_EARG, "mi_unet_volume_derive: the spacing must be finite and positive");
    const double sx = spacing_xyz[0], sy = spacing_xyz[1], sz = spacing_xyz[2], nv = (double)c->voxels;
    out->volume_mm3 = nv * sx * sy * sz;
    out->surface_mm2 = (double)c->faces_x * sy * sz + (double)c->faces_y * sx * sz + (double)c->faces_z * sx * sy;
    out->cx_mm = ((double)c->sx / nv + 0.5) * sx;
    out->cy_mm = ((double)c->sy / nv + 0.5) * sy;
    out->cz_mm = ((double)c->sz / nv + 0.5) * sz;
    out->extent_x_mm = (double)(c->x1 - c->x0 + 1) * sx;
    out->extent_y_mm = (double)(c->y1 - c->y0 + 1) * sy;
    out->extent_z_mm = (double)(c->z1 - c->z0 + 1) * sz;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_components(mi_unet_t *h, const uint8_t *masks, int D, int H, int W, const int *values, int n,
                              const mi_unet_volume_opts *opts, uint8_t *out, int32_t *ids, mi_unet_vcomp *table, int cap,
                              int32_t *found, int32_t *kept)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_volume_opts o = opts ? *opts : kDefaultVolumeOpts;
    if (int rc = check_volume_args("mi_unet_volume_components", masks, D, H, W, values, n, o, table, cap, found, kept)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, N = dhw * n, table_bytes = (size_t)n * cap * sizeof(mi_unet_vcomp);
    // device and pinned alike: the volume, out, ids (when asked for), the table, found and kept; device only: the kernels' workspace
    const size_t at_out = up256(dhw), at_ids = at_out + up256(N), at_table = at_ids + (ids ? up256(N * sizeof(int32_t)) : 0);
    const size_t at_counts = at_table + up256(table_bytes), at_ws = at_counts + up256((size_t)2 * n * sizeof(int32_t));
    const size_t dev_need = at_ws + volume_workspace_bytes(D, H, W, n), host_need = at_ws;
    hipStream_t s = h->stream;
    if (int rc = h->ws_volume.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_volume.d, *const p = h->ws_volume.p;
    host_copy(h, p, masks, dhw);
    HIP_TRY(hipMemcpyAsync(d, p, dhw, hipMemcpyHostToDevice, s));
    VolumeArgs a;
    a.D = D; a.H = H; a.W = W; a.n = n; a.cap = cap;
    a.connectivity = o.connectivity; a.min_voxels = o.min_voxels; a.keep_largest = o.keep_largest;
    for (int k = 0; k < n; ++k) a.v[k] = values[k];
    const hipError_t e = launch_volume_components(d, a, d + at_out, ids ? reinterpret_cast<int32_t *>(d + at_ids) : nullptr,
                                                  reinterpret_cast<mi_unet_vcomp *>(d + at_table), reinterpret_cast<int32_t *>(d + at_counts),
                                                  d + at_ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume launch: ") + hipGetErrorString(e));
    if (out) HIP_TRY(hipMemcpyAsync(p + at_out, d + at_out, N, hipMemcpyDeviceToHost, s));
    if (ids) HIP_TRY(hipMemcpyAsync(p + at_ids, d + at_ids, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p + at_table, d + at_table, at_ws - at_table, hipMemcpyDeviceToHost, s));      // the table and the counts
    HIP_TRY(hipStreamSynchronize(s));                           // the call's only host synchronisation
    for (int k = 0; k < n; ++k)                                 // (a plane with more roots than slots: impossible, see volume.hip)
        if (reinterpret_cast<const int32_t *>(p + at_counts)[k] < 0) return fail(MI_UNET_EHIP, "mi_unet_volume_components: the slot table overflowed");
    if (out) host_copy(h, out, p + at_out, N);
    if (ids) host_copy(h, ids, p + at_ids, N * sizeof(int32_t));
    memcpy(table, p + at_table, table_bytes);
    memcpy(found, p + at_counts, (size_t)n * sizeof(int32_t));
    memcpy(kept, p + at_counts + (size_t)n * sizeof(int32_t), (size_t)n * sizeof(int32_t));
    return MI_UNET_OK;
}
#endif

}  // extern "C"
