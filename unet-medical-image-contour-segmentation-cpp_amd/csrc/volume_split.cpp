// volume_split.cpp -- touching objects split into pieces: cores regrown by geodesic distance (include/mi_unet.h: mi_unet_volume_split;
// DESIGN.md 7.21): the argument checks, the definition as sequential host arithmetic (mi_unet_volume_split_host: erosion from the
// definition, flood-fill labels, Dijkstra with a binary heap on (length, marker)), the derived metrics (mi_unet_volume_split_derive) and
// the entry point on the handle, which owns the stage's workspace and drives the rounds of the growth.  With MIUNET_NO_DEVICE only the
// host arithmetic is compiled (stage_common.h; tests/cpu/volume_split_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <queue>
#include <string>
#include <utility>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vpiece) == 40, "mi_unet_vpiece is 40 bytes without padding");
static_assert(sizeof(mi_unet_vsplit_stat) == 64, "mi_unet_vsplit_stat is 64 bytes without padding");

namespace miunet {

namespace {

constexpr mi_unet_vsplit_opts kDefaultSplitOpts{ 26, 0, 1 };
constexpr int kMaxR = MI_UNET_VOLUME_CLEAN_MAX_R;
constexpr uint64_t kUnreached = ~(uint64_t)0;

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_split_args(const char *fn, const uint8_t *masks, int D, int H, int W, const int *values, int n, const int *units,
                     const mi_unet_vsplit_opts &o, const mi_unet_vcomp *table, int cap, const int32_t *found)
{
    const std::string f = fn;
    if (!masks || !values || !units || !table || !found) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_min1(f, D, H, W)) return rc;
    if (int rc = check_values(f, values, n, MI_UNET_VOLUME_MAX_VALUES)) return rc;
    if (!product_below_2_31(n, D, H, W)) return fail(MI_UNET_EARG, f + ": n * D * H * W must stay below 2^31");
    for (int a = 0; a < 3; ++a)
        if (units[a] < 1 || units[a] > kMaxR)
            return fail(MI_UNET_EARG, f + ": spacing unit " + std::to_string(units[a]) + " is outside 1 .. " + std::to_string(kMaxR));
    if (o.connectivity != 6 && o.connectivity != 18 && o.connectivity != 26)
        return fail(MI_UNET_EARG, f + ": connectivity " + std::to_string(o.connectivity) + " is none of 6, 18, 26");
    if (o.neck_r < 0 || o.neck_r > kMaxR)
        return fail(MI_UNET_EARG, f + ": neck_r " + std::to_string(o.neck_r) + " is outside 0 .. " + std::to_string(kMaxR));
    if (o.min_core < 0) return fail(MI_UNET_EARG, f + ": min_core " + std::to_string(o.min_core) + " is negative");
    if (cap < 1 || cap > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": cap " + std::to_string(cap) + " is outside 1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE));
    // D H W < 2^31 and the units sum to less than 2^18: the product fits 64 bits
    if ((int64_t)D * H * W * ((int64_t)units[0] + units[1] + units[2]) >= ((int64_t)1 << 33))
        return fail(MI_UNET_EARG, f + ": D * H * W * (ux + uy + uz) must stay below 2^33");
    return MI_UNET_OK;
}

// a piece while it is gathered: the table's entry, the info's entry
struct Piece { mi_unet_vcomp c; mi_unet_vpiece p; };

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_split_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const int spacing_units[3],
                              const mi_unet_vsplit_opts *opts, int32_t *ids, mi_unet_vcomp *table, mi_unet_vpiece *info, int cap,
                              int32_t *found, mi_unet_vsplit_stat *stats, int32_t *rounds)
{
    const mi_unet_vsplit_opts o = opts ? *opts : kDefaultSplitOpts;
    if (int rc = check_split_args("mi_unet_volume_split_host", masks, D, H, W, values, n, spacing_units, o, table, cap, found)) return rc;
    const size_t hw = (size_t)H * W, dhw = (size_t)D * hw;
    const int max_axes = o.connectivity == 6 ? 1 : o.connectivity == 18 ? 2 : 3;
    const int64_t u[3] = { spacing_units[0], spacing_units[1], spacing_units[2] };
    // the neighbours of the connectivity with the cost of the step, and the ball's offsets other than the voxel itself
    struct Step { int dz, dy, dx; int64_t cost; };
    std::vector<Step> steps, ball;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int axes = (dz != 0) + (dy != 0) + (dx != 0);
                if (axes >= 1 && axes <= max_axes) steps.push_back({ dz, dy, dx, (dx != 0) * u[0] + (dy != 0) * u[1] + (dz != 0) * u[2] });
            }
    {
        const int e[3] = { o.neck_r / spacing_units[0], o.neck_r / spacing_units[1], o.neck_r / spacing_units[2] };
        const int64_t r2 = (int64_t)o.neck_r * o.neck_r;
        for (int dz = -std::min(e[2], D - 1); dz <= std::min(e[2], D - 1); ++dz)
            for (int dy = -std::min(e[1], H - 1); dy <= std::min(e[1], H - 1); ++dy)
                for (int dx = -std::min(e[0], W - 1); dx <= std::min(e[0], W - 1); ++dx)
                    if ((dz || dy || dx) && dx * u[0] * dx * u[0] + dy * u[1] * dy * u[1] + dz * u[2] * dz * u[2] <= r2)
                        ball.push_back({ dz, dy, dx, 0 });
    }
    std::vector<uint8_t> set(dhw), core(dhw);
    std::vector<int32_t> lab(dhw), stack, core_size, piece_of_marker;
    std::vector<uint64_t> key(dhw);
    std::vector<Piece> pieces;
    std::vector<int32_t> order, rank_of;
    typedef std::pair<uint64_t, int32_t> Item;
    for (int k = 0; k < n; ++k) {
        const int v = values[k];
        auto at = [&](int z, int y, int x) { return (size_t)z * hw + (size_t)y * W + x; };
        auto inside = [&](int z, int y, int x) { return z >= 0 && z < D && y >= 0 && y < H && x >= 0 && x < W; };
        mi_unet_vsplit_stat st{};
        st.value = v;
        for (size_t i = 0; i < dhw; ++i) { set[i] = masks[i] == v; st.in_voxels += set[i]; }
        // CORES: a voxel of S stays when every voxel of the ball round it that lies inside the volume is in S
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    uint8_t c = set[at(z, y, x)];
                    for (size_t b = 0; c && b < ball.size(); ++b) {
                        const int zz = z + ball[b].dz, yy = y + ball[b].dy, xx = x + ball[b].dx;
                        if (inside(zz, yy, xx) && !set[at(zz, yy, xx)]) c = 0;
                    }
                    core[at(z, y, x)] = c;
                    st.core_voxels += c;
                }
        // flood fill of `sel` from voxel i under the connectivity: every voxel reached gets lab = l; returns their number
        auto flood = [&](const auto &sel, size_t i, int32_t l) {
            int32_t count = 1;
            lab[i] = l;
            stack.assign(1, (int32_t)i);
            while (!stack.empty()) {
                const int32_t p = stack.back();
                stack.pop_back();
                const int z = (int)((size_t)p / hw), y = (int)((size_t)p % hw) / W, x = (int)((size_t)p % hw) % W;
                for (const Step &s : steps) {
                    const int zz = z + s.dz, yy = y + s.dy, xx = x + s.dx;
                    if (!inside(zz, yy, xx)) continue;
                    const size_t q = at(zz, yy, xx);
                    if (!sel(q) || lab[q] >= 0) continue;
                    lab[q] = l;
                    ++count;
                    stack.push_back((int32_t)q);
                }
            }
            return count;
        };
        // the cores in raster order of their first voxels: the label of a core is that voxel, its marker
        std::fill(lab.begin(), lab.end(), -1);
        core_size.assign(dhw, 0);
        for (size_t i = 0; i < dhw; ++i)
            if (core[i] && lab[i] < 0) {
                core_size[i] = flood([&](size_t q) { return core[q] != 0; }, i, (int32_t)i);
                ++st.cores;
                st.cores_kept += core_size[i] >= o.min_core;
            }
        // GROWTH: Dijkstra on (length, marker) from every voxel of every kept core
        std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
        for (size_t i = 0; i < dhw; ++i) {
            key[i] = kUnreached;
            if (core[i] && core_size[lab[i]] >= o.min_core) {
                key[i] = (uint64_t)lab[i];
                heap.push(Item(key[i], (int32_t)i));
            }
        }
        while (!heap.empty()) {
            const Item it = heap.top();
            heap.pop();
            if (it.first != key[it.second]) continue;
            const int32_t p = it.second;
            const int z = (int)((size_t)p / hw), y = (int)((size_t)p % hw) / W, x = (int)((size_t)p % hw) % W;
            for (const Step &s : steps) {
                const int zz = z + s.dz, yy = y + s.dy, xx = x + s.dx;
                if (!inside(zz, yy, xx)) continue;
                const size_t q = at(zz, yy, xx);
                const uint64_t cand = it.first + ((uint64_t)s.cost << 31);
                if (set[q] && cand < key[q]) {
                    key[q] = cand;
                    heap.push(Item(cand, (int32_t)q));
                }
            }
        }
        // the pieces: lab = the index of the voxel's piece.  A cored piece is named by its marker, whichever of its voxels comes first.
        pieces.clear();
        piece_of_marker.assign(dhw, -1);
        std::fill(lab.begin(), lab.end(), -1);
        auto new_piece = [&](int32_t core_first, int32_t core_voxels) {
            Piece pc{};
            pc.c = mi_unet_vcomp{ 0, 0x7FFFFFFF, W, H, D, -1, -1, -1, 1, v, 0, 0, 0, 0, 0, 0 };
            pc.p = mi_unet_vpiece{ core_first, core_voxels, 0, 0, 0, 0 };
            pieces.push_back(pc);
            return (int32_t)pieces.size() - 1;
        };
        for (size_t i = 0; i < dhw; ++i) {
            if (!set[i] || lab[i] >= 0) continue;
            if (key[i] == kUnreached) {
                flood([&](size_t q) { return set[q] && key[q] == kUnreached; }, i, new_piece(-1, 0));
                ++st.coreless;
            } else {
                const int32_t m = (int32_t)(key[i] & 0x7FFFFFFFu);
                if (piece_of_marker[m] < 0) piece_of_marker[m] = new_piece(m, core_size[m]);
                lab[i] = piece_of_marker[m];
            }
        }
        auto piece_at = [&](int z, int y, int x) { return inside(z, y, x) && set[at(z, y, x)] ? lab[at(z, y, x)] : -1; };
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const size_t i = at(z, y, x);
                    if (!set[i]) continue;
                    const int32_t l = lab[i];
                    mi_unet_vcomp &c = pieces[l].c;
                    mi_unet_vpiece &p = pieces[l].p;
                    ++c.voxels;
                    c.first = std::min(c.first, (int32_t)i);
                    c.x0 = std::min(c.x0, x); c.y0 = std::min(c.y0, y); c.z0 = std::min(c.z0, z);
                    c.x1 = std::max(c.x1, x); c.y1 = std::max(c.y1, y); c.z1 = std::max(c.z1, z);
                    c.sx += x; c.sy += y; c.sz += z;
                    if (key[i] != kUnreached) p.reach = std::max(p.reach, (int64_t)(key[i] >> 31));
                    const int32_t nb[6] = { piece_at(z, y, x - 1), piece_at(z, y, x + 1), piece_at(z, y - 1, x), piece_at(z, y + 1, x),
                                            piece_at(z - 1, y, x), piece_at(z + 1, y, x) };
                    int64_t *const faces[3] = { &c.faces_x, &c.faces_y, &c.faces_z }, *const cut[3] = { &p.cut_x, &p.cut_y, &p.cut_z };
                    for (int j = 0; j < 6; ++j) {
                        *faces[j / 2] += nb[j] != l;
                        *cut[j / 2] += nb[j] != l && nb[j] >= 0;
                    }
                }
        const int np = (int)pieces.size();
        order.resize(np);
        for (int c = 0; c < np; ++c) order[c] = c;
        std::sort(order.begin(), order.end(), [&](int a, int b) {
            return pieces[a].c.voxels != pieces[b].c.voxels ? pieces[a].c.voxels > pieces[b].c.voxels : pieces[a].c.first < pieces[b].c.first;
        });
        rank_of.resize(np);
        for (int r = 0; r < np; ++r) {
            rank_of[order[r]] = r;
            st.max_reach = std::max(st.max_reach, pieces[order[r]].p.reach);
        }
        st.pieces = np;
        found[k] = np;
        for (int r = 0; r < cap; ++r) {
            mi_unet_vcomp *const t = table + (size_t)k * cap + r;
            mi_unet_vpiece *const q = info ? info + (size_t)k * cap + r : nullptr;
            if (r < np) {
                *t = pieces[order[r]].c;
                if (q) *q = pieces[order[r]].p;
            } else {
                std::memset(t, 0, sizeof *t);
                if (q) std::memset(q, 0, sizeof *q);
            }
        }
        if (ids)
            for (size_t i = 0; i < dhw; ++i) ids[(size_t)k * dhw + i] = !set[i] ? 0 : rank_of[lab[i]] < cap ? 1 + rank_of[lab[i]] : -1;
        if (stats) stats[k] = st;
        if (rounds) rounds[k] = 0;
    }
    return MI_UNET_OK;
}

int mi_unet_volume_split_derive(const mi_unet_vpiece *p, const double spacing_xyz[3], double unit_mm, mi_unet_vpiece_metrics *out)
{
    if (!p || !spacing_xyz || !out) return fail(MI_UNET_EARG, "mi_unet_volume_split_derive: null argument");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing_xyz[a]) || !(spacing_xyz[a] > 0.0))
            return fail(MI_UNET_EARG, "mi_unet_volume_split_derive: the spacing must be finite and positive");
    if (!std::isfinite(unit_mm) || !(unit_mm > 0.0)) return fail(MI_UNET_EARG, "mi_unet_volume_split_derive: unit_mm must be finite and positive");
    const double sx = spacing_xyz[0], sy = spacing_xyz[1], sz = spacing_xyz[2];
    out->reach_mm = (double)p->reach * unit_mm;
    out->cut_mm2 = (double)p->cut_x * sy * sz + (double)p->cut_y * sx * sz + (double)p->cut_z * sx * sy;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_split(mi_unet_t *h, const uint8_t *masks, int D, int H, int W, const int *values, int n, const int spacing_units[3],
                         const mi_unet_vsplit_opts *opts, int32_t *ids, mi_unet_vcomp *table, mi_unet_vpiece *info, int cap, int32_t *found,
                         mi_unet_vsplit_stat *stats, int32_t *rounds)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vsplit_opts o = opts ? *opts : kDefaultSplitOpts;
    if (int rc = check_split_args("mi_unet_volume_split", masks, D, H, W, values, n, spacing_units, o, table, cap, found)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, N = dhw * n;
    const size_t table_bytes = (size_t)n * cap * sizeof(mi_unet_vcomp), info_bytes = (size_t)n * cap * sizeof(mi_unet_vpiece);
    // device and pinned alike: the volume, ids (when asked for), the table, the info, the plane results, the activity of a batch of
    // rounds; device only: the kernels' workspace
    Layout c;
    c.take(dhw);
    const size_t at_ids = c.take(ids ? N * sizeof(int32_t) : 0), at_table = c.take(table_bytes), at_info = c.take(info_bytes);
    const size_t at_res = c.take((size_t)n * sizeof(VolumeSplitResult));
    const size_t at_act = c.take((size_t)VSPLIT_BATCH * n * sizeof(unsigned)), at_ws = c.end;
    const size_t dev_need = at_ws + volume_split_workspace_bytes(D, H, W, n), host_need = at_ws;
    hipStream_t s = h->stream;
    if (int rc = h->ws_vsplit.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vsplit.d, *const p = h->ws_vsplit.p;
    host_copy(h, p, masks, dhw);
    HIP_TRY(hipMemcpyAsync(d, p, dhw, hipMemcpyHostToDevice, s));
    VolumeSplitArgs a;
    a.D = D; a.H = H; a.W = W; a.n = n; a.cap = cap;
    a.ux = spacing_units[0]; a.uy = spacing_units[1]; a.uz = spacing_units[2];
    a.connectivity = o.connectivity; a.neck_r = o.neck_r; a.min_core = o.min_core;
    for (int k = 0; k < n; ++k) a.v[k] = values[k];
    hipError_t e = launch_volume_split_seed(d, a, d + at_ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume split launch: ") + hipGetErrorString(e));
    // The growth: VSPLIT_BATCH rounds are queued at a time, then the host reads how many tiles ran in each of them.  A round in which
    // none ran ends the growth (every later round of the batch found nothing to do either).
    unsigned *const d_act = reinterpret_cast<unsigned *>(d + at_act);
    const unsigned *const p_act = reinterpret_cast<const unsigned *>(p + at_act);
    std::vector<int32_t> plane_rounds(n, 0);
    for (int base = 0;; base += VSPLIT_BATCH) {
        HIP_TRY(hipMemsetAsync(d_act, 0, (size_t)VSPLIT_BATCH * n * sizeof(unsigned), s));
        for (int r = 0; r < VSPLIT_BATCH; ++r) {
            e = launch_volume_split_round(d, a, d + at_ws, base + r, d_act + (size_t)r * n, s);
            if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume split launch: ") + hipGetErrorString(e));
        }
        HIP_TRY(hipMemcpyAsync(p + at_act, d_act, (size_t)VSPLIT_BATCH * n * sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        bool idle = false;
        for (int r = 0; r < VSPLIT_BATCH && !idle; ++r) {
            idle = true;
            for (int k = 0; k < n; ++k)
                if (p_act[(size_t)r * n + k]) { plane_rounds[k] = base + r + 1; idle = false; }
        }
        if (idle) break;
    }
    e = launch_volume_split_finish(d, a, ids ? reinterpret_cast<int32_t *>(d + at_ids) : nullptr, reinterpret_cast<mi_unet_vcomp *>(d + at_table),
                                   reinterpret_cast<mi_unet_vpiece *>(d + at_info), reinterpret_cast<VolumeSplitResult *>(d + at_res),
                                   d + at_ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume split launch: ") + hipGetErrorString(e));
    if (ids) HIP_TRY(hipMemcpyAsync(p + at_ids, d + at_ids, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p + at_table, d + at_table, at_act - at_table, hipMemcpyDeviceToHost, s));      // the table, the info, the results
    HIP_TRY(hipStreamSynchronize(s));
    const VolumeSplitResult *const res = reinterpret_cast<const VolumeSplitResult *>(p + at_res);
    for (int k = 0; k < n; ++k)                                 // (a plane with more roots than slots: impossible, see volume.hip)
        if (res[k].found < 0) return fail(MI_UNET_EHIP, "mi_unet_volume_split: the slot table overflowed");
    if (ids) host_copy(h, ids, p + at_ids, N * sizeof(int32_t));
    memcpy(table, p + at_table, table_bytes);
    if (info) memcpy(info, p + at_info, info_bytes);
    for (int k = 0; k < n; ++k) {
        found[k] = res[k].found;
        if (stats)
            stats[k] = mi_unet_vsplit_stat{ values[k], res[k].in_voxels, res[k].core_voxels, res[k].cores, res[k].cores_kept, res[k].found,
                                            res[k].coreless, res[k].max_reach };
        if (rounds) rounds[k] = plane_rounds[k];
    }
    return MI_UNET_OK;
}
#endif

}  // extern "C"
