// volume_branches.cpp -- a skeleton split into nodes and branches, short spurs pruned (include/mi_unet.h: mi_unet_volume_branches;
// DESIGN.md 7.23): the argument checks, the definition as sequential host arithmetic (mi_unet_volume_branches_host: classes by counting
// neighbours, clusters and branches by flood fills started in raster order, so a set is met at its lowest voxel, then the rows voxel
// by voxel, and the pruning rounds on top), the derived metrics (mi_unet_volume_branches_derive_branch, mi_unet_volume_branches_derive)
// and the entry point on the handle, which owns the stage's workspace and reads one word per round.
// With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h; tests/cpu/volume_branches_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vbranch) == 88, "mi_unet_vbranch is 88 bytes without padding");
static_assert(sizeof(mi_unet_vnode) == 56, "mi_unet_vnode is 56 bytes without padding");
static_assert(sizeof(mi_unet_vgraph) == 128, "mi_unet_vgraph is 128 bytes without padding");
static_assert(sizeof(mi_unet_vbranch_info) == 24, "mi_unet_vbranch_info is 24 bytes without padding");

namespace miunet {

namespace {

constexpr mi_unet_vbranch_opts kDefaultBranchOpts{ 0, 0 };
constexpr int kMaxSide = MI_UNET_SCORE_VOLUME_MAX_SIDE;

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_branches_args(const char *fn, const int32_t *ids, int D, int H, int W, int m, const int *units, const mi_unet_vbranch_opts &o,
                        const mi_unet_vnode *nodes, int cap_nodes, const mi_unet_vbranch *branches, int cap_branches, const mi_unet_vgraph *graph)
{
    const std::string f = fn;
    if (!ids || !units || !graph) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_max(f, D, H, W, kMaxSide)) return rc;
    if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return fail(MI_UNET_EARG, f + ": D * H * W must stay below 2^31");    // (< 2^39: no overflow)
    if (m < 1 || m > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components (1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE) + ")");
    if (int rc = check_units_min1(f, units)) return rc;
    if (!d2_fits(D + 2, H + 2, W + 2, units))
        return fail(MI_UNET_EARG, f + ": the squared diagonal of the wrapped volume in spacing units must stay below 2^31");
    if (cap_nodes < 0 || cap_nodes > MI_UNET_VBRANCH_MAX_ROWS || cap_branches < 0 || cap_branches > MI_UNET_VBRANCH_MAX_ROWS)
        return fail(MI_UNET_EARG, f + ": caps " + std::to_string(cap_nodes) + ", " + std::to_string(cap_branches) + " (0 .. " +
                                      std::to_string(MI_UNET_VBRANCH_MAX_ROWS) + ")");
    if ((cap_nodes > 0 && !nodes) || (cap_branches > 0 && !branches)) return fail(MI_UNET_EARG, f + ": a null table with a cap above 0");
    if (o.prune_voxels < 0 || o.prune_voxels > MI_UNET_VBRANCH_MAX_PRUNE || o.prune_rounds < 0 || o.prune_rounds > MI_UNET_VBRANCH_MAX_PRUNE)
        return fail(MI_UNET_EARG, f + ": prune " + std::to_string(o.prune_voxels) + ", rounds " + std::to_string(o.prune_rounds) + " (0 .. " +
                                      std::to_string(MI_UNET_VBRANCH_MAX_PRUNE) + ")");
    return MI_UNET_OK;
}

int check_spacing(const std::string &f, const double *spacing_xyz, double unit_mm)
{
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing_xyz[a]) || !(spacing_xyz[a] > 0.0)) return fail(MI_UNET_EARG, f + ": the spacing must be finite and positive");
    if (!std::isfinite(unit_mm) || !(unit_mm > 0.0)) return fail(MI_UNET_EARG, f + ": unit_mm must be finite and positive");
    return MI_UNET_OK;
}

template <class T>
double length_of(const T *links, const double *spacing_xyz)
{
    double length = 0.0;
    for (int k = 0; k < 7; ++k) {
        const int cls = k + 1;
        const double ex = (cls & 1) ? spacing_xyz[0] : 0.0, ey = (cls & 2) ? spacing_xyz[1] : 0.0, ez = (cls & 4) ? spacing_xyz[2] : 0.0;
        length += (double)links[k] * std::sqrt(ex * ex + ey * ey + ez * ez);
    }
    return length;
}

enum : uint8_t { kNone = 0, kIsolated = 1, kEnd = 2, kBranch = 3, kJunction = 4 };

// The graph of one state, by the definition.  node_of / branch_of: per voxel the rank of its node / branch, or -1.
struct HostGraph {
    int D, H, W;
    size_t hw;
    const int32_t *cur, *r2;
    std::vector<uint8_t> cls;
    std::vector<int32_t> node_of, branch_of;
    std::vector<mi_unet_vnode> nodes;
    std::vector<mi_unet_vbranch> branches;

    // f(q, link class) for every same-object neighbour q of voxel i
    template <class F>
    void neighbours(size_t i, F f) const
    {
        const int z = (int)(i / hw), y = (int)(i % hw) / W, x = (int)(i % hw) % W;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!dz && !dy && !dx) continue;
                    const int zz = z + dz, yy = y + dy, xx = x + dx;
                    if (zz < 0 || zz >= D || yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    const size_t q = (size_t)zz * hw + (size_t)yy * W + xx;
                    if (cur[q] == cur[i]) f(q, std::abs(dx) + 2 * std::abs(dy) + 4 * std::abs(dz) - 1);
                }
    }

    // the 26-connected set of voxels of i's id and class that holds i, i first
    std::vector<size_t> flood(size_t i, std::vector<int32_t> &mark, int32_t rank) const
    {
        std::vector<size_t> set{ i };
        mark[i] = rank;
        for (size_t at = 0; at < set.size(); ++at)
            neighbours(set[at], [&](size_t q, int) {
                if (cls[q] == cls[i] && mark[q] < 0) { mark[q] = rank; set.push_back(q); }
            });
        return set;
    }

    void build(const int32_t *state, const int32_t *radius, int d, int h, int w)
    {
        D = d; H = h; W = w; hw = (size_t)h * w; cur = state; r2 = radius;
        const size_t dhw = (size_t)D * hw;
        cls.assign(dhw, kNone);
        node_of.assign(dhw, -1);
        branch_of.assign(dhw, -1);
        nodes.clear();
        branches.clear();
        for (size_t i = 0; i < dhw; ++i) {
            if (!cur[i]) continue;
            int deg = 0;
            neighbours(i, [&](size_t, int) { ++deg; });
            cls[i] = deg == 0 ? kIsolated : deg == 1 ? kEnd : deg == 2 ? kBranch : kJunction;
        }
        // NODES, in raster order: a cluster is met at its lowest voxel
        for (size_t i = 0; i < dhw; ++i) {
            if (cls[i] == kNone || cls[i] == kBranch || node_of[i] >= 0) continue;
            mi_unet_vnode n{};
            n.first = (int64_t)i; n.id = cur[i]; n.kind = cls[i] == kIsolated ? 0 : cls[i] == kEnd ? 1 : 2;
            const int32_t rank = (int32_t)nodes.size();
            std::vector<size_t> set;
            if (cls[i] == kJunction) set = flood(i, node_of, rank);
            else { set.push_back(i); node_of[i] = rank; }
            for (const size_t p : set) {
                n.sz += (int64_t)(p / hw); n.sy += (int64_t)((p % hw) / W); n.sx += (int64_t)((p % hw) % W);
                if (r2) {
                    n.r2_min = n.voxels ? std::min(n.r2_min, r2[p]) : r2[p];
                    n.r2_max = n.voxels ? std::max(n.r2_max, r2[p]) : r2[p];
                }
                ++n.voxels;
            }
            nodes.push_back(n);
        }
        // BRANCHES, in raster order of their keys
        for (size_t i = 0; i < dhw; ++i) {
            if (cls[i] == kBranch && branch_of[i] < 0) {
                mi_unet_vbranch b{};
                b.first = (int64_t)i; b.id = cur[i];
                std::vector<size_t> att;
                for (const size_t p : flood(i, branch_of, (int32_t)branches.size())) {
                    if (r2) {
                        b.r2_min = b.voxels ? std::min(b.r2_min, r2[p]) : r2[p];
                        b.r2_max = b.voxels ? std::max(b.r2_max, r2[p]) : r2[p];
                        b.r2_sum += r2[p];
                    }
                    ++b.voxels;
                    neighbours(p, [&](size_t q, int c) {
                        if (cls[q] != kBranch) { att.push_back(q); ++b.links[c]; }
                        else if (q > p) ++b.links[c];
                    });
                }
                attach(b, att, 0);
                branches.push_back(b);
            } else if (cls[i] == kEnd) {
                size_t only = 0;
                neighbours(i, [&](size_t q, int) { only = q; });
                if (cls[only] == kJunction || (cls[only] == kEnd && only > i)) {
                    mi_unet_vbranch b{};
                    b.first = (int64_t)i; b.id = cur[i];
                    neighbours(i, [&](size_t, int c) { ++b.links[c]; });
                    attach(b, { i, only }, 2);
                    branches.push_back(b);
                }
            }
        }
    }

    void attach(mi_unet_vbranch &b, const std::vector<size_t> &att, int open_kind)
    {
        if (att.empty()) {
            b.kind = 1; b.att_lo = b.att_hi = -1; b.node_a = b.node_b = -1;
            return;
        }
        b.kind = open_kind;
        b.att_lo = (int64_t)*std::min_element(att.begin(), att.end());
        b.att_hi = (int64_t)*std::max_element(att.begin(), att.end());
        b.node_a = node_of[b.att_lo]; b.node_b = node_of[b.att_hi];
        for (const size_t q : att) ++nodes[node_of[q]].degree;
    }

    bool is_spur(const mi_unet_vbranch &b, int prune_voxels) const
    {
        if (b.kind == 1 || (int64_t)b.voxels + 1 > prune_voxels) return false;
        const int ka = nodes[b.node_a].kind, kb = nodes[b.node_b].kind;
        return (ka == 1 && kb == 2) || (ka == 2 && kb == 1);
    }
};

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_branches_host(const int32_t *ids, const int32_t *r2, int D, int H, int W, int m, const int spacing_units[3],
                                 const mi_unet_vbranch_opts *opts, mi_unet_vnode *nodes, int cap_nodes, mi_unet_vbranch *branches, int cap_branches,
                                 mi_unet_vgraph *graph, int32_t *map, int32_t *out_ids, mi_unet_vbranch_info *info)
{
    const mi_unet_vbranch_opts o = opts ? *opts : kDefaultBranchOpts;
    if (int rc = check_branches_args("mi_unet_volume_branches_host", ids, D, H, W, m, spacing_units, o, nodes, cap_nodes, branches, cap_branches, graph))
        return rc;
    const size_t dhw = (size_t)D * H * W;
    std::vector<int32_t> cur(dhw);
    for (size_t i = 0; i < dhw; ++i) cur[i] = ids[i] >= 1 && ids[i] <= m ? ids[i] : 0;
    std::vector<mi_unet_vgraph> g((size_t)m);
    std::memset(g.data(), 0, g.size() * sizeof(mi_unet_vgraph));
    HostGraph hg;
    int32_t rounds = 0, stable = 0;
    for (;;) {
        hg.build(cur.data(), r2, D, H, W);
        std::vector<int32_t> spurs;
        for (size_t b = 0; b < hg.branches.size(); ++b)
            if (hg.is_spur(hg.branches[b], o.prune_voxels)) spurs.push_back((int32_t)b);
        stable = spurs.empty();
        if (stable || (o.prune_rounds > 0 && rounds >= o.prune_rounds)) break;
        std::vector<uint8_t> dead(hg.branches.size(), 0);
        for (const int32_t b : spurs) {
            const mi_unet_vbranch &row = hg.branches[b];
            dead[b] = 1;
            ++g[row.id - 1].pruned_spurs;
            g[row.id - 1].pruned_voxels += (int64_t)row.voxels + 1;
        }
        std::vector<int32_t> next(cur);
        for (size_t i = 0; i < dhw; ++i)
            if (hg.branch_of[i] >= 0 && dead[hg.branch_of[i]]) next[i] = 0;
        for (const int32_t b : spurs) {                          // the end voxel of the spur
            const mi_unet_vbranch &row = hg.branches[b];
            next[hg.nodes[row.node_a].kind == 1 ? row.att_lo : row.att_hi] = 0;
        }
        cur.swap(next);
        ++rounds;
    }
    for (const mi_unet_vnode &n : hg.nodes) {
        mi_unet_vgraph &r = g[n.id - 1];
        ++r.nodes;
        r.isolated += n.kind == 0; r.ends += n.kind == 1; r.junction_nodes += n.kind == 2;
        if (n.kind == 2) r.junction_voxels += n.voxels;
    }
    for (const mi_unet_vbranch &b : hg.branches) {
        mi_unet_vgraph &r = g[b.id - 1];
        ++r.branches;
        r.closed += b.kind == 1;
        for (int c = 0; c < 7; ++c) r.links[c] += b.links[c];
    }
    const size_t n_nodes = std::min(hg.nodes.size(), (size_t)cap_nodes), n_branches = std::min(hg.branches.size(), (size_t)cap_branches);
    if (n_nodes) std::memcpy(nodes, hg.nodes.data(), n_nodes * sizeof(mi_unet_vnode));
    if (n_branches) std::memcpy(branches, hg.branches.data(), n_branches * sizeof(mi_unet_vbranch));
    std::memcpy(graph, g.data(), g.size() * sizeof(mi_unet_vgraph));
    if (map)
        for (size_t i = 0; i < dhw; ++i) map[i] = hg.branch_of[i] >= 0 ? hg.branch_of[i] + 1 : hg.node_of[i] >= 0 ? -(hg.node_of[i] + 1) : 0;
    if (out_ids) std::memcpy(out_ids, cur.data(), dhw * sizeof(int32_t));
    if (info) *info = mi_unet_vbranch_info{ (int64_t)hg.nodes.size(), (int64_t)hg.branches.size(), rounds, stable };
    return MI_UNET_OK;
}

int mi_unet_volume_branches_derive_branch(const mi_unet_vbranch *row, int H, int W, const double spacing_xyz[3], double unit_mm,
                                          mi_unet_vbranch_metrics *out)
{
    const std::string f = "mi_unet_volume_branches_derive_branch";
    if (!row || !spacing_xyz || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (H < 1 || W < 1) return fail(MI_UNET_EARG, f + ": H and W are at least 1");
    if (int rc = check_spacing(f, spacing_xyz, unit_mm)) return rc;
    out->length_mm = length_of(row->links, spacing_xyz);
    out->chord_mm = 0.0;
    if (row->kind != 1 && row->att_lo >= 0 && row->att_hi >= 0) {
        const int64_t hw = (int64_t)H * W, a = row->att_lo, b = row->att_hi;
        const double ex = (double)(b % hw % W - a % hw % W) * spacing_xyz[0], ey = (double)(b % hw / W - a % hw / W) * spacing_xyz[1],
                     ez = (double)(b / hw - a / hw) * spacing_xyz[2];
        out->chord_mm = std::sqrt(ex * ex + ey * ey + ez * ez);
    }
    out->tortuosity = row->kind != 1 && out->chord_mm > 0.0 ? out->length_mm / out->chord_mm : 0.0;
    out->radius_min_mm = std::sqrt((double)row->r2_min) * unit_mm;
    out->radius_max_mm = std::sqrt((double)row->r2_max) * unit_mm;
    out->radius_rms_mm = row->voxels ? std::sqrt((double)row->r2_sum / (double)row->voxels) * unit_mm : 0.0;
    return MI_UNET_OK;
}

int mi_unet_volume_branches_derive(const mi_unet_vgraph *g, const mi_unet_vbranch *branches, int64_t n_branches, int64_t found_nodes, int id,
                                   const double spacing_xyz[3], double unit_mm, mi_unet_vgraph_metrics *out)
{
    const std::string f = "mi_unet_volume_branches_derive";
    if (!g || !spacing_xyz || !out || (n_branches > 0 && !branches)) return fail(MI_UNET_EARG, f + ": null argument");
    if (n_branches < 0 || found_nodes < 0 || found_nodes > ((int64_t)1 << 31)) return fail(MI_UNET_EARG, f + ": a count out of range");
    if (int rc = check_spacing(f, spacing_xyz, unit_mm)) return rc;
    // the id's graph: every branch that joins two parts makes them one
    std::vector<int32_t> parent((size_t)found_nodes);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int32_t v) {
        while (parent[v] != v) v = parent[v] = parent[parent[v]];
        return v;
    };
    int64_t rows = 0, joined = 0;
    for (int64_t b = 0; b < n_branches; ++b) {
        const mi_unet_vbranch &r = branches[b];
        if (r.id != id) continue;
        ++rows;
        if (r.kind == 1) continue;
        if (r.node_a < 0 || r.node_b < 0 || r.node_a >= found_nodes || r.node_b >= found_nodes)
            return fail(MI_UNET_EARG, f + ": a branch names a node outside 0 .. found_nodes - 1");
        const int32_t a = find(r.node_a), c = find(r.node_b);
        if (a != c) { parent[std::max(a, c)] = std::min(a, c); ++joined; }
    }
    if (rows < g->branches)
        return fail(MI_UNET_EARG, f + ": the table holds " + std::to_string(rows) + " of the id's " + std::to_string(g->branches) + " branches (truncated)");
    out->length_mm = length_of(g->links, spacing_xyz);
    out->parts = g->nodes - joined + g->closed;
    out->loops = g->branches - g->nodes - g->closed + out->parts;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_branches(mi_unet_t *h, const int32_t *ids, const int32_t *r2, int D, int H, int W, int m, const int spacing_units[3],
                            const mi_unet_vbranch_opts *opts, mi_unet_vnode *nodes, int cap_nodes, mi_unet_vbranch *branches, int cap_branches,
                            mi_unet_vgraph *graph, int32_t *map, int32_t *out_ids, mi_unet_vbranch_info *info)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vbranch_opts o = opts ? *opts : kDefaultBranchOpts;
    if (int rc = check_branches_args("mi_unet_volume_branches", ids, D, H, W, m, spacing_units, o, nodes, cap_nodes, branches, cap_branches, graph))
        return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, vol_bytes = dhw * sizeof(int32_t), graph_bytes = (size_t)m * sizeof(mi_unet_vgraph);
    // a state has no more nodes and no more branches than voxels
    const size_t rows_n = std::min<size_t>((size_t)cap_nodes, dhw), rows_b = std::min<size_t>((size_t)cap_branches, dhw);
    // device and pinned alike: the ids (the state), r2, the map, both tables, the per-id table, the round's words; device only: the
    // kernels' workspace
    Layout c;
    c.take(vol_bytes);
    const size_t at_r2 = c.take(r2 ? vol_bytes : 0), at_map = c.take(map ? vol_bytes : 0), at_nodes = c.take(rows_n * sizeof(mi_unet_vnode)),
                 at_branches = c.take(rows_b * sizeof(mi_unet_vbranch)), at_graph = c.take(graph_bytes), at_state = c.take(sizeof(VbrState)),
                 at_ws = c.end;
    const size_t dev_need = at_ws + volume_branches_workspace_bytes(D, H, W), host_need = at_ws;
    hipStream_t s = h->stream;
    if (int rc = h->ws_vbranch.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vbranch.d.get(), *const p = h->ws_vbranch.p.get();
    int32_t *const d_cur = reinterpret_cast<int32_t *>(d);
    const int32_t *const d_r2 = r2 ? reinterpret_cast<const int32_t *>(d + at_r2) : nullptr;
    VbrState *const d_state = reinterpret_cast<VbrState *>(d + at_state);
    const VbrState *const p_state = reinterpret_cast<const VbrState *>(p + at_state);
    host_copy(h, p, ids, vol_bytes);
    HIP_TRY(hipMemcpyAsync(d, p, vol_bytes, hipMemcpyHostToDevice, s));
    if (r2) {
        host_copy(h, p + at_r2, r2, vol_bytes);
        HIP_TRY(hipMemcpyAsync(d + at_r2, p + at_r2, vol_bytes, hipMemcpyHostToDevice, s));
    }
    VolumeBranchesArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m; a.prune_voxels = o.prune_voxels;
    auto launched = [&](hipError_t e) { return e == hipSuccess ? MI_UNET_OK : fail(MI_UNET_EHIP, std::string("volume branches launch: ") + hipGetErrorString(e)); };
    mi_unet_vgraph *const d_graph = reinterpret_cast<mi_unet_vgraph *>(d + at_graph);
    if (int rc = launched(launch_volume_branches_begin(d_cur, a, d_graph, d_state, d + at_ws, s))) return rc;
    // The rounds: the host reads how many spurs the state's graph holds, one word, before it queues the deletion and the next round.  A
    // round that deletes takes at least one voxel, so there are at most D H W of them.
    int32_t rounds = 0, stable = 0;
    for (;;) {
        if (int rc = launched(launch_volume_branches_round(d_cur, a, rounds == 0, d_state, d + at_ws, s))) return rc;
        HIP_TRY(hipMemcpyAsync(p + at_state, d_state, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        stable = p_state->spurs == 0;
        if (stable || (o.prune_rounds > 0 && rounds >= o.prune_rounds)) break;
        if (int rc = launched(launch_volume_branches_delete(d_cur, a, d_graph, d_state, d + at_ws, s))) return rc;
        ++rounds;
    }
    // the final state's graph: numbered, then the host learns how many rows there are
    if (int rc = launched(launch_volume_branches_number(d_cur, a, d_state, d + at_ws, s))) return rc;
    HIP_TRY(hipMemcpyAsync(p + at_state, d_state, sizeof(VbrState), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const size_t found_n = p_state->found_nodes, found_b = p_state->found_branches;
    const size_t n_nodes = std::min(found_n, (size_t)cap_nodes), n_branches = std::min(found_b, (size_t)cap_branches);
    if (int rc = launched(launch_volume_branches_rows(d_cur, d_r2, a, reinterpret_cast<mi_unet_vnode *>(d + at_nodes), (int)n_nodes,
                                                      reinterpret_cast<mi_unet_vbranch *>(d + at_branches), (int)n_branches, d_graph,
                                                      map ? reinterpret_cast<int32_t *>(d + at_map) : nullptr, d_state, d + at_ws, s)))
        return rc;
    if (out_ids) HIP_TRY(hipMemcpyAsync(p, d, vol_bytes, hipMemcpyDeviceToHost, s));
    if (map) HIP_TRY(hipMemcpyAsync(p + at_map, d + at_map, vol_bytes, hipMemcpyDeviceToHost, s));
    if (n_nodes) HIP_TRY(hipMemcpyAsync(p + at_nodes, d + at_nodes, n_nodes * sizeof(mi_unet_vnode), hipMemcpyDeviceToHost, s));
    if (n_branches) HIP_TRY(hipMemcpyAsync(p + at_branches, d + at_branches, n_branches * sizeof(mi_unet_vbranch), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p + at_graph, d + at_graph, graph_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out_ids) host_copy(h, out_ids, p, vol_bytes);
    if (map) host_copy(h, map, p + at_map, vol_bytes);
    if (n_nodes) memcpy(nodes, p + at_nodes, n_nodes * sizeof(mi_unet_vnode));
    if (n_branches) memcpy(branches, p + at_branches, n_branches * sizeof(mi_unet_vbranch));
    memcpy(graph, p + at_graph, graph_bytes);
    if (info) *info = mi_unet_vbranch_info{ (int64_t)found_n, (int64_t)found_b, rounds, stable };
    return MI_UNET_OK;
}
#endif

}  // extern "C"
