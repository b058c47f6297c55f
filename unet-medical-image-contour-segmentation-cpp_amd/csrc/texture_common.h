// texture_common.h -- what the host halves of the texture stages share (volume_texture.cpp, volume_zones.cpp, volume_nbhood.cpp;
// DESIGN.md 7.15, 7.17, 7.18): the argument checks they make with the same text, the quantiser that turns ids and intensity into
// keys, the flood over zones of equal key, the 16 features of a level-by-size matrix and, for the device entry points, the fill of
// VolumeTextureArgs and the upload of both stacks.  Header-only: a stand-alone host test compiles one stage file and nothing else.
// The four fields every stage's options begin with -- mode, levels, lo, width -- travel as a mi_unet_vtexture_opts (common_opts).
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>
#include <utility>
#include <vector>

#include "stage_common.h"

namespace miunet {

template <class O>
inline mi_unet_vtexture_opts common_opts(const O &o) { return mi_unet_vtexture_opts{ o.mode, o.levels, o.lo, o.width }; }

// sides, 2^28 voxels, m, mode, levels: in the order every stage's check_*_args has them
inline int check_texture_volume(const std::string &f, int D, int H, int W, int m, const mi_unet_vtexture_opts &o)
{
    if (int rc = check_sides_max(f, D, H, W, MI_UNET_SCORE_VOLUME_MAX_SIDE)) return rc;
    if ((int64_t)D * H * W > (int64_t)MI_UNET_VTEX_MAX_VOXELS) return fail(MI_UNET_EARG, f + ": D * H * W must not pass 2^28");   // (< 2^39: no overflow)
    if (m < 1 || m > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components (1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE) + ")");
    if (o.mode != MI_UNET_VTEX_COUNT && o.mode != MI_UNET_VTEX_WIDTH) return fail(MI_UNET_EARG, f + ": mode " + std::to_string(o.mode) + " does not exist");
    if (o.levels < 2 || o.levels > MI_UNET_VTEX_MAX_LEVELS)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(o.levels) + " levels (2 .. " + std::to_string(MI_UNET_VTEX_MAX_LEVELS) + ")");
    return MI_UNET_OK;
}

// width, then lo: behind a stage's own cells check
inline int check_texture_bins(const std::string &f, const mi_unet_vtexture_opts &o)
{
    if (o.width < 1 || o.width > 65536) return fail(MI_UNET_EARG, f + ": width " + std::to_string(o.width) + " is outside 1 .. 65536");
    if (o.lo < 0 || o.lo > 65535) return fail(MI_UNET_EARG, f + ": lo " + std::to_string(o.lo) + " is outside 0 .. 65535");
    return MI_UNET_OK;
}

// what the functions that derive features ask of a component and its levels
inline int check_texture_component(const std::string &f, int voxels, int L)
{
    if (voxels < 1) return fail(MI_UNET_EARG, f + ": voxels " + std::to_string(voxels) + " (a component has at least one voxel)");
    if (L < 2 || L > MI_UNET_VTEX_MAX_LEVELS) return fail(MI_UNET_EARG, f + ": " + std::to_string(L) + " levels (2 .. " + std::to_string(MI_UNET_VTEX_MAX_LEVELS) + ")");
    return MI_UNET_OK;
}

// The quantiser: voxels, imin and imax of the components 1 .. m into `t` (a stage's zeroed table; all three begin with these fields), and
// per voxel key = id << 8 | level, 0 outside the components.
template <class T>
inline std::vector<int32_t> texture_keys(const int32_t *ids, const uint16_t *intensity, size_t dhw, const mi_unet_vtexture_opts &o, std::vector<T> &t)
{
    const int32_t m = (int32_t)t.size(), L = o.levels;
    auto member = [&](int32_t id) { return id >= 1 && id <= m; };
    for (size_t i = 0; i < dhw; ++i) {
        if (!member(ids[i])) continue;
        T &c = t[ids[i] - 1];
        const int32_t v = intensity[i];
        c.imin = c.voxels ? std::min(c.imin, v) : v;
        c.imax = c.voxels ? std::max(c.imax, v) : v;
        ++c.voxels;
    }
    std::vector<int32_t> key(dhw, 0);
    for (size_t i = 0; i < dhw; ++i) {
        if (!member(ids[i])) continue;
        const T &c = t[ids[i] - 1];
        const int32_t v = intensity[i];
        int32_t l;
        if (o.mode == MI_UNET_VTEX_COUNT) l = ((v - c.imin) * L) / (c.imax - c.imin + 1);
        else l = v < o.lo ? 0 : std::min(L - 1, (v - o.lo) / o.width);
        key[i] = (ids[i] << 8) | l;
    }
    return key;
}

// The zones of a key stack -- 26-connected voxels of one key -- in raster order of their first voxels: zone(first, key, members)
template <class F>
inline void for_each_zone(const std::vector<int32_t> &key, int D, int H, int W, F &&zone)
{
    // the first voxel of a zone that has not been seen opens it; the zone is flooded from there
    std::vector<uint8_t> seen(key.size(), 0);
    std::vector<int32_t> todo, members;
    for (size_t i = 0; i < key.size(); ++i) {
        const int32_t k = key[i];
        if (!k || seen[i]) continue;
        seen[i] = 1;
        todo.assign(1, (int32_t)i);
        members.clear();
        while (!todo.empty()) {
            const int32_t p = todo.back();
            todo.pop_back();
            members.push_back(p);
            const int px = p % W, py = (p / W) % H, pz = p / (W * H);
            for (int dz = -1; dz <= 1; ++dz)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (px + dx < 0 || px + dx >= W || py + dy < 0 || py + dy >= H || pz + dz < 0 || pz + dz >= D) continue;
                        const int32_t q = p + (dz * H + dy) * W + dx;
                        if (key[(size_t)q] != k || seen[(size_t)q]) continue;
                        seen[(size_t)q] = 1;
                        todo.push_back(q);
                    }
        }
        zone((int32_t)i, k, members);
    }
}

struct Cell {
    int64_t i, j, c;            // level + 1; run length, zone size, dependence or zone distance; count
};

// the non-zero cells of one component's L x cols table, sorted by (i, j); none for a table that was not asked for
inline std::vector<Cell> cells_of(const uint32_t *row, int L, int cols)
{
    std::vector<Cell> cells;
    if (!row) return cells;
    for (int l = 0; l < L; ++l)
        for (int j = 0; j < cols; ++j)
            if (const uint32_t v = row[(size_t)l * cols + j]) cells.push_back(Cell{ l + 1, j + 1, (int64_t)v });
    return cells;
}

// the 16 features of mi_unet_vzone_features (the formulas of the 7.17 block of the header, in its order of summation) over the non-zero
// cells of one matrix, sorted by (i, j); `space` = voxels * directions; `energy`, where given, receives sum p^2
inline void matrix_features(const std::vector<Cell> &cells, int L, double space, mi_unet_vzone_features *out, double *energy)
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
        if (energy) *energy = nan;
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
    double sl = 0.0, sh = 0.0, ll = 0.0, lh = 0.0, gv = 0.0, sv = 0.0, ent = 0.0, en = 0.0;
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
        en += p * p;
    }
    o.short_emphasis = se / n; o.long_emphasis = le / n; o.low_grey_emphasis = lg / n; o.high_grey_emphasis = hg / n;
    o.short_low = sl / n; o.short_high = sh / n; o.long_low = ll / n; o.long_high = lh / n;
    o.grey_nonuniformity = gn / n; o.grey_nonuniformity_norm = gn / n / n;
    o.size_nonuniformity = sn / n; o.size_nonuniformity_norm = sn / n / n;
    o.percentage = n / space;
    o.grey_variance = gv; o.size_variance = sv; o.entropy = ent;
    *out = o;
    if (energy) *energy = en;
}

#ifndef MIUNET_NO_DEVICE
inline VolumeTextureArgs texture_args(int D, int H, int W, int m, const mi_unet_vtexture_opts &o)
{
    VolumeTextureArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m; a.mode = o.mode; a.L = o.levels; a.lo = o.lo; a.width = o.width;
    return a;
}

// ids and intensity of `dhw` voxels through the pinned side of `ws` to its device side, at the same two offsets on both
inline int upload_stacks(mi_unet *h, Workspace &ws, size_t at_ids, const int32_t *ids, size_t at_int, const uint16_t *intensity, size_t dhw)
{
    host_copy(h, ws.p.get() + at_ids, ids, dhw * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(ws.d.get() + at_ids, ws.p.get() + at_ids, dhw * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    host_copy(h, ws.p.get() + at_int, intensity, dhw * sizeof(uint16_t));
    HIP_TRY(hipMemcpyAsync(ws.d.get() + at_int, ws.p.get() + at_int, dhw * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    return MI_UNET_OK;
}
#endif

}  // namespace miunet
