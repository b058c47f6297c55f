// volume_skeleton.cpp -- the components of an id stack thinned to medial lines (include/mi_unet.h: mi_unet_volume_skeleton; DESIGN.md
// 7.22): the argument checks, the definition as sequential host arithmetic (mi_unet_volume_skeleton_host: the schedule voxel by voxel,
// the simple-point test as two flood fills over adjacency lists built from the offsets), the derived metrics
// (mi_unet_volume_skeleton_derive) and the entry point on the handle, which owns the stage's workspace and reads one counter per pass.
// With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h; tests/cpu/volume_skeleton_host_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vskel) == 112, "mi_unet_vskel is 112 bytes without padding");
static_assert(sizeof(mi_unet_vskel_info) == 16, "mi_unet_vskel_info is 16 bytes without padding");

namespace miunet {

namespace {

constexpr mi_unet_vskel_opts kDefaultSkelOpts{ 0, 1 };
constexpr int kMaxSide = MI_UNET_SCORE_VOLUME_MAX_SIDE;

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_skeleton_args(const char *fn, const int32_t *ids, int D, int H, int W, int m, const int *units, const mi_unet_vskel_opts &o,
                        const mi_unet_vskel *table)
{
    const std::string f = fn;
    if (!ids || !units || !table) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_max(f, D, H, W, kMaxSide)) return rc;
    if ((int64_t)D * H * W >= ((int64_t)1 << 31)) return fail(MI_UNET_EARG, f + ": D * H * W must stay below 2^31");    // (< 2^39: no overflow)
    if (m < 1 || m > MI_UNET_VOLUME_MAX_TABLE)
        return fail(MI_UNET_EARG, f + ": " + std::to_string(m) + " components (1 .. " + std::to_string(MI_UNET_VOLUME_MAX_TABLE) + ")");
    if (int rc = check_units_min1(f, units)) return rc;
    // the volume with its layer of "nothing" on every side
    if (!d2_fits(D + 2, H + 2, W + 2, units))
        return fail(MI_UNET_EARG, f + ": the squared diagonal of the wrapped volume in spacing units must stay below 2^31");
    if (o.max_passes < 0) return fail(MI_UNET_EARG, f + ": max_passes " + std::to_string(o.max_passes) + " is negative");
    if (o.radius != 0 && o.radius != 1) return fail(MI_UNET_EARG, f + ": radius " + std::to_string(o.radius) + " is neither 0 nor 1");
    return MI_UNET_OK;
}

int check_simple_args(const char *fn, uint32_t first_word, uint32_t n_words, const uint32_t *bits)
{
    const std::string f = fn;
    if (!bits) return fail(MI_UNET_EARG, f + ": null argument");
    if (n_words < 1 || (uint64_t)first_word + n_words > ((uint64_t)1 << 21))
        return fail(MI_UNET_EARG, f + ": words " + std::to_string(first_word) + " + " + std::to_string(n_words) + " are outside the 2^21 of the 2^26 codes");
    return MI_UNET_OK;
}

// The neighbourhood of the definition: the 26 offsets in raster order, which of them are 26-adjacent to each other, and inside the 18
// neighbours which are 6-adjacent; all built from the offsets themselves.
struct Nbhood {
    int dz[26], dy[26], dx[26];
    uint32_t adj26[26], adj6[26], n18 = 0, faces = 0;
    Nbhood()
    {
        int i = 0;
        for (int z = -1; z <= 1; ++z)
            for (int y = -1; y <= 1; ++y)
                for (int x = -1; x <= 1; ++x)
                    if (z || y || x) { dz[i] = z; dy[i] = y; dx[i] = x; ++i; }
        auto l1 = [&](int a) { return std::abs(dz[a]) + std::abs(dy[a]) + std::abs(dx[a]); };
        for (int a = 0; a < 26; ++a) {
            if (l1(a) <= 2) n18 |= 1u << a;
            if (l1(a) == 1) faces |= 1u << a;
        }
        for (int a = 0; a < 26; ++a) {
            adj26[a] = adj6[a] = 0;
            for (int b = 0; b < 26; ++b) {
                if (a == b) continue;
                const int ez = std::abs(dz[a] - dz[b]), ey = std::abs(dy[a] - dy[b]), ex = std::abs(dx[a] - dx[b]);
                if (std::max(ez, std::max(ey, ex)) <= 1) adj26[a] |= 1u << b;
                if (ez + ey + ex == 1 && l1(a) <= 2 && l1(b) <= 2) adj6[a] |= 1u << b;
            }
        }
    }
};
const Nbhood kNb;

// the bits of `set` reached from `seed` over adj
inline uint32_t flood(uint32_t seed, uint32_t set, const uint32_t *adj)
{
    uint32_t seen = seed, todo = seed;
    while (todo) {
        const int a = __builtin_ctz(todo);
        todo &= todo - 1;
        const uint32_t fresh = adj[a] & set & ~seen;
        seen |= fresh;
        todo |= fresh;
    }
    return seen;
}

enum Refusal { kSimple = 0, kObject = 1, kBackground = 2 };

inline Refusal classify(uint32_t code)
{
    if (!code || flood(code & (0u - code), code, kNb.adj26) != code) return kObject;
    const uint32_t bg = ~code & kNb.n18;
    uint32_t faces = bg & kNb.faces;
    if (!faces) return kBackground;
    return (faces & ~flood(faces & (0u - faces), bg, kNb.adj6)) ? kBackground : kSimple;
}

// one pass of the exact squared distance along an axis (see volume_skeleton.hip): in[] holds the term of the axes before
inline int dist_scan(const int32_t *ids, const int32_t *in, size_t line, size_t stride, int at, int n, int u)
{
    const int32_t L = ids[line + at * stride];
    int best = in[line + at * stride];
    for (int dir = -1; dir <= 1; dir += 2)
        for (int d = 1;; ++d) {
            const int step = d * u * d * u;
            if (step >= best) break;
            const int q = at + dir * d;
            if (q < 0 || q >= n || ids[line + q * stride] != L) { best = step; break; }
            best = std::min(best, step + in[line + q * stride]);
        }
    return best;
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_skeleton_simple_host(uint32_t first_word, uint32_t n_words, uint32_t *bits)
{
    if (int rc = check_simple_args("mi_unet_volume_skeleton_simple_host", first_word, n_words, bits)) return rc;
    for (uint32_t w = 0; w < n_words; ++w) {
        uint32_t r = 0;
        for (uint32_t b = 0; b < 32; ++b) r |= (uint32_t)(classify(((first_word + w) << 5) | b) == kSimple) << b;
        bits[w] = r;
    }
    return MI_UNET_OK;
}

int mi_unet_volume_skeleton_host(const int32_t *ids, int D, int H, int W, int m, const int spacing_units[3], const mi_unet_vskel_opts *opts,
                                 int32_t *out_ids, int32_t *r2, mi_unet_vskel *table, mi_unet_vskel_info *info)
{
    const mi_unet_vskel_opts o = opts ? *opts : kDefaultSkelOpts;
    if (int rc = check_skeleton_args("mi_unet_volume_skeleton_host", ids, D, H, W, m, spacing_units, o, table)) return rc;
    const size_t hw = (size_t)H * W, dhw = (size_t)D * hw;
    const bool want_dist = o.radius || r2;
    std::vector<int32_t> cur(dhw);
    std::vector<mi_unet_vskel> t((size_t)m);
    std::memset(t.data(), 0, t.size() * sizeof(mi_unet_vskel));
    for (size_t i = 0; i < dhw; ++i) {
        cur[i] = ids[i] >= 1 && ids[i] <= m ? ids[i] : 0;
        if (cur[i]) ++t[cur[i] - 1].voxels_in;
    }
    // RADIUS on the input: z, then y, then x
    std::vector<int32_t> dist;
    if (want_dist) {
        std::vector<int32_t> gz(dhw), f(dhw);
        dist.resize(dhw);
        const int ux = spacing_units[0], uy = spacing_units[1], uz = spacing_units[2];
        for (size_t c = 0; c < hw; ++c) {
            int32_t prev = -1;
            int run = 0;
            for (int z = 0; z < D; ++z) {
                const int32_t v = cur[(size_t)z * hw + c];
                run = v == prev ? run + 1 : 1;
                prev = v;
                gz[(size_t)z * hw + c] = run;
            }
            prev = -1;
            for (int z = D - 1; z >= 0; --z) {
                const int32_t v = cur[(size_t)z * hw + c];
                run = v == prev ? run + 1 : 1;
                prev = v;
                const int g = std::min(run, gz[(size_t)z * hw + c]) * uz;
                gz[(size_t)z * hw + c] = g * g;
            }
        }
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (cur[(size_t)z * hw + (size_t)y * W + x]) f[(size_t)z * hw + (size_t)y * W + x] = dist_scan(cur.data(), gz.data(), (size_t)z * hw + x, (size_t)W, y, H, uy);
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x)
                    if (cur[(size_t)z * hw + (size_t)y * W + x]) dist[(size_t)z * hw + (size_t)y * W + x] = dist_scan(cur.data(), f.data(), (size_t)z * hw + (size_t)y * W, 1, x, W, ux);
    }
    // the 26 same-object bits of voxel (z, y, x) with id v in the current state
    auto code_of = [&](int z, int y, int x, int32_t v) {
        uint32_t code = 0;
        for (int b = 0; b < 26; ++b) {
            const int zz = z + kNb.dz[b], yy = y + kNb.dy[b], xx = x + kNb.dx[b];
            if (zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W && cur[(size_t)zz * hw + (size_t)yy * W + xx] == v) code |= 1u << b;
        }
        return code;
    };
    // SCHEDULE
    std::vector<uint8_t> endm(dhw);
    std::vector<int32_t> cand[8];
    int64_t deleted = 0;
    int32_t passes = 0, stable = 0;
    static const int kDir[6][3] = { { -1, 0, 0 }, { 1, 0, 0 }, { 0, -1, 0 }, { 0, 1, 0 }, { 0, 0, -1 }, { 0, 0, 1 } };      // (dz, dy, dx)
    for (;;) {
        int64_t gone = 0;
        for (int z = 0; z < D; ++z)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const size_t i = (size_t)z * hw + (size_t)y * W + x;
                    endm[i] = cur[i] && __builtin_popcount(code_of(z, y, x, cur[i])) == 1;
                }
        for (int d = 0; d < 6; ++d) {
            for (int s = 0; s < 8; ++s) cand[s].clear();
            for (int z = 0; z < D; ++z)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        const size_t i = (size_t)z * hw + (size_t)y * W + x;
                        if (!cur[i]) continue;
                        const int zz = z + kDir[d][0], yy = y + kDir[d][1], xx = x + kDir[d][2];
                        const bool same = zz >= 0 && zz < D && yy >= 0 && yy < H && xx >= 0 && xx < W && cur[(size_t)zz * hw + (size_t)yy * W + xx] == cur[i];
                        if (!same) cand[(x & 1) | (y & 1) << 1 | (z & 1) << 2].push_back((int32_t)i);
                    }
            for (int s = 0; s < 8; ++s)
                for (const int32_t i : cand[s]) {               // (one after the other: within a subfield the order cannot show)
                    if (!cur[i] || endm[i]) continue;
                    const int z = (int)((size_t)i / hw), y = (int)((size_t)i % hw) / W, x = (int)((size_t)i % hw) % W;
                    if (classify(code_of(z, y, x, cur[i])) == kSimple) { cur[i] = 0; ++gone; }
                }
        }
        ++passes;
        deleted += gone;
        stable = gone == 0;
        if (stable || (o.max_passes > 0 && passes >= o.max_passes)) break;
    }
    // the skeleton counted
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const size_t i = (size_t)z * hw + (size_t)y * W + x;
                if (out_ids) out_ids[i] = cur[i];
                if (r2) r2[i] = cur[i] ? dist[i] : 0;
                if (!cur[i]) continue;
                mi_unet_vskel &c = t[cur[i] - 1];
                const uint32_t code = code_of(z, y, x, cur[i]);
                const int nb = __builtin_popcount(code);
                c.ends += nb == 1;
                c.isolated += nb == 0;
                c.junctions += nb >= 3;
                for (int b = 13; b < 26; ++b)                   // a pair from its voxel of the lower index
                    if (code >> b & 1u) ++c.links[std::abs(kNb.dx[b]) + 2 * std::abs(kNb.dy[b]) + 4 * std::abs(kNb.dz[b]) - 1];
                if (o.radius) {
                    c.r2_min = c.voxels ? std::min(c.r2_min, dist[i]) : dist[i];
                    c.r2_max = std::max(c.r2_max, dist[i]);
                    c.r2_sum += dist[i];
                }
                ++c.voxels;
            }
    std::memcpy(table, t.data(), t.size() * sizeof(mi_unet_vskel));
    if (info) *info = mi_unet_vskel_info{ deleted, passes, stable };
    return MI_UNET_OK;
}

int mi_unet_volume_skeleton_derive(const mi_unet_vskel *c, const double spacing_xyz[3], double unit_mm, mi_unet_vskel_metrics *out)
{
    if (!c || !spacing_xyz || !out) return fail(MI_UNET_EARG, "mi_unet_volume_skeleton_derive: null argument");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(spacing_xyz[a]) || !(spacing_xyz[a] > 0.0))
            return fail(MI_UNET_EARG, "mi_unet_volume_skeleton_derive: the spacing must be finite and positive");
    if (!std::isfinite(unit_mm) || !(unit_mm > 0.0)) return fail(MI_UNET_EARG, "mi_unet_volume_skeleton_derive: unit_mm must be finite and positive");
    double length = 0.0;
    int64_t links = 0;
    for (int k = 0; k < 7; ++k) {
        const int cls = k + 1;
        const double ex = (cls & 1) ? spacing_xyz[0] : 0.0, ey = (cls & 2) ? spacing_xyz[1] : 0.0, ez = (cls & 4) ? spacing_xyz[2] : 0.0;
        length += (double)c->links[k] * std::sqrt(ex * ex + ey * ey + ez * ez);
        links += c->links[k];
    }
    out->length_mm = length;
    out->radius_min_mm = std::sqrt((double)c->r2_min) * unit_mm;
    out->radius_max_mm = std::sqrt((double)c->r2_max) * unit_mm;
    out->radius_rms_mm = c->voxels ? std::sqrt((double)c->r2_sum / (double)c->voxels) * unit_mm : 0.0;
    out->loops = c->voxels ? links - c->voxels + 1 : 0;
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_skeleton_simple(mi_unet_t *h, uint32_t first_word, uint32_t n_words, uint32_t *bits)
{
    if (int rc = check_handle(h, false)) return rc;
    if (int rc = check_simple_args("mi_unet_volume_skeleton_simple", first_word, n_words, bits)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t bytes = (size_t)n_words * sizeof(uint32_t);
    hipStream_t s = h->stream;
    if (int rc = h->ws_vskel.reserve(bytes, bytes, s)) return rc;
    hipError_t e = launch_volume_skeleton_simple(first_word, n_words, reinterpret_cast<uint32_t *>(h->ws_vskel.d.get()), s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume skeleton launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(h->ws_vskel.p.get(), h->ws_vskel.d.get(), bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(bits, h->ws_vskel.p.get(), bytes);
    return MI_UNET_OK;
}

int mi_unet_volume_skeleton(mi_unet_t *h, const int32_t *ids, int D, int H, int W, int m, const int spacing_units[3],
                            const mi_unet_vskel_opts *opts, int32_t *out_ids, int32_t *r2, mi_unet_vskel *table, mi_unet_vskel_info *info)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_vskel_opts o = opts ? *opts : kDefaultSkelOpts;
    if (int rc = check_skeleton_args("mi_unet_volume_skeleton", ids, D, H, W, m, spacing_units, o, table)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, table_bytes = (size_t)m * sizeof(mi_unet_vskel);
    const bool want_dist = o.radius || r2;
    // device and pinned alike: the ids (the state, then the skeleton), r2 (when asked for), the table, the pass state; device only: the
    // kernels' workspace
    Layout c;
    c.take(dhw * sizeof(int32_t));
    const size_t at_r2 = c.take(r2 ? dhw * sizeof(int32_t) : 0), at_table = c.take(table_bytes), at_pass = c.take(sizeof(VskPass)), at_ws = c.end;
    const size_t dev_need = at_ws + volume_skeleton_workspace_bytes(D, H, W), host_need = at_ws;
    hipStream_t s = h->stream;
    if (int rc = h->ws_vskel.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vskel.d.get(), *const p = h->ws_vskel.p.get();
    int32_t *const d_cur = reinterpret_cast<int32_t *>(d);
    mi_unet_vskel *const d_table = reinterpret_cast<mi_unet_vskel *>(d + at_table);
    VskPass *const d_pass = reinterpret_cast<VskPass *>(d + at_pass);
    host_copy(h, p, ids, dhw * sizeof(int32_t));
    HIP_TRY(hipMemcpyAsync(d, p, dhw * sizeof(int32_t), hipMemcpyHostToDevice, s));
    VolumeSkeletonArgs a;
    a.D = D; a.H = H; a.W = W; a.m = m;
    a.ux = spacing_units[0]; a.uy = spacing_units[1]; a.uz = spacing_units[2];
    hipError_t e = launch_volume_skeleton_begin(d_cur, a, want_dist, d_table, d + at_ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume skeleton launch: ") + hipGetErrorString(e));
    // The passes: the host reads what a pass deleted, one word, before it queues the next.  A pass deletes a voxel or is the last, so
    // there are at most D H W + 1 of them.
    const VskPass *const p_pass = reinterpret_cast<const VskPass *>(p + at_pass);
    int64_t deleted = 0;
    int32_t passes = 0, stable = 0;
    for (;;) {
        e = launch_volume_skeleton_pass(d_cur, a, d + at_ws, d_pass, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume skeleton launch: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(p + at_pass, d_pass, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        ++passes;
        deleted += p_pass->deleted;
        stable = p_pass->deleted == 0;
        if (stable || (o.max_passes > 0 && passes >= o.max_passes)) break;
    }
    e = launch_volume_skeleton_finish(d_cur, a, want_dist, o.radius != 0, r2 ? reinterpret_cast<int32_t *>(d + at_r2) : nullptr, d_table, d + at_ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume skeleton launch: ") + hipGetErrorString(e));
    if (out_ids) HIP_TRY(hipMemcpyAsync(p, d, dhw * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r2) HIP_TRY(hipMemcpyAsync(p + at_r2, d + at_r2, dhw * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(p + at_table, d + at_table, table_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (out_ids) host_copy(h, out_ids, p, dhw * sizeof(int32_t));
    if (r2) host_copy(h, r2, p + at_r2, dhw * sizeof(int32_t));
    memcpy(table, p + at_table, table_bytes);
    if (info) *info = mi_unet_vskel_info{ deleted, passes, stable };
    return MI_UNET_OK;
}
#endif

}  // extern "C"
