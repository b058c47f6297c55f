// volume_clean.cpp -- a stack of masks cleaned as one volume (include/mi_unet.h: mi_unet_volume_clean): the argument
// checks, the ball (mi_unet_volume_ball), the definition as sequential host arithmetic (mi_unet_volume_clean_host) and the entry point
// on the handle, which owns the stage's workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h;
// tests/cpu/volume_clean_host_test.cpp).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_volume_clean_stat) == 48, "mi_unet_volume_clean_stat is 48 bytes without padding");

namespace miunet {

namespace {

constexpr mi_unet_volume_clean_opts kDefaultCleanOpts{ 1, 0, 0 };
constexpr int kMaxR = MI_UNET_VOLUME_CLEAN_MAX_R;

int check_units(const std::string &f, const int *units)
{
    for (int a = 0; a < 3; ++a)
        if (units[a] < 1 || units[a] > kMaxR)
            return fail(MI_UNET_EARG, f + ": spacing unit " + std::to_string(units[a]) + " is outside 1 .. " + std::to_string(kMaxR));
    return MI_UNET_OK;
}

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails
int check_clean_args(const char *fn, const uint8_t *masks, int D, int H, int W, const int *values, int n, const int *units,
                     const mi_unet_volume_clean_opts &o, const uint8_t *out)
{
    const std::string f = fn;
    if (!masks || !values || !units || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_sides_min1(f, D, H, W)) return rc;
    if (int rc = check_values(f, values, n, MI_UNET_VOLUME_MAX_VALUES)) return rc;
    if (!product_below_2_31(n, D, H, W)) return fail(MI_UNET_EARG, f + ": n * D * H * W must stay below 2^31");
    if (int rc = check_units(f, units)) return rc;
    if (o.fill != 0 && o.fill != 1) return fail(MI_UNET_EARG, f + ": fill " + std::to_string(o.fill) + " is neither 0 nor 1");
    if (o.close_r < 0 || o.close_r > kMaxR)
        return fail(MI_UNET_EARG, f + ": close_r " + std::to_string(o.close_r) + " is outside 0 .. " + std::to_string(kMaxR));
    if (o.open_r < 0 || o.open_r > kMaxR)
        return fail(MI_UNET_EARG, f + ": open_r " + std::to_string(o.open_r) + " is outside 0 .. " + std::to_string(kMaxR));
    if (out == masks && n > 1) return fail(MI_UNET_EARG, f + ": out may be masks only with one value");
    return MI_UNET_OK;
}

bool single_voxel(const int *units, int r) { return r / units[0] == 0 && r / units[1] == 0 && r / units[2] == 0; }

mi_unet_volume_clean_stat make_stat(int value, int64_t c_in, int64_t c_fill, int64_t c_close, int64_t c_open)
{
    mi_unet_volume_clean_stat s;
    s.value = value; s.reserved = 0;
    s.in_voxels = c_in; s.filled = c_fill - c_in; s.closed = c_close - c_fill; s.opened = c_close - c_open; s.out_voxels = c_open;
    return s;
}

struct Shape { int D, H, W; };

// The voxels not in `set` that no 6-connected path through such voxels joins to a face of the volume are added to it: a flood of the
// complement from the faces, then everything the flood did not reach.
void fill_cavities(std::vector<uint8_t> &set, Shape sh)
{
    const int D = sh.D, H = sh.H, W = sh.W;
    const size_t hw = (size_t)H * W;
    std::vector<uint8_t> outside(set.size(), 0);
    std::vector<int32_t> stack;
    auto push = [&](int z, int y, int x) {
        const size_t i = (size_t)z * hw + (size_t)y * W + x;
        if (set[i] || outside[i]) return;
        outside[i] = 1;
        stack.push_back((int32_t)i);
    };
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                if (z == 0 || z == D - 1 || y == 0 || y == H - 1 || x == 0 || x == W - 1) push(z, y, x);
    while (!stack.empty()) {
        const int32_t i = stack.back();
        stack.pop_back();
        const int z = (int)((size_t)i / hw), y = (int)((size_t)i % hw) / W, x = (int)((size_t)i % hw) % W;
        if (z > 0) push(z - 1, y, x);
        if (z + 1 < D) push(z + 1, y, x);
        if (y > 0) push(z, y - 1, x);
        if (y + 1 < H) push(z, y + 1, x);
        if (x > 0) push(z, y, x - 1);
        if (x + 1 < W) push(z, y, x + 1);
    }
    for (size_t i = 0; i < set.size(); ++i) set[i] = set[i] || !outside[i];
}

// One dilation (inv false) or erosion (inv true) of `set` by B(r), in place.  The squared distance of every voxel to the nearest seed
// inside the volume, as far as the ball reaches: the nearest seed of the column, then along y, then along x.  A seed is a voxel of the
// set, or for the erosion a voxel inside the volume that is not in it; the erosion's result is the complement.
void morph(std::vector<uint8_t> &set, Shape sh, const int *units, int r, bool inv)
{
    const int D = sh.D, H = sh.H, W = sh.W;
    const int64_t ux = units[0], uy = units[1], uz = units[2], r2 = (int64_t)r * r, none = r2 + 1;
    const int ex = std::min(r / units[0], W - 1), ey = std::min(r / units[1], H - 1), ez = std::min(r / units[2], D - 1);
    const size_t hw = (size_t)H * W;
    std::vector<int64_t> gz(set.size()), f(set.size());
    for (size_t c = 0; c < hw; ++c)
        for (int z = 0; z < D; ++z) {
            int64_t best = none;
            for (int dz = -ez; dz <= ez; ++dz)
                if (z + dz >= 0 && z + dz < D && (set[(size_t)(z + dz) * hw + c] != 0) != inv) best = std::min(best, dz * uz * dz * uz);
            gz[(size_t)z * hw + c] = best;
        }
    for (int z = 0; z < D; ++z)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int64_t best = none;
                for (int dy = -ey; dy <= ey; ++dy)
                    if (y + dy >= 0 && y + dy < H) best = std::min(best, gz[(size_t)z * hw + (size_t)(y + dy) * W + x] + dy * uy * dy * uy);
                f[(size_t)z * hw + (size_t)y * W + x] = best;
            }
    for (size_t row = 0; row < (size_t)D * H; ++row)
        for (int x = 0; x < W; ++x) {
            int64_t best = none;
            for (int dx = -ex; dx <= ex; ++dx)
                if (x + dx >= 0 && x + dx < W) best = std::min(best, f[row * W + x + dx] + dx * ux * dx * ux);
            set[row * W + x] = (best <= r2) != inv;
        }
}

int64_t count(const std::vector<uint8_t> &set) { return (int64_t)std::count(set.begin(), set.end(), (uint8_t)1); }

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_ball(const int spacing_units[3], int r, int extent[3], uint8_t *elem)
{
    const std::string f = "mi_unet_volume_ball";
    if (!spacing_units || !extent) return fail(MI_UNET_EARG, f + ": null argument");
    if (int rc = check_units(f, spacing_units)) return rc;
    if (r < 0 || r > kMaxR) return fail(MI_UNET_EARG, f + ": r " + std::to_string(r) + " is outside 0 .. " + std::to_string(kMaxR));
    const int e[3] = { r / spacing_units[0], r / spacing_units[1], r / spacing_units[2] };
    for (int a = 0; a < 3; ++a) extent[a] = e[a];
    if (!elem) return MI_UNET_OK;
    const int64_t r2 = (int64_t)r * r;
    size_t at = 0;
    for (int dz = -e[2]; dz <= e[2]; ++dz)
        for (int dy = -e[1]; dy <= e[1]; ++dy)
            for (int dx = -e[0]; dx <= e[0]; ++dx) {
                const int64_t tx = (int64_t)dx * spacing_units[0], ty = (int64_t)dy * spacing_units[1], tz = (int64_t)dz * spacing_units[2];
                elem[at++] = tx * tx + ty * ty + tz * tz <= r2;
            }
    return MI_UNET_OK;
}

int mi_unet_volume_clean_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const int spacing_units[3],
                              const mi_unet_volume_clean_opts *opts, uint8_t *out, mi_unet_volume_clean_stat *stats)
{
    const mi_unet_volume_clean_opts o = opts ? *opts : kDefaultCleanOpts;
    if (int rc = check_clean_args("mi_unet_volume_clean_host", masks, D, H, W, values, n, spacing_units, o, out)) return rc;
    const size_t dhw = (size_t)D * H * W;
    const Shape sh{ D, H, W };
    std::vector<uint8_t> set(dhw);
    for (int k = 0; k < n; ++k) {
        const int v = values[k];
        for (size_t i = 0; i < dhw; ++i) set[i] = masks[i] == v;            // (`out` may be `masks`: then n == 1 and this is the only read)
        const int64_t c_in = count(set);
        if (o.fill) fill_cavities(set, sh);
        const int64_t c_fill = count(set);
        if (!single_voxel(spacing_units, o.close_r)) {
            morph(set, sh, spacing_units, o.close_r, false);
            morph(set, sh, spacing_units, o.close_r, true);
        }
        const int64_t c_close = count(set);
        if (!single_voxel(spacing_units, o.open_r)) {
            morph(set, sh, spacing_units, o.open_r, true);
            morph(set, sh, spacing_units, o.open_r, false);
        }
        const int64_t c_open = count(set);
        for (size_t i = 0; i < dhw; ++i) out[(size_t)k * dhw + i] = set[i] ? (uint8_t)v : 0;
        if (stats) stats[k] = make_stat(v, c_in, c_fill, c_close, c_open);
    }
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_clean(mi_unet_t *h, const uint8_t *masks, int D, int H, int W, const int *values, int n, const int spacing_units[3],
                         const mi_unet_volume_clean_opts *opts, uint8_t *out, mi_unet_volume_clean_stat *stats)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_volume_clean_opts o = opts ? *opts : kDefaultCleanOpts;
    if (int rc = check_clean_args("mi_unet_volume_clean", masks, D, H, W, values, n, spacing_units, o, out)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t dhw = (size_t)D * H * W, N = dhw * n, count_bytes = (size_t)n * 4 * sizeof(unsigned long long);
    // device and pinned alike: the volume, out, the counts; device only: the kernels' workspace
    const size_t at_out = up256(dhw), at_counts = at_out + up256(N), at_ws = at_counts + up256(count_bytes);
    const size_t dev_need = at_ws + volume_clean_workspace_bytes(D, H, W, n), host_need = at_ws;
    hipStream_t s = h->stream;
    if (int rc = h->ws_vclean.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_vclean.d, *const p = h->ws_vclean.p;
    host_copy(h, p, masks, dhw);
    HIP_TRY(hipMemcpyAsync(d, p, dhw, hipMemcpyHostToDevice, s));
    VolumeCleanArgs a;
    a.D = D; a.H = H; a.W = W; a.n = n;
    a.ux = spacing_units[0]; a.uy = spacing_units[1]; a.uz = spacing_units[2];
    a.fill = o.fill; a.close_r = o.close_r; a.open_r = o.open_r;
    for (int k = 0; k < n; ++k) a.v[k] = values[k];
    const hipError_t e = launch_volume_clean(d, a, d + at_out, reinterpret_cast<unsigned long long *>(d + at_counts), d + at_ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume clean launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p + at_out, d + at_out, at_ws - at_out, hipMemcpyDeviceToHost, s));      // out and the counts
    HIP_TRY(hipStreamSynchronize(s));                           // the call's only host synchronisation
    host_copy(h, out, p + at_out, N);
    if (stats) {
        const unsigned long long *const c = reinterpret_cast<const unsigned long long *>(p + at_counts);
        for (int k = 0; k < n; ++k) {
            // a step that was not run (no fill, a ball that is the single voxel) left no count: it is the one before it
            const int64_t c_in = (int64_t)c[4 * k], c_fill = o.fill ? (int64_t)c[4 * k + 1] : c_in;
            const int64_t c_close = single_voxel(spacing_units, o.close_r) ? c_fill : (int64_t)c[4 * k + 2];
            const int64_t c_open = single_voxel(spacing_units, o.open_r) ? c_close : (int64_t)c[4 * k + 3];
            stats[k] = make_stat(values[k], c_in, c_fill, c_close, c_open);
        }
    }
    return MI_UNET_OK;
}
#endif

}  // extern "C"
