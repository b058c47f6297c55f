// volume_interp.cpp -- slices put between the slices of a stack of masks, shape-based (include/mi_unet.h: mi_unet_volume_interp;
// DESIGN.md 7.16): the argument checks, the definition as sequential host arithmetic (mi_unet_volume_interp_host) and the entry point
// on the handle, which owns the stage's workspace.  With MIUNET_NO_DEVICE only the host arithmetic is compiled (stage_common.h;
// tests/cpu/volume_interp_host_test.cpp).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "stage_common.h"

static_assert(sizeof(mi_unet_vinterp_stat) == 40, "mi_unet_vinterp_stat is 40 bytes without padding");

namespace miunet {

namespace {

constexpr int kMaxSide = MI_UNET_SCORE_VOLUME_MAX_SIDE;
constexpr int kMaxFactor = MI_UNET_VINTERP_MAX_FACTOR;
constexpr int32_t kNone = MI_UNET_VINTERP_NONE;

int gcd(int a, int b) { return b ? gcd(b, a % b) : a; }

// ((W - 1) ux)^2 + ((H - 1) uy)^2 < 2^31 - 1 without overflow for any unit: a term of 46341 or more fails by itself
bool e_fits(int H, int W, int ux, int uy)
{
    if (W > 1 && ux > 46340 / (W - 1)) return false;
    if (H > 1 && uy > 46340 / (H - 1)) return false;
    const int64_t tx = (int64_t)(W - 1) * ux, ty = (int64_t)(H - 1) * uy;
    return tx * tx + ty * ty < (int64_t)kNone;
}

// every MI_UNET_EARG case of the two entry points; nothing has been queued or written when it fails.  ux, uy: the reduced units
int check_interp_args(const char *fn, const uint8_t *masks, int D, int H, int W, const int *values, int n, const int *units, int factor,
                      const uint16_t *intensity, const uint8_t *out, const uint16_t *intensity_out, int &ux, int &uy)
{
    const std::string f = fn;
    if (!masks || !values || !units || !out) return fail(MI_UNET_EARG, f + ": null argument");
    if ((intensity == nullptr) != (intensity_out == nullptr))
        return fail(MI_UNET_EARG, f + ": intensity and intensity_out are given together or not at all");
    if (int rc = check_sides_max(f, D, H, W, kMaxSide)) return rc;
    if (int rc = check_values(f, values, n, MI_UNET_VOLUME_MAX_VALUES)) return rc;
    if (factor < 1 || factor > kMaxFactor)
        return fail(MI_UNET_EARG, f + ": factor " + std::to_string(factor) + " is outside 1 .. " + std::to_string(kMaxFactor));
    const long long Dp = (long long)(D - 1) * factor + 1;
    if (!product_below_2_31(n, Dp, H, W)) return fail(MI_UNET_EARG, f + ": n * D' * H * W must stay below 2^31");
    if (int rc = check_units_min1(f, units, 2)) return rc;
    const int g = gcd(units[0], units[1]);
    ux = units[0] / g; uy = units[1] / g;
    if (!e_fits(H, W, ux, uy)) return fail(MI_UNET_EARG, f + ": ((W - 1) ux)^2 + ((H - 1) uy)^2 must stay below 2^31 - 1");
    const size_t in_bytes = (size_t)D * H * W, out_bytes = (size_t)n * Dp * H * W;
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(masks), o0 = reinterpret_cast<uintptr_t>(out);
    if (o0 < m0 + in_bytes && m0 < o0 + out_bytes) return fail(MI_UNET_EARG, f + ": out overlaps masks");
    return MI_UNET_OK;
}

// The signed squared distance of one slice of one plane (the DISTANCE of include/mi_unet.h): h = down and up the columns the index
// distance to the nearest pixel of the other state (kSent = none), then along each row the minimum over the columns, by a scan outward
// that stops once (ux dx)^2 alone reaches the best so far.
constexpr int kSent = 0x7FFF;

void signed_distance(const uint8_t *m, int v, int H, int W, int ux, int uy, std::vector<int> &h, int32_t *f)
{
    const size_t hw = (size_t)H * W;
    bool any_set = false, any_unset = false;
    for (size_t i = 0; i < hw; ++i) (m[i] == v ? any_set : any_unset) = true;
    if (!(any_set && any_unset)) {
        for (size_t i = 0; i < hw; ++i) f[i] = any_set ? kNone : -kNone;
        return;
    }
    for (int x = 0; x < W; ++x) {
        int d = kSent;
        for (int y = 0; y < H; ++y) {
            const bool cur = m[(size_t)y * W + x] == v;
            d = (y > 0 && cur != (m[(size_t)(y - 1) * W + x] == v)) ? 1 : std::min(d + 1, kSent);
            h[(size_t)y * W + x] = d;
        }
        d = kSent;
        for (int y = H - 1; y >= 0; --y) {
            const bool cur = m[(size_t)y * W + x] == v;
            d = (y < H - 1 && cur != (m[(size_t)(y + 1) * W + x] == v)) ? 1 : std::min(d + 1, kSent);
            h[(size_t)y * W + x] = std::min(h[(size_t)y * W + x], d);
        }
    }
    for (int y = 0; y < H; ++y) {
        const uint8_t *const mr = m + (size_t)y * W;
        const int *const hr = h.data() + (size_t)y * W;
        for (int x = 0; x < W; ++x) {
            const bool st = mr[x] == v;
            int64_t best = hr[x] == kSent ? (int64_t)kNone : (int64_t)uy * hr[x] * uy * hr[x];
            for (int dx = 1; ; ++dx) {
                const int xl = x - dx, xr = x + dx;
                if (xl < 0 && xr >= W) break;
                const int64_t t = (int64_t)ux * dx * ux * dx;
                if (t >= best) break;
                for (int xx : { xl, xr }) {
                    if (xx < 0 || xx >= W) continue;
                    if ((mr[xx] == v) != st) best = std::min(best, t);
                    else if (hr[xx] != kSent) best = std::min(best, t + (int64_t)uy * hr[xx] * uy * hr[xx]);
                }
            }
            f[(size_t)y * W + x] = st ? (int32_t)best : -(int32_t)best;
        }
    }
}

}  // namespace

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_volume_interp_slices(int D, int factor)
{
    if (D < 1 || D > kMaxSide || factor < 1 || factor > kMaxFactor) return -1;
    return (D - 1) * factor + 1;
}

int mi_unet_volume_interp_host(const uint8_t *masks, int D, int H, int W, const int *values, int n, const int units_xy[2], int factor,
                               const uint16_t *intensity, uint8_t *out, uint16_t *intensity_out, mi_unet_vinterp_stat *stats)
{
    int ux = 1, uy = 1;
    if (int rc = check_interp_args("mi_unet_volume_interp_host", masks, D, H, W, values, n, units_xy, factor, intensity, out, intensity_out, ux, uy))
        return rc;
    const int k = factor;
    const size_t hw = (size_t)H * W, Dp = (size_t)(D - 1) * k + 1;
    std::vector<int> h(hw);
    std::vector<int32_t> field(2 * hw);
    for (int p = 0; p < n; ++p) {
        const int v = values[p];
        mi_unet_vinterp_stat st{ 0, 0, 0, 0, 0 };
        uint8_t *const o = out + (size_t)p * Dp * hw;
        signed_distance(masks, v, H, W, ux, uy, h, field.data());
        for (int z = 0; z < D; ++z) {
            const int32_t *const fa = field.data() + (size_t)(z & 1) * hw;
            int32_t *const fb = field.data() + (size_t)((z + 1) & 1) * hw;
            if (z + 1 < D) signed_distance(masks + (size_t)(z + 1) * hw, v, H, W, ux, uy, h, fb);
            for (int j = 0; j < (z + 1 < D ? k : 1); ++j) {
                uint8_t *const os = o + ((size_t)z * k + j) * hw;
                for (size_t i = 0; i < hw; ++i) {
                    const bool sa = fa[i] > 0;
                    bool set = sa;
                    if (j == 0) {
                        st.in_voxels += sa;
                    } else if (sa != (fb[i] > 0)) {
                        const int64_t e_set = sa ? fa[i] : fb[i], e_unset = sa ? -(int64_t)fb[i] : -(int64_t)fa[i];
                        const int64_t w_set = sa ? k - j : j, w_unset = k - w_set;
                        const int64_t lhs = w_set * w_set * e_set, rhs = w_unset * w_unset * e_unset;
                        set = lhs >= rhs;
                        ++st.mixed;
                        st.mixed_set += set;
                        st.ties += lhs == rhs;
                    }
                    os[i] = set ? (uint8_t)v : (uint8_t)0;
                    st.out_voxels += set;
                }
            }
        }
        if (stats) stats[p] = st;
    }
    if (intensity)
        for (int z = 0; z < D; ++z)
            for (int j = 0; j < (z + 1 < D ? k : 1); ++j)
                for (size_t i = 0; i < hw; ++i) {
                    const unsigned a = intensity[(size_t)z * hw + i], b = j ? intensity[(size_t)(z + 1) * hw + i] : 0u;
                    intensity_out[((size_t)z * k + j) * hw + i] = (uint16_t)(((unsigned)(k - j) * a + (unsigned)j * b + (unsigned)k / 2) / (unsigned)k);
                }
    return MI_UNET_OK;
}

#ifndef MIUNET_NO_DEVICE
int mi_unet_volume_interp(mi_unet_t *h, const uint8_t *masks, int D, int H, int W, const int *values, int n, const int units_xy[2], int factor,
                          const uint16_t *intensity, uint8_t *out, uint16_t *intensity_out, mi_unet_vinterp_stat *stats)
{
    if (int rc = check_handle(h, false)) return rc;
    int ux = 1, uy = 1;
    if (int rc = check_interp_args("mi_unet_volume_interp", masks, D, H, W, values, n, units_xy, factor, intensity, out, intensity_out, ux, uy))
        return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t hw = (size_t)H * W, dhw = (size_t)D * hw, Dp = (size_t)(D - 1) * factor + 1, N = (size_t)n * Dp * hw;
    const size_t count_bytes = (size_t)n * D * 5 * sizeof(unsigned long long);      // per plane and slice pair: the blend's counts
    const size_t in_i = intensity ? dhw * sizeof(uint16_t) : 0, out_i = intensity ? Dp * hw * sizeof(uint16_t) : 0;
    // device and pinned alike: the masks, the intensity, then what comes back in one copy: out, the counts, the intensity between the
    // slices; device only: the kernels' workspace
    const size_t at_int = up256(dhw), at_out = at_int + up256(in_i), at_counts = at_out + up256(N), at_iout = at_counts + up256(count_bytes);
    const size_t at_ws = at_iout + up256(out_i);
    const size_t dev_need = at_ws + volume_interp_workspace_bytes(D, H, W, n), host_need = at_ws;
    hipStream_t s = h->stream;
    if (int rc = h->ws_volume_interp.reserve(dev_need, host_need, s)) return rc;
    uint8_t *const d = h->ws_volume_interp.d, *const p = h->ws_volume_interp.p;
    host_copy(h, p, masks, dhw);
    if (intensity) host_copy(h, p + at_int, intensity, in_i);
    HIP_TRY(hipMemcpyAsync(d, p, intensity ? at_int + in_i : dhw, hipMemcpyHostToDevice, s));      // the call's one upload
    VolumeInterpArgs a;
    a.D = D; a.H = H; a.W = W; a.n = n; a.ux = ux; a.uy = uy; a.k = factor;
    for (int k = 0; k < n; ++k) a.v[k] = values[k];
    const hipError_t e = launch_volume_interp(d, intensity ? reinterpret_cast<const uint16_t *>(d + at_int) : nullptr, a, d + at_out,
                                              intensity ? reinterpret_cast<uint16_t *>(d + at_iout) : nullptr,
                                              reinterpret_cast<unsigned long long *>(d + at_counts), d + at_ws, s);
    if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("volume interp launch: ") + hipGetErrorString(e));
    HIP_TRY(hipMemcpyAsync(p + at_out, d + at_out, (intensity ? at_iout + out_i : at_counts + count_bytes) - at_out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));                           // the call's only host synchronisation
    host_copy(h, out, p + at_out, N);
    if (intensity) host_copy(h, intensity_out, p + at_iout, out_i);
    if (stats) {
        const unsigned long long *const c = reinterpret_cast<const unsigned long long *>(p + at_counts);
        for (int k = 0; k < n; ++k) {
            int64_t sum[5] = { 0, 0, 0, 0, 0 };
            for (size_t z = 0; z < (size_t)D; ++z)
                for (int j = 0; j < 5; ++j) sum[j] += (int64_t)c[((size_t)k * D + z) * 5 + j];
            stats[k] = mi_unet_vinterp_stat{ sum[0], sum[1], sum[2], sum[3], sum[4] };
        }
    }
    return MI_UNET_OK;
}
#endif

}  // extern "C"
