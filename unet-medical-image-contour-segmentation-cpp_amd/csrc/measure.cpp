// measure.cpp -- region measurement (include/mi_unet.h: mi_unet_set_measure): the setting, the report behind
// mi_unet_last_regions, the stage alone on host buffers, and the derived quantities as host arithmetic (mi_unet_region_derive).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "engine_handle.h"

static_assert(sizeof(mi_unet_region) == 96, "mi_unet_region is 96 bytes without padding");

namespace miunet {

int check_measure_size(int H, int W, const std::string &fn)
{
    const unsigned __int128 m = (unsigned)std::max(H, W);
    if ((unsigned __int128)(unsigned)H * (unsigned)W * m * m >= (unsigned __int128)3 << 62)
        return fail(MI_UNET_EARG, fn + ": " + std::to_string(H) + " x " + std::to_string(W) + " is too large to measure (a moment sum could pass 2^62)");
    return 0;
}

int grow_region_buffers(mi_unet *h, const RegionLayout &rl)
{
    const size_t need = rl.bytes();
    if (need <= h->regions_cap) return 0;
    h->regions_cap = 0;
    HIP_TRY(h->d_regions.reset(need));
    for (auto &b : h->h_regions) HIP_TRY(b.reset(need));
    h->regions_cap = need;
    return 0;
}

void begin_region_call(mi_unet *h, bool measuring, int planes, int cap)
{
    h->last_regions_valid = false;
    h->last_region_planes = measuring ? planes : 0;
    h->last_region_cap = measuring ? cap : 0;
    if (measuring) {
        h->last_regions.assign((size_t)planes * cap, mi_unet_region{});
        h->last_region_counts.assign((size_t)planes, 0);
    }
}

void regions_to_report(mi_unet *h, const RegionLayout &rl, int plane0, int half)
{
    const uint8_t *base = h->h_regions[half];
    memcpy(h->last_regions.data() + (size_t)plane0 * rl.cap, rl.regions(base), (size_t)rl.planes * rl.cap * sizeof(mi_unet_region));
    memcpy(h->last_region_counts.data() + plane0, rl.counts(base), (size_t)rl.planes * sizeof(int32_t));
}

void finish_region_call(mi_unet *h) { h->last_regions_valid = h->last_region_cap > 0; }

}  // namespace miunet

using namespace miunet;

extern "C" {

int mi_unet_set_measure(mi_unet_t *h, const mi_unet_measure *m)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_measure v = m ? *m : mi_unet_measure{ 0, 0 };
    if (v.channel < 0 || v.channel >= h->cfg.in_ch)
        return fail(MI_UNET_EARG, "mi_unet_set_measure: channel " + std::to_string(v.channel) + " is outside 0.." + std::to_string(h->cfg.in_ch - 1));
    h->measure = { v.on != 0, v.channel };
    return MI_UNET_OK;
}

int mi_unet_get_measure(const mi_unet_t *h, mi_unet_measure *m)
{
    if (!h || !m) return fail(MI_UNET_EARG, "mi_unet_get_measure: null argument");
    *m = h->measure;
    return MI_UNET_OK;
}

int mi_unet_last_regions(const mi_unet_t *h, mi_unet_region *regions, int32_t *counts, int cap_planes, int *planes, int *cap_contours)
{
    if (!h || !planes || !cap_contours || cap_planes < 0) return fail(MI_UNET_EARG, "mi_unet_last_regions: bad argument");
    if (!h->last_regions_valid)
        return fail(MI_UNET_ESTATE, "mi_unet_last_regions: the last contour-returning call on this handle did not measure (mi_unet_set_measure), or there was none");
    *planes = h->last_region_planes;
    *cap_contours = h->last_region_cap;
    const size_t np = (size_t)std::min(h->last_region_planes, cap_planes);
    if (regions) memcpy(regions, h->last_regions.data(), np * h->last_region_cap * sizeof(mi_unet_region));
    if (counts) memcpy(counts, h->last_region_counts.data(), np * sizeof(int32_t));
    return MI_UNET_OK;
}

int mi_unet_measure_regions(mi_unet_t *h, const uint8_t *masks, const uint8_t *tiles, int B, int channel, mi_unet_region *regions,
                            int cap_contours, int32_t *counts)
{
    if (int rc = check_handle(h, false)) return rc;
    if (!masks || !regions || !counts || B < 0 || cap_contours <= 0) return fail(MI_UNET_EARG, "mi_unet_measure_regions: bad argument");
    if (tiles && (channel < 0 || channel >= h->cfg.in_ch))
        return fail(MI_UNET_EARG, "mi_unet_measure_regions: channel " + std::to_string(channel) + " is outside 0.." + std::to_string(h->cfg.in_ch - 1));
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int H = h->cfg.height, W = h->cfg.width, Bm = h->cfg.max_batch;
    const size_t hw = (size_t)H * W, C = (size_t)h->cfg.in_ch;
    if (int rc = check_measure_size(H, W, "mi_unet_measure_regions")) return rc;
    const size_t scratch = sizeof(float) * (size_t)Bm * hw * h->ch[0];
    hipStream_t s = h->stream;
    for (int b0 = 0; b0 < B; b0 += Bm) {
        const int bm = std::min(Bm, B - b0);
        if (contour_workspace_bytes(bm, H, W, cap_contours) > scratch)
            return fail(MI_UNET_EARG, "contour workspace does not fit the scratch buffer (cap_contours too large)");
        const RegionLayout rl{ bm, cap_contours };
        HIP_TRY(hipStreamSynchronize(s));
        if (int rc = grow_region_buffers(h, rl)) return rc;
        uint8_t *const d_reg = h->d_regions;
        memcpy(h->h_labels, masks + b0 * hw, bm * hw);
        HIP_TRY(hipMemcpyAsync(h->d_labels, h->h_labels, bm * hw, hipMemcpyHostToDevice, s));
        if (tiles) {
            memcpy(h->h_img, tiles + b0 * hw * C, bm * hw * C);
            HIP_TRY(hipMemcpyAsync(h->d_img, h->h_img, bm * hw * C, hipMemcpyHostToDevice, s));
        }
        hipError_t e = launch_label_contours(h->d_labels, bm, H, W, cap_contours, h->d_s1, s);
        if (e == hipSuccess)
            e = launch_measure_regions(bm, H, W, 1, tiles ? h->d_img.get() : nullptr, (int)C, channel, rl.regions(d_reg), rl.counts(d_reg),
                                       cap_contours, h->d_s1, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("region launch: ") + hipGetErrorString(e));
        HIP_TRY(hipMemcpyAsync(h->h_regions[0], d_reg, rl.bytes(), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const uint8_t *base = h->h_regions[0];
        memcpy(regions + (size_t)b0 * cap_contours, rl.regions(base), (size_t)bm * cap_contours * sizeof(mi_unet_region));
        memcpy(counts + b0, rl.counts(base), (size_t)bm * sizeof(int32_t));
    }
    return MI_UNET_OK;
}

int mi_unet_region_derive(const mi_unet_region *r, mi_unet_region_shape *out)
{
    if (!r || !out) return fail(MI_UNET_EARG, "mi_unet_region_derive: null argument");
    if (r->area < 1) return fail(MI_UNET_EARG, "mi_unet_region_derive: area " + std::to_string(r->area) + " (a region has at least one pixel)");
    const __int128 A = r->area;
    const double Ad = (double)r->area, A2 = Ad * Ad;
    // exact 128-bit numerators, converted once: A * sxx < 2^93, sx^2 < 2^124
    auto central = [&](int64_t sab, int64_t sa, int64_t sb) { return (double)(A * sab - (__int128)sa * sb) / A2; };
    const double a = central(r->sxx, r->sx, r->sx) + 1.0 / 12.0, c = central(r->syy, r->sy, r->sy) + 1.0 / 12.0;
    const double b = central(r->sxy, r->sx, r->sy);
    const double root = std::sqrt((a - c) * (a - c) + 4.0 * b * b);
    out->cx = (double)r->sx / Ad;
    out->cy = (double)r->sy / Ad;
    out->major = 4.0 * std::sqrt(((a + c) + root) / 2.0);
    out->minor = 4.0 * std::sqrt(std::max(((a + c) - root) / 2.0, 0.0));
    out->theta = 0.5 * std::atan2(2.0 * b, a - c);
    out->mean = (double)r->si / Ad;
    out->std = std::sqrt(std::max(central(r->sii, r->si, r->si), 0.0));
    return MI_UNET_OK;
}

}  // extern "C"
