// pipeline_tiled.cpp -- the tiled entry points (mi_unet_infer_tiled_*, mi_unet_segment_tiled_raw16), the blend settings and
// mi_unet_tile_axis.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "engine_handle.h"
#include "tile_grid.h"

using namespace miunet;

namespace {

// ---- tiled inference (include/mi_unet.h: mi_unet_infer_tiled_*) ------------------------------------------------
// One image of any size >= the engine's tile: uploaded once, cut into the overlapping tiles of tile_grid.h on the device, run in
// tile order through run_microbatch in micro-batches of max_batch (the buffers, routes, graphs and numeric guard of
// mi_unet_infer_u8), stitched on the device, and only then postprocessed / traced at full size.  Everything is enqueued on the
// engine's stream; the host waits once, at the end.
struct TiledCall {
    const char *fn;
    const uint8_t *img;                    // u8 form: [H][W][in_ch] ...
    const uint16_t *const *planes;         // ... or RAW form: in_ch planes of u16 [H][W]
    int H, W, halo;
    uint8_t *norm, *out_u8;                // out_u8: label map (infer) or 0 / 255 mask (segment)
    float *logits;
    const mi_unet_target *targets; int K;  // segment: K >= 1 targets, out_u8 and the contour arrays are [K]...; K = 0: infer
    int32_t *xy; int cap_points; int32_t *start; int cap_contours; int32_t *count;
    const mi_unet_morph *morph = nullptr; int n_morph = 0;     // segment: the targets' morphology, 1 or K entries; null: the 3x3 open
};

int ensure_tiled_buffers(mi_unet *h, size_t npix, bool want_logits, bool raw, bool blend)
{
    mi_unet::Tiled &t = h->tiled;
    const size_t C = (size_t)h->cfg.in_ch;
    if (npix <= t.px_cap && (!want_logits || npix <= t.logit_cap) && (!raw || npix <= t.raw_cap) && (!blend || npix <= t.acc_cap)) return 0;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (npix > t.px_cap) {
        t.px_cap = 0;
        HIP_TRY(t.d_img.reset(round_up(npix * C, 4)));            // whole dwords: launch_tile_gather reads aligned dwords
        HIP_TRY(t.d_labels.reset(npix));
        HIP_TRY(t.h_img.reset(npix * C));
        HIP_TRY(t.h_out.reset(npix));
        t.px_cap = npix;
    }
    if (want_logits && npix > t.logit_cap) {
        t.logit_cap = 0;
        HIP_TRY(t.d_logits.reset(npix * h->cfg.classes));
        t.logit_cap = npix;
    }
    if (raw && npix > t.raw_cap) {
        t.raw_cap = 0;
        HIP_TRY(t.d_raw.reset(round_up(npix, 8) * C));            // every plane starts on 16 bytes
        HIP_TRY(t.h_raw.reset(round_up(npix, 8) * C));
        t.raw_cap = npix;
    }
    if (blend && npix > t.acc_cap) {
        t.acc_cap = 0;
        HIP_TRY(t.d_acc.reset(npix * h->cfg.classes));
        t.acc_cap = npix;
    }
    return 0;
}

// the launch log of mi_unet_get_kernel_stats for a launch outside the plan: the event pair of launch_plan, algorithmic bytes
int stat_begin(mi_unet *h, hipStream_t s, hipEvent_t &e1)
{
    e1 = nullptr;
    if (!h->profiling) return 0;
    if (int rc = grow_events(h->ev_pool, h->ev_used + 2)) return rc;
    hipEvent_t e0 = h->ev_pool[h->ev_used++];
    e1 = h->ev_pool[h->ev_used++];
    HIP_TRY(hipEventRecord(e0, s));
    return 0;
}

int stat_end(mi_unet *h, hipStream_t s, hipEvent_t e1, const char *name, const char *kernel, double bytes)
{
    if (!e1) return 0;
    HIP_TRY(hipEventRecord(e1, s));
    mi_unet_kernel_stat ks{};
    snprintf(ks.name, sizeof ks.name, "%s", name);
    snprintf(ks.kernel, sizeof ks.kernel, "%s", kernel);
    ks.bytes = bytes;
    ks.ms = -1.f;
    h->stats.push_back(ks);
    return 0;
}

int check_planes(const mi_unet *h, const uint16_t *const *planes, const char *fn)
{
    if (!planes) return fail(MI_UNET_EARG, std::string(fn) + ": null plane list");
    for (int p = 0; p < h->cfg.in_ch; ++p)
        if (!planes[p]) return fail(MI_UNET_EARG, std::string(fn) + ": plane " + std::to_string(p) + " is null");
    return 0;
}

int run_tiled_call(mi_unet *h, const TiledCall &c)
{
    const std::string fn = c.fn;
    const int th = h->cfg.height, tw = h->cfg.width, C = h->cfg.in_ch, Bm = h->cfg.max_batch, classes = h->cfg.classes;
    const int H = c.H, W = c.W;
    if (H < th || W < tw)
        return fail(MI_UNET_EARG, fn + ": image " + std::to_string(H) + " x " + std::to_string(W) + " is smaller than the engine's tile " +
                                      std::to_string(th) + " x " + std::to_string(tw));
    if (c.halo < 0 || 2 * (long long)c.halo >= std::min(th, tw))
        return fail(MI_UNET_EARG, fn + ": halo " + std::to_string(c.halo) + " must satisfy 0 <= 2 * halo < min(tile height, tile width) = " +
                                      std::to_string(std::min(th, tw)));
    if ((long long)H * W > (1ll << 30) || W > (1 << 28))                    // 32-bit byte offsets inside a row of logits
        return fail(MI_UNET_EARG, fn + ": images of more than 2^30 pixels or wider than 2^28 are not supported");
    TileGrid g;
    if (!tile_grid(H, W, th, tw, c.halo, g)) return fail(MI_UNET_EARG, fn + ": illegal tile grid");
    const size_t npix = (size_t)H * W, thw = (size_t)th * tw;
    const int nt = g.ny * g.nx;
    // segment: the call's targets as K planes of the stitched image, min_area from the full image; infer: the label map itself,
    // postprocessed in place for the reference's target when mi_unet_set_postprocess is on
    const bool segment = c.K > 0;
    TargetTable tab = segment ? target_table(c.targets, c.K, H, W) : h->postprocess ? default_targets(H, W) : TargetTable{};
    if (segment && c.morph) table_morph(tab, c.morph, c.n_morph);
    const int K = segment ? c.K : 1;
    const ContourLayout cl{ K, c.cap_points, c.cap_contours };
    // the full-size tail stages borrow the network's scratch buffer: checked before anything is enqueued
    const size_t scratch = sizeof(float) * h->s_floats;
    const std::string what = (K > 1 ? std::to_string(K) + " targets of a " : std::string("a ")) + std::to_string(H) + " x " + std::to_string(W) + " image (";
    if (tab.K && postprocess_workspace_bytes(K, H, W) > scratch)
        return fail(MI_UNET_EARG, fn + ": the postprocess workspace of " + what +
                                      std::to_string(postprocess_workspace_bytes(K, H, W)) + " bytes) exceeds the scratch buffer (" +
                                      std::to_string(scratch) + " bytes)");
    if (segment && contour_workspace_bytes(K, H, W, c.cap_contours) > scratch)
        return fail(MI_UNET_EARG, fn + ": the contour workspace of " + what +
                                      std::to_string(contour_workspace_bytes(K, H, W, c.cap_contours)) + " bytes) exceeds the scratch buffer (" +
                                      std::to_string(scratch) + " bytes)");
    if ((long long)K * H * W > 0x7FFFFFFFLL) return fail(MI_UNET_EARG, fn + ": targets x pixels exceeds 2^31 - 1");
    if (segment && h->measure.on)
        if (int rc = check_measure_size(H, W, fn)) return rc;
    // blending or mirror averaging (mi_unet_set_tile_blend): nv views per tile, view k = t * nv + v, the network's logits
    // accumulated into t.d_acc, which also returns the blended logits; otherwise the ownership stitch
    const mi_unet_tile_blend bl = h->blend;
    const bool blend = bl.mode != MI_UNET_BLEND_OWNER || bl.mirror != 0, owner = bl.mode == MI_UNET_BLEND_OWNER;
    const int nv = blend ? tile_view_count(bl.mirror) : 1, nk = nt * nv;
    const float *d_wy = h->d_blend_w, *d_wx = h->d_blend_w ? h->d_blend_w + th : nullptr;
    HIP_TRY(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    if (int rc = ensure_tiled_buffers(h, npix, c.logits != nullptr && !blend, c.planes != nullptr, blend)) return rc;
    if (segment)
        if (int rc = grow_contour_buffers(h, cl)) return rc;
    if (c.planes)
        if (int rc = begin_window_call(h, (size_t)C, (size_t)C, (unsigned long long)npix, fn)) return rc;
    const mi_unet_window &win = h->window;
    const bool minmax = win.mode == MI_UNET_WINDOW_MINMAX, fixed = win.mode == MI_UNET_WINDOW_FIXED;
    mi_unet::Tiled &t = h->tiled;
    if (segment && K * npix > t.multi_cap) {
        HIP_TRY(hipStreamSynchronize(s));
        t.multi_cap = 0;
        HIP_TRY(t.d_multi.reset(K * npix));
        HIP_TRY(t.h_multi.reset(K * npix));
        t.multi_cap = K * npix;
    }
    // stage boundaries: start | pre | (gather | network + stitch or blend) per micro-batch | postprocess | contours | download
    const int nmb = (nk + Bm - 1) / Bm;
    const size_t n_marks = 2 + 2 * (size_t)nmb + 3;
    if (int rc = grow_events(t.ev, n_marks)) return rc;
    size_t mark = 0;
    hipEvent_t e1 = nullptr;
    hipError_t e = hipSuccess;
    HIP_TRY(hipEventRecord(t.ev[mark++], s));

    // ---- the image onto the device, once
    if (c.img) {
        host_copy(h, t.h_img, c.img, npix * C);
        HIP_TRY(hipMemcpyAsync(t.d_img, t.h_img, npix * C, hipMemcpyHostToDevice, s));
    } else {
        const size_t plane_stride = round_up(npix, 8);                       // launch_minmax_u16 / launch_normalise_u16 read 16-byte groups
        int src_of[4] = {};                        // a caller holding one plane passes its pointer in_ch times: upload and scan it once
        for (int p = 0; p < C; ++p) {
            src_of[p] = (p > 0 && c.planes[p] == c.planes[p - 1]) ? src_of[p - 1] : p;
            const int mn = src_of[p];
            uint16_t *d_plane = t.d_raw + (size_t)mn * plane_stride;
            if (mn == p) {
                hipPointerAttribute_t attr;                    // pinned caller memory is read by the DMA engine directly (as stage_raw16)
                const bool pinned = hipPointerGetAttributes(&attr, c.planes[p]) == hipSuccess && attr.type == hipMemoryTypeHost;
                if (!pinned) {
                    (void)hipGetLastError();
                    host_copy(h, t.h_raw + (size_t)p * plane_stride, c.planes[p], npix * sizeof(uint16_t));
                }
                HIP_TRY(hipMemcpyAsync(d_plane, pinned ? c.planes[p] : t.h_raw + (size_t)p * plane_stride, npix * sizeof(uint16_t), hipMemcpyHostToDevice, s));
                e = enqueue_window(h, d_plane, npix, (size_t)p, (size_t)p, s);
                if (e != hipSuccess) return fail(MI_UNET_EHIP, fn + ": min/max or window launch: " + hipGetErrorString(e));
            }
            h->win_src[p] = mn;
            if (int rc = stat_begin(h, s, e1)) return rc;
            e = minmax ? launch_normalise_u16(d_plane, W, H, h->d_mnmx + 2 * mn, t.d_img + p, C, s)
                       : launch_normalise_u16_window(d_plane, W, H, fixed ? nullptr : h->d_mnmx + 2 * mn, win.lo, win.hi, t.d_img + p, C, s);
            if (e != hipSuccess) return fail(MI_UNET_EHIP, fn + ": normalise launch: " + hipGetErrorString(e));
            if (int rc = stat_end(h, s, e1, ("tiled.normalise." + std::to_string(p)).c_str(), "normalise_u16", 3.0 * npix)) return rc;
        }
    }
    if (blend) HIP_TRY(hipMemsetAsync(t.d_acc, 0, sizeof(float) * npix * classes, s));
    HIP_TRY(hipEventRecord(t.ev[mark++], s));

    // ---- tiles (views) in order, micro-batches of max_batch: gather -> network -> stitch, or -> blend (+ finalize after the last)
    auto owned_px = [&](int tile) {
        const int ty = tile / g.nx, tx = tile % g.nx;
        return (double)(tile_cut(H, th, g.sy, g.ny, ty + 1) - tile_cut(H, th, g.sy, g.ny, ty)) *
               (tile_cut(W, tw, g.sx, g.nx, tx + 1) - tile_cut(W, tw, g.sx, g.nx, tx));
    };
    float *d_tile_logits = (c.logits || blend) ? h->d_logits : nullptr;
    for (int t0 = 0; t0 < nk; t0 += Bm) {
        const int nb = std::min(Bm, nk - t0);
        const std::string tag = "[" + std::to_string(t0) + "," + std::to_string(t0 + nb) + ")";
        if (int rc = stat_begin(h, s, e1)) return rc;
        e = nv > 1 ? launch_tile_gather_views(t.d_img, round_up(npix * C, 4), H, W, C, th, tw, c.halo, bl.mirror, t0, nb, h->d_img, s)
                   : launch_tile_gather(t.d_img, round_up(npix * C, 4), H, W, C, th, tw, c.halo, t0, nb, h->d_img, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, fn + ": gather launch: " + hipGetErrorString(e));
        if (int rc = stat_end(h, s, e1, ("tiled.gather" + tag).c_str(), "tile_gather", 2.0 * nb * thw * C)) return rc;
        HIP_TRY(hipEventRecord(t.ev[mark++], s));
        if (int rc = run_microbatch(h, h->d_img, nb, h->d_labels, d_tile_logits)) return rc;
        if (!blend) {
            // owned pixels of this micro-batch: read once from the tile results, written once
            double owned = 0;
            for (int k = t0; k < t0 + nb; ++k) owned += owned_px(k);
            if (int rc = stat_begin(h, s, e1)) return rc;
            e = launch_tile_stitch(h->d_labels, d_tile_logits, classes, H, W, th, tw, c.halo, t0, nb, t.d_labels, c.logits ? t.d_logits : nullptr, s);
            if (e != hipSuccess) return fail(MI_UNET_EHIP, fn + ": stitch launch: " + hipGetErrorString(e));
            if (int rc = stat_end(h, s, e1, ("tiled.stitch" + tag).c_str(), "tile_stitch", 2.0 * owned * (1.0 + (c.logits ? 4.0 * classes : 0.0)))) return rc;
        } else {
            // per (view, pixel it contributes to): its logits read once, the accumulator read and written once
            double covered = 0;
            for (int k = t0; k < t0 + nb; ++k) covered += owner ? owned_px(k / nv) : (double)thw;
            if (int rc = stat_begin(h, s, e1)) return rc;
            e = launch_tile_blend(h->d_logits, classes, H, W, th, tw, c.halo, bl.mirror, owner, d_wy, d_wx, t0, nb, t.d_acc, s);
            if (e != hipSuccess) return fail(MI_UNET_EHIP, fn + ": blend launch: " + hipGetErrorString(e));
            if (int rc = stat_end(h, s, e1, ("tiled.blend" + tag).c_str(), "tile_blend", 12.0 * classes * covered)) return rc;
            if (t0 + nb == nk) {
                if (int rc = stat_begin(h, s, e1)) return rc;
                e = launch_blend_finalize(t.d_acc, classes, H, W, th, tw, c.halo, bl.mirror, owner, d_wy, d_wx, t.d_labels, c.logits ? t.d_acc : nullptr, s);
                if (e != hipSuccess) return fail(MI_UNET_EHIP, fn + ": blend finalize launch: " + hipGetErrorString(e));
                if (int rc = stat_end(h, s, e1, "tiled.finalize", "blend_finalize", (double)npix * (4.0 * classes + 1.0 + (c.logits ? 4.0 * classes : 0.0)))) return rc;
            }
        }
        HIP_TRY(hipEventRecord(t.ev[mark++], s));
    }

    // ---- the tail, on the stitched image: one image of H x W, never per tile
    uint8_t *const d_result = segment ? t.d_multi.get() : t.d_labels.get(), *const h_result = segment ? t.h_multi.get() : t.h_out.get();
    const hipEvent_t post_done = t.ev[mark++];
    // mi_unet_set_measure: intensity from the full-size normalised image, coordinates of the stitched mask; K planes over one image
    const bool measuring = segment && h->measure.on;
    const RegionLayout rl{ K, c.cap_contours };
    if (segment) {
        if (measuring)
            if (int rc = grow_region_buffers(h, rl)) return rc;     // (s was synchronised by the call before this one)
        begin_region_call(h, measuring, K, c.cap_contours);
    }
    const MeasureArgs ma{ t.d_img, 0 };
    if (int rc = enqueue_tail(h, t.d_labels, 1, H, W, tab, d_result, h->d_s1, segment ? &cl : nullptr, post_done, s, fn + ": ",
                              measuring ? &ma : nullptr))
        return rc;
    HIP_TRY(hipEventRecord(t.ev[mark++], s));
    HIP_TRY(hipMemcpyAsync(h_result, d_result, K * npix, hipMemcpyDeviceToHost, s));
    if (c.norm) HIP_TRY(hipMemcpyAsync(t.h_img, t.d_img, npix * C, hipMemcpyDeviceToHost, s));
    if (c.planes)
        if (int rc = enqueue_window_download(h, (size_t)C, s)) return rc;
    if (segment)
        if (int rc = contours_to_pinned(h, cl, s)) return rc;
    if (c.logits) HIP_TRY(hipMemcpyAsync(c.logits, blend ? t.d_acc : t.d_logits, sizeof(float) * npix * classes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(t.ev[mark++], s));
    HIP_TRY(hipStreamSynchronize(s));
    host_copy(h, c.out_u8, h_result, K * npix);
    if (c.norm) host_copy(h, c.norm, t.h_img, npix * C);
    if (segment) contours_to_caller(h, cl, c.xy, c.start, c.count);
    if (measuring) regions_to_report(h, rl, 0, 0);
    if (segment) finish_region_call(h);
    if (c.planes) finish_window_call(h, (size_t)C);

    for (float &m : h->stage_ms) m = 0.f;
    auto span = [&](size_t a, size_t b, int stage) -> int {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, t.ev[a], t.ev[b]));
        h->stage_ms[stage] += ms;
        return 0;
    };
    if (int rc = span(0, 1, MI_UNET_STAGE_UPLOAD_PRE)) return rc;
    for (int k = 0; k < nmb; ++k) {
        if (int rc = span(1 + 2 * (size_t)k, 2 + 2 * (size_t)k, MI_UNET_STAGE_UPLOAD_PRE)) return rc;
        if (int rc = span(2 + 2 * (size_t)k, 3 + 2 * (size_t)k, MI_UNET_STAGE_NETWORK)) return rc;
    }
    const size_t m0 = 1 + 2 * (size_t)nmb;
    if (int rc = span(m0, m0 + 1, MI_UNET_STAGE_POSTPROCESS)) return rc;
    if (int rc = span(m0 + 1, m0 + 2, MI_UNET_STAGE_CONTOURS)) return rc;
    return span(m0 + 2, m0 + 3, MI_UNET_STAGE_DOWNLOAD);
}

}  // namespace

extern "C" {

int mi_unet_tile_axis(int L, int T, int halo, int *origins, int *cuts) { return tile_axis(L, T, halo, origins, cuts); }

int mi_unet_tile_blend_weights(int T, const mi_unet_tile_blend *b, float *w)
{
    if (T < 1 || !b || !w) return fail(MI_UNET_EARG, "mi_unet_tile_blend_weights: T < 1 or a null pointer");
    if (b->mode < MI_UNET_BLEND_OWNER || b->mode > MI_UNET_BLEND_GAUSSIAN)
        return fail(MI_UNET_EARG, "tile blend: unknown mode " + std::to_string(b->mode));
    if (b->mirror < 0 || b->mirror > (MI_UNET_MIRROR_X | MI_UNET_MIRROR_Y))
        return fail(MI_UNET_EARG, "tile blend: mirror " + std::to_string(b->mirror) + " is outside 0..3");
    if (b->mode == MI_UNET_BLEND_GAUSSIAN && !(std::isfinite(b->sigma_scale) && b->sigma_scale > 0.f))
        return fail(MI_UNET_EARG, "tile blend: the Gaussian needs a finite sigma_scale > 0");
    // the definition of include/mi_unet.h: double, one rounding to float; i - c is exact, so w(i) == w(T - 1 - i)
    const double c = (T - 1) / 2.0, s = (double)b->sigma_scale * T;
    for (int i = 0; i < T; ++i) {
        const double d = i - c;
        w[i] = b->mode == MI_UNET_BLEND_GAUSSIAN ? (float)std::max(std::exp(-(d * d) / (2.0 * s * s)), 0x1p-20) : 1.f;
    }
    return MI_UNET_OK;
}

int mi_unet_set_tile_blend(mi_unet_t *h, const mi_unet_tile_blend *b)
{
    if (int rc = check_handle(h, false)) return rc;
    const mi_unet_tile_blend def{ MI_UNET_BLEND_OWNER, 0.125f, 0 };
    const mi_unet_tile_blend nb = b ? *b : def;
    const int th = h->cfg.height, tw = h->cfg.width;
    std::vector<float> tab((size_t)th + tw);
    if (int rc = mi_unet_tile_blend_weights(th, &nb, tab.data())) return rc;
    if (int rc = mi_unet_tile_blend_weights(tw, &nb, tab.data() + th)) return rc;
    HIP_TRY(hipSetDevice(h->cfg.device));
    if (!h->d_blend_w) HIP_TRY(h->d_blend_w.reset(tab.size()));
    HIP_TRY(hipStreamSynchronize(h->stream));                            // no call of this handle still reads the old tables
    HIP_TRY(hipMemcpy(h->d_blend_w, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice));
    h->blend = nb;
    return MI_UNET_OK;
}

int mi_unet_get_tile_blend(const mi_unet_t *h, mi_unet_tile_blend *b)
{
    if (!h || !b) return fail(MI_UNET_EARG, "mi_unet_get_tile_blend: null argument");
    *b = h->blend;
    return MI_UNET_OK;
}

int mi_unet_infer_tiled_u8(mi_unet_t *h, const uint8_t *img, int H, int W, int halo, uint8_t *labels, float *logits)
{
    if (int rc = check_handle(h, true)) return rc;
    if (!img || !labels) return fail(MI_UNET_EARG, "mi_unet_infer_tiled_u8: null image or label buffer");
    const TiledCall c{ "mi_unet_infer_tiled_u8", img, nullptr, H, W, halo, nullptr, labels, logits, nullptr, 0, nullptr, 0, nullptr, 0, nullptr };
    return run_tiled_call(h, c);
}

int mi_unet_infer_tiled_raw16(mi_unet_t *h, const uint16_t *const *planes, int W, int H, int halo, uint8_t *norm, uint8_t *labels,
                              float *logits)
{
    if (int rc = check_handle(h, true)) return rc;
    if (int rc = check_planes(h, planes, "mi_unet_infer_tiled_raw16")) return rc;
    if (!labels) return fail(MI_UNET_EARG, "mi_unet_infer_tiled_raw16: null label buffer");
    const TiledCall c{ "mi_unet_infer_tiled_raw16", nullptr, planes, H, W, halo, norm, labels, logits, nullptr, 0, nullptr, 0, nullptr, 0, nullptr };
    return run_tiled_call(h, c);
}

// mi_unet_segment_tiled_raw16 (the reference's target, whatever the handle's setting) and its _multi form (the handle's targets)
static int segment_tiled_call(mi_unet_t *h, const char *fn, bool multi, const uint16_t *const *planes, int W, int H, int halo, uint8_t *norm,
                              uint8_t *mask, int32_t *xy, int cap_points, int32_t *start, int cap_contours, int32_t *count)
{
    if (int rc = check_handle(h, true)) return rc;
    if (int rc = check_planes(h, planes, fn)) return rc;
    if (!mask || !xy || !start || !count || cap_points <= 0 || cap_contours <= 0)
        return fail(MI_UNET_EARG, std::string(fn) + ": null output buffer or non-positive capacity");
    if (multi)
        if (int rc = check_morph_list(h, fn)) return rc;
    const TiledCall c{ fn, nullptr, planes, H, W, halo, norm, mask, nullptr, multi ? h->targets : &kDefaultTarget, multi ? h->n_targets : 1,
                       xy, cap_points, start, cap_contours, count, multi ? h->morph : nullptr, multi ? h->n_morph : 0 };
    return run_tiled_call(h, c);
}

int mi_unet_segment_tiled_raw16(mi_unet_t *h, const uint16_t *const *planes, int W, int H, int halo, uint8_t *norm, uint8_t *mask,
                                int32_t *xy, int cap_points, int32_t *start, int cap_contours, int32_t *count)
{
    return segment_tiled_call(h, "mi_unet_segment_tiled_raw16", false, planes, W, H, halo, norm, mask, xy, cap_points, start, cap_contours, count);
}

int mi_unet_segment_tiled_raw16_multi(mi_unet_t *h, const uint16_t *const *planes, int W, int H, int halo, uint8_t *norm, uint8_t *mask,
                                      int32_t *xy, int cap_points, int32_t *start, int cap_contours, int32_t *count)
{
    return segment_tiled_call(h, "mi_unet_segment_tiled_raw16_multi", true, planes, W, H, halo, norm, mask, xy, cap_points, start, cap_contours,
                              count);
}

}  // extern "C"
