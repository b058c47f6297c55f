// pipeline_raw.cpp -- the RAW-in entry points (mi_unet_infer_raw16, mi_unet_segment_raw16): staging ring, the three-stream
// pipeline over micro-batches and its stage times.
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

namespace miunet {
// upload + min/max + resample `bm` RAW images into h->d_img.  An engine with in_ch = C > 1 takes C planes per image
// (plane c of image i at index i*C + c, each with its own size and its own min/max, as if every plane went through
// preprocess_raw on its own) and interleaves them into the HWC tile the first layer reads; a caller holding one plane per
// image passes its pointer C times (the grey -> B,G,R replication cv::imread(IMREAD_COLOR) does at src/mask2polygon.cpp:117).
// large host copies (RAW staging in, tiles / masks out) on the handle's helper threads (MIUNET_COPY_THREADS, default 4; 1 = plain memcpy)
void host_copy(mi_unet *h, void *dst, const void *src, size_t bytes)
{
    if (h->copy_threads > 1 && bytes >= (1u << 20)) {
        if (!h->copy_pool) h->copy_pool.reset(new CopyPool(h->copy_threads - 1));
        h->copy_pool->copy(dst, src, bytes);
    } else {
        memcpy(dst, src, bytes);
    }
}
}  // namespace miunet

namespace {

// `plane0` = index of the micro-batch's first plane in the call: plane i's window lives in slot plane0 + i (begin_window_call)
int stage_raw16(mi_unet *h, const uint16_t *const *raws, const int *widths, const int *heights, int bm, size_t plane0, hipStream_t s,
                uint8_t *d_tiles)
{
    const int C = h->cfg.in_ch;
    const size_t hw = (size_t)h->cfg.height * h->cfg.width;
    const mi_unet_window &win = h->window;
    const bool minmax = win.mode == MI_UNET_WINDOW_MINMAX, fixed = win.mode == MI_UNET_WINDOW_FIXED;
    int slot = mi_unet::RAW_RING - 1, mn_src = 0;
    for (int i = 0; i < bm * C; ++i) {
        const int w = widths[i], ht = heights[i];
        if (!raws[i] || w <= 0 || ht <= 0) return fail(MI_UNET_EARG, "RAW16 input: bad image description");
        const size_t n = (size_t)w * ht;
        if (n > h->raw_cap) {                    // grow the staging ring (outside any captured region)
            HIP_TRY(hipStreamSynchronize(s));
            h->raw_cap = 0;
            for (int r = 0; r < mi_unet::RAW_RING; ++r) {
                h->raw_busy[r] = false;
                HIP_TRY(h->d_raw[r].reset(n));
                HIP_TRY(h->h_raw[r].reset(n));
                if (!h->raw_done[r]) HIP_TRY(h->raw_done[r].reset(hipEventDisableTiming));
            }
            h->raw_cap = n;
        }
        // a caller holding one plane per image passes its pointer C times: upload and scan it once, resample it C times
        const bool same_plane = i % C != 0 && raws[i] == raws[i - 1] && w == widths[i - 1] && ht == heights[i - 1];
        if (!same_plane) {
            slot = (slot + 1) % mi_unet::RAW_RING;
            mn_src = i;
            if (h->raw_busy[slot]) { HIP_TRY(hipEventSynchronize(h->raw_done[slot])); h->raw_busy[slot] = false; }   // slot consumed
            // a caller that keeps its RAW images in pinned memory (mi_unet_host_alloc) skips the staging copy: the DMA engine
            // reads its buffer directly, the host thread only enqueues
            hipPointerAttribute_t attr;
            const bool pinned = hipPointerGetAttributes(&attr, raws[i]) == hipSuccess && attr.type == hipMemoryTypeHost;
            if (!pinned) {
                (void)hipGetLastError();             // an ordinary host pointer is "invalid value" to the query: not an error of ours
                host_copy(h, h->h_raw[slot], raws[i], n * sizeof(uint16_t));
            }
            HIP_TRY(hipMemcpyAsync(h->d_raw[slot], pinned ? raws[i] : h->h_raw[slot], n * sizeof(uint16_t), hipMemcpyHostToDevice, s));
        }
        const int r = slot;
        h->win_src[plane0 + i] = (int)(plane0 + mn_src);
        const unsigned *pair = h->d_mnmx + 2 * (plane0 + mn_src);
        uint8_t *dst = d_tiles + (size_t)(i / C) * hw * C + i % C;
        hipError_t e = same_plane ? hipSuccess : enqueue_window(h, h->d_raw[r], n, plane0 + mn_src, (size_t)mn_src, s);
        if (e == hipSuccess)
            e = minmax ? launch_resample_u8(h->d_raw[r], w, ht, pair, dst, h->cfg.width, h->cfg.height, C, s)
                       : launch_resample_u8_window(h->d_raw[r], w, ht, fixed ? nullptr : pair, win.lo, win.hi, dst, h->cfg.width,
                                                   h->cfg.height, C, s);
        if (e != hipSuccess) return fail(MI_UNET_EHIP, std::string("preprocess launch: ") + hipGetErrorString(e));
        HIP_TRY(hipEventRecord(h->raw_done[r], s));
        h->raw_busy[r] = true;
    }
    return 0;
}

int ensure_raw_pipeline(mi_unet *h, bool two_buffers, bool segment)
{
    if (!h->pre_stream) HIP_TRY(hipStreamCreateWithFlags(&h->pre_stream, hipStreamNonBlocking));
    if (!h->tail_stream) HIP_TRY(hipStreamCreateWithFlags(&h->tail_stream, hipStreamNonBlocking));
    if (!h->dl_stream) HIP_TRY(hipStreamCreateWithFlags(&h->dl_stream, hipStreamNonBlocking));
    const size_t npix = (size_t)h->cfg.max_batch * h->cfg.height * h->cfg.width;
    if (!h->d_labels2) HIP_TRY(h->d_labels2.reset(npix));
    for (int i = 0; i < 2; ++i) {
        for (Event *e : { &h->tiles_done[i], &h->net_done[i], &h->tile_ready[i], &h->out_done[i] })
            if (!*e) HIP_TRY(e->reset(hipEventDisableTiming));
        for (Event &e : h->tail_ev[i])
            if (!e) HIP_TRY(e.reset());
        for (Event &e : h->stage_ev[i])
            if (!e) HIP_TRY(e.reset());
    }
    for (int i = 0; i < 3; ++i)
        for (Event &e : h->pre_ev[i])
            if (!e) HIP_TRY(e.reset());
    if (two_buffers && !segment && !h->h_labels2) HIP_TRY(h->h_labels2.reset(npix));   // (segment calls download into h_multi)
    for (int i = 0; i < (two_buffers ? 2 : 1); ++i)
        if (!h->h_tiles[i]) HIP_TRY(h->h_tiles[i].reset(npix * h->cfg.in_ch));
    if (two_buffers && !h->d_img2) HIP_TRY(h->d_img2.reset(npix * h->cfg.in_ch));
    return 0;
}

// The RAW-in entry points as one loop over micro-batches.  Per micro-batch k on the engine's stream: network -> [postprocess ->
// mask_to_image -> contours] -> D2H; on the second stream, meanwhile: the host staging copies, H2D transfers and
// preprocessing kernels of micro-batch k + 1 into the other tile buffer.
struct RawCall {
    const uint16_t *const *raws; const int *widths, *heights; int B;
    uint8_t *tiles, *out_u8; float *logits;            // out_u8: label maps (infer) or 0 / 255 masks (segment)
    TargetTable targets;                               // segment: K >= 1 targets, out_u8 and the contour arrays are [B][K]...; K = 0: infer
    int32_t *xy; int cap_points; int32_t *start; int cap_contours; int32_t *counts;
};

int run_raw_call(mi_unet *h, const RawCall &c)
{
    HIP_TRY(hipSetDevice(h->cfg.device));
    const int H = h->cfg.height, W = h->cfg.width, Bm = h->cfg.max_batch;
    const size_t hw = (size_t)H * W, C = (size_t)h->cfg.in_ch;
    hipStream_t s = h->stream;
    if (c.B <= 0) return MI_UNET_OK;
    // segment: K planes per image behind the network, (image, target) pairs as the batch of every tail stage, in d_multi / h_multi;
    // infer: the label maps themselves, postprocessed in place for the reference's target when mi_unet_set_postprocess is on
    const bool segment = c.targets.K > 0;
    const TargetTable tab = segment ? c.targets : h->postprocess ? default_targets(H, W) : TargetTable{};
    const int K = segment ? tab.K : 1;
    // mi_unet_set_measure: the tail of every micro-batch also measures its regions, from the tile buffer the network read
    const bool measuring = segment && h->measure.on;
    if (measuring)
        if (int rc = check_measure_size(H, W, "RAW16 input")) return rc;
    // every image description is checked BEFORE anything is enqueued: a bad width in image k + 1 must not be found after the
    // network of micro-batch k has started
    unsigned long long max_samples = 0;
    for (size_t i = 0; i < (size_t)c.B * C; ++i) {
        if (!c.raws[i] || c.widths[i] <= 0 || c.heights[i] <= 0)
            return fail(MI_UNET_EARG, "RAW16 input: bad image description (image " + std::to_string(i / C) + ", plane " + std::to_string(i % C) + ")");
        max_samples = std::max(max_samples, (unsigned long long)c.widths[i] * (unsigned long long)c.heights[i]);
    }
    if (int rc = begin_window_call(h, (size_t)c.B * C, (size_t)Bm * C, max_samples, "RAW16 input")) return rc;
    // micro-batches: chunks of max_batch images -- and the FIRST chunk is cut once more when it is large (a quarter, at least
    // four images, then the rest), so that the network starts as soon as a few images have been uploaded and preprocessed
    // and the upload of the rest hides under it.
    struct MB { int b0, bm; };
    std::vector<MB> mbs;
    for (int b0 = 0; b0 < c.B; b0 += Bm) mbs.push_back({ b0, std::min(Bm, c.B - b0) });
    // MIUNET_RAW_SPLIT = 0: whole chunks only; "a" or "a,b,...": the first chunk is cut into a, b, ... images and the rest
    // (default: a quarter of the chunk, at least four, then the rest -- same-card sweep at 16 images: 0 -> 749, 2 -> 780, 4 -> 787,
    // 6 -> 737, 8 -> 779 images/s from pinned memory, tools/dev/split_sweep.py)
    // (h->raw_split, parsed at create)
    if (!(h->raw_split.size() == 1 && h->raw_split[0] == 0) && mbs[0].bm >= 8) {
        std::vector<int> cuts = h->raw_split;
        if (cuts.size() == 1 && cuts[0] < 0) cuts[0] = std::max(4, mbs[0].bm / 4);
        int left = mbs[0].bm, b0 = 0;
        std::vector<MB> parts;
        for (int cnt : cuts) {
            if (cnt <= 0 || cnt >= left) break;
            parts.push_back({ b0, cnt });
            b0 += cnt; left -= cnt;
        }
        parts.push_back({ b0, left });
        mbs.erase(mbs.begin());
        mbs.insert(mbs.begin(), parts.begin(), parts.end());
    }
    const int n_mb = (int)mbs.size();
    if (int rc = ensure_raw_pipeline(h, n_mb > 1, segment)) return rc;
    for (float &m : h->stage_ms) m = 0.f;
    auto tile_buf = [&](int k) { return (k & 1) ? h->d_img2.get() : h->d_img.get(); };
    auto out_buf = [&](int k) { return segment ? h->h_multi[k & 1].get() : (k & 1) ? h->h_labels2.get() : h->h_labels.get(); };
    auto stage = [&](int k) -> int {                   // upload + preprocess micro-batch k on the second stream
        const int bm = mbs[k].bm, par = k & 1;
        const size_t b0 = (size_t)mbs[k].b0;
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(h->pre_stream, c.tiles ? h->tiles_done[par].get() : h->net_done[par].get(), 0));   // its last readers: network and tile download of k - 2
        if (k >= 2 && measuring) HIP_TRY(hipStreamWaitEvent(h->pre_stream, h->out_done[par], 0));   // ... and, measuring, the tail of k - 2
        HIP_TRY(hipEventRecord(h->pre_ev[k % 3][0], h->pre_stream));
        if (int rc = stage_raw16(h, c.raws + b0 * C, c.widths + b0 * C, c.heights + b0 * C, bm, b0 * C, h->pre_stream, tile_buf(k))) return rc;
        HIP_TRY(hipEventRecord(h->pre_ev[k % 3][1], h->pre_stream));
        HIP_TRY(hipEventRecord(h->tile_ready[par], h->pre_stream));
        return 0;
    };
    auto enqueue = [&](int k) -> int {                 // micro-batch k: network on the engine's stream, everything behind it on the tail stream
        const int bm = mbs[k].bm, par = k & 1;
        const size_t b0 = (size_t)mbs[k].b0;
        uint8_t *d_tiles = tile_buf(k);
        uint8_t *d_lab = par ? h->d_labels2.get() : h->d_labels.get();
        hipStream_t ts = h->tail_stream;
        const ContourLayout cl{ bm * K, c.cap_points, c.cap_contours };
        if (segment && contour_workspace_bytes(bm * K, H, W, c.cap_contours) > h->tail_ws_bytes)
            return fail(MI_UNET_EARG, "contour workspace does not fit (cap_contours too large)");
        HIP_TRY(hipStreamWaitEvent(s, h->tile_ready[par], 0));
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(s, h->out_done[par], 0));                      // the tail of k - 2 has read this label buffer
        HIP_TRY(hipEventRecord(h->stage_ev[par][0], s));
        float *d_lg = c.logits ? h->d_logits.get() : nullptr;
        if (int rc = run_microbatch(h, d_tiles, bm, d_lab, d_lg)) return rc;                   // UNet + argmax
        HIP_TRY(hipEventRecord(h->stage_ev[par][1], s));
        if (c.logits)                                  // (a debugging output: into the caller's pageable memory, which blocks the host)
            HIP_TRY(hipMemcpyAsync(c.logits + b0 * hw * h->cfg.classes, h->d_logits, sizeof(float) * bm * hw * h->cfg.classes,
                                   hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(h->net_done[par], s));
        if (c.tiles) {                                 // the tiles leave on their own stream, beside the tail kernels
            HIP_TRY(hipStreamWaitEvent(h->dl_stream, h->net_done[par], 0));
            HIP_TRY(hipMemcpyAsync(h->h_tiles[par], d_tiles, bm * hw * C, hipMemcpyDeviceToHost, h->dl_stream));
            HIP_TRY(hipEventRecord(h->tiles_done[par], h->dl_stream));
        }
        // ---- tail: ordered behind the network of k, concurrent with the network of k + 1
        HIP_TRY(hipStreamWaitEvent(ts, h->net_done[par], 0));
        Event *tv = h->tail_ev[par];
        HIP_TRY(hipEventRecord(tv[0], ts));
        uint8_t *d_result = segment ? h->d_multi.get() : d_lab;
        const MeasureArgs ma{ d_tiles, par };
        if (int rc = enqueue_tail(h, d_lab, bm, H, W, tab, d_result, h->d_tail_ws, segment ? &cl : nullptr, tv[1], ts, std::string(),
                                  measuring ? &ma : nullptr))
            return rc;
        HIP_TRY(hipEventRecord(tv[2], ts));
        HIP_TRY(hipMemcpyAsync(out_buf(k), d_result, bm * K * hw, hipMemcpyDeviceToHost, ts));
        if (segment)
            if (int rc = contours_to_pinned(h, cl, ts, par)) return rc;
        if (k == n_mb - 1)                             // every plane of the call has been staged in front of this network: its windows leave too
            if (int rc = enqueue_window_download(h, (size_t)c.B * C, ts)) return rc;
        HIP_TRY(hipEventRecord(tv[3], ts));
        HIP_TRY(hipEventRecord(h->out_done[par], ts));
        return 0;
    };
    auto finalize = [&](int k) -> int {                // micro-batch k has left the device: pinned halves -> the caller's arrays
        const int bm = mbs[k].bm, par = k & 1;
        const size_t b0 = (size_t)mbs[k].b0;
        if (c.tiles) {                                 // (done long before the tail: copied out while the tail still runs)
            HIP_TRY(hipEventSynchronize(h->tiles_done[par]));
            host_copy(h, c.tiles + b0 * hw * C, h->h_tiles[par], bm * hw * C);
        }
        HIP_TRY(hipEventSynchronize(h->out_done[par]));
        host_copy(h, c.out_u8 + b0 * K * hw, out_buf(k), bm * K * hw);
        if (segment)
            contours_to_caller(h, ContourLayout{ bm * K, c.cap_points, c.cap_contours }, c.xy + b0 * K * c.cap_points * 2,
                               c.start + b0 * K * (c.cap_contours + 1), c.counts + b0 * K, par);
        if (measuring) regions_to_report(h, RegionLayout{ bm * K, c.cap_contours }, (int)b0 * K, par);
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->pre_ev[k % 3][0], h->pre_ev[k % 3][1]));
        h->stage_ms[MI_UNET_STAGE_UPLOAD_PRE] += ms;
        HIP_TRY(hipEventElapsedTime(&ms, h->stage_ev[par][0], h->stage_ev[par][1]));
        h->stage_ms[MI_UNET_STAGE_NETWORK] += ms;
        for (int st = 0; st < 3; ++st) {
            HIP_TRY(hipEventElapsedTime(&ms, h->tail_ev[par][st], h->tail_ev[par][st + 1]));
            h->stage_ms[MI_UNET_STAGE_POSTPROCESS + st] += ms;
        }
        return 0;
    };
    // MIUNET_RAW_TRACE=1: host-side timeline of the call on stderr (when did each enqueue / staging / copy-out start and end)
    const bool trace = h->raw_trace;
    const auto t_call = std::chrono::steady_clock::now();
    auto mark = [&](const char *what, int k) {
        if (trace) fprintf(stderr, "[raw %8.3f ms] %s %d\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(), what, k);
    };
    {
        int bmax = 0;
        for (const MB &m : mbs) bmax = std::max(bmax, m.bm);
        size_t need = postprocess_workspace_bytes(bmax * K, H, W);
        if (segment) {
            if (int rc = grow_contour_buffers(h, ContourLayout{ bmax * K, c.cap_points, c.cap_contours })) return rc;
            // (nothing of an earlier call is in flight: every RAW-in call drains its streams before it returns)
            if (measuring)
                if (int rc = grow_region_buffers(h, RegionLayout{ bmax * K, c.cap_contours })) return rc;
            begin_region_call(h, measuring, c.B * K, c.cap_contours);
            need = std::max(need, contour_workspace_bytes(bmax * K, H, W, c.cap_contours));
        }
        if (int rc = ensure_tail_buffers(h, need, segment ? (size_t)bmax * K * hw : 0)) return rc;
    }
    // Once the first micro-batch is enqueued, H2D copies read the caller's (possibly page-locked) RAW buffers directly and the tail
    // writes the handle's pinned mirrors: an error return with work still in flight would let the caller free buffers under the
    // DMA engine.  Every failure path below therefore drains ALL four streams before the call returns.
    auto pipeline = [&]() -> int {
        HIP_TRY(hipStreamSynchronize(s));                  // an external stream may still be reading the tile buffers
        mark("stage begin", 0);
        if (int rc = stage(0)) return rc;
        mark("stage end", 0);
        for (int k = 0; k < n_mb; ++k) {
            if (int rc = enqueue(k)) return rc;
            mark("enqueued", k);
            if (k + 1 < n_mb) {                            // the host's staging copies of k + 1 run while the device works on k
                if (int rc = stage(k + 1)) return rc;
                mark("stage end", k + 1);
            }
            if (k >= 1) {
                if (int rc = finalize(k - 1)) return rc;   // ... and so does the copy-out of k - 1
                mark("finalized", k - 1);
            }
        }
        if (int rc = finalize(n_mb - 1)) return rc;
        mark("finalized", n_mb - 1);
        HIP_TRY(hipStreamSynchronize(s));                  // D2H copies into the caller's own (pageable) logits included
        return MI_UNET_OK;
    };
    const int rc = pipeline();
    if (rc != MI_UNET_OK) {
        const std::string keep = engine_last_error();
        for (hipStream_t q : { h->pre_stream, s, h->tail_stream, h->dl_stream })
            if (q) (void)hipStreamSynchronize(q);
        for (int i = 0; i < mi_unet::RAW_RING; ++i) h->raw_busy[i] = false;
        return fail(rc, keep);
    }
    finish_window_call(h, (size_t)c.B * C);
    if (segment) finish_region_call(h);
    mark("done", 0);
    return MI_UNET_OK;
}

}  // namespace

extern "C" {

int mi_unet_infer_raw16(mi_unet_t *h, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                        uint8_t *tiles, uint8_t *labels, float *logits)
{
    if (int rc = check_handle(h, true)) return rc;
    if (!raws || !widths || !heights || !labels || B < 0) return fail(MI_UNET_EARG, "mi_unet_infer_raw16: bad argument");
    return run_raw_call(h, RawCall{ raws, widths, heights, B, tiles, labels, logits, TargetTable{}, nullptr, 0, nullptr, 0, nullptr });
}

// mi_unet_segment_raw16 (the reference's target, whatever the handle's setting) and its _multi form (the handle's targets)
static int segment_raw16_call(mi_unet_t *h, const char *name, bool multi, const uint16_t *const *raws, const int *widths, const int *heights,
                              int B, uint8_t *tiles, uint8_t *masks, int32_t *xy, int cap_points, int32_t *start, int cap_contours, int32_t *counts)
{
    if (int rc = check_handle(h, true)) return rc;
    if (!raws || !widths || !heights || !masks || !xy || !start || !counts || B < 0 || cap_points <= 0 || cap_contours <= 0)
        return fail(MI_UNET_EARG, std::string("mi_unet_") + name + ": bad argument");
    const int H = h->cfg.height, W = h->cfg.width;
    if (multi)
        if (int rc = check_morph_list(h, (std::string("mi_unet_") + name).c_str())) return rc;
    const TargetTable tab = multi ? target_table(h, H, W) : default_targets(H, W);
    if ((size_t)std::min(B, h->cfg.max_batch) * tab.K * H * W > 0x7FFFFFFFull)
        return fail(MI_UNET_EARG, std::string(name) + ": max_batch x targets x height x width exceeds 2^31 - 1");
    return run_raw_call(h, RawCall{ raws, widths, heights, B, tiles, masks, nullptr, tab, xy, cap_points, start, cap_contours, counts });
}

int mi_unet_segment_raw16(mi_unet_t *h, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                          uint8_t *tiles, uint8_t *masks, int32_t *xy, int cap_points, int32_t *start, int cap_contours,
                          int32_t *counts)
{
    return segment_raw16_call(h, "segment_raw16", false, raws, widths, heights, B, tiles, masks, xy, cap_points, start, cap_contours, counts);
}

int mi_unet_segment_raw16_multi(mi_unet_t *h, const uint16_t *const *raws, const int *widths, const int *heights, int B,
                                uint8_t *tiles, uint8_t *masks, int32_t *xy, int cap_points, int32_t *start, int cap_contours,
                                int32_t *counts)
{
    return segment_raw16_call(h, "segment_raw16_multi", true, raws, widths, heights, B, tiles, masks, xy, cap_points, start, cap_contours, counts);
}

int mi_unet_last_stage_ms(const mi_unet_t *h, float *ms)
{
    if (!h || !ms) return fail(MI_UNET_EARG, "mi_unet_last_stage_ms: null argument");
    for (int i = 0; i < MI_UNET_N_STAGES; ++i) ms[i] = h->stage_ms[i];
    return MI_UNET_OK;
}

}  // extern "C"
